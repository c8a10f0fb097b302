"""Host side of processor_flow: the NumPy restatement of EstimateMissingFlow's
loop, driven by the CPU oracle's flow_field, against what the reference
produced (tests/golden/missing_flow.npz), and the box arithmetic against the
boxes the reference derived."""
import numpy as np
import pytest

from oracle import flow_oracle
from sofima_amd import processor_flow
from tests import missing_flow_ref as ref

CASES = ('fwd', 'bwd')


@pytest.fixture(scope='module')
def fixture(golden):
  return golden('missing_flow')


@pytest.mark.parametrize('name', CASES)
def test_restatement_with_the_oracle_equals_the_reference(fixture, name):
  cfg = ref.config(fixture, name)
  flow, images, kw = ref.case_kwargs(fixture, cfg, name)
  trace = []
  got, filled = ref.estimate_missing_flow_np(flow, images, flow_oracle.flow_field, trace=trace,
                                             **kw)
  want = fixture[name + '_out']
  assert got.dtype == np.float32 and got.shape == want.shape
  assert np.array_equal(np.isnan(got), np.isnan(want))
  assert np.array_equal(got[2], want[2])
  assert np.array_equal(got[:2], want[:2], equal_nan=True)
  assert np.array_equal(filled, fixture[name + '_filled'])
  # what the cases are there for
  events = {e for _, _, e in trace}
  assert np.isnan(want[0]).any() and (filled.sum(0) > 0).sum() >= 2
  assert ('break-stack' if name == 'fwd' else 'masked-prev') in events
  assert np.all(want[2][np.isnan(want[0])] == cfg['delta_z'])


@pytest.mark.parametrize('name', CASES)
def test_geometry_of_the_flow_cases(fixture, name):
  cfg = ref.config(fixture, name)
  start, size = fixture[name + '_box']
  volume = fixture['images'].shape[::-1]
  keys = {k: cfg[k] for k in ref.GEOMETRY_KEYS}
  want = {k: fixture[f'{name}_geo_{k}'] for k in ref.geometry_np(start, size, volume, **keys)}
  for got in (ref.geometry_np(start, size, volume, **keys),
              ref.geometry_as_dict(processor_flow.missing_flow_geometry(start, size, volume,
                                                                        **keys))):
    for k, v in want.items():
      assert np.array_equal(got[k], v), (k, got[k], v)
  assert np.array_equal(fixture[name + '_out_box'], [want['out_start'], want['out_size']])


def test_geometry_of_the_clipped_boxes(fixture):
  cfg = ref.config(fixture, 'clip')
  keys = {k: cfg[k] for k in ref.GEOMETRY_KEYS}
  volume = fixture['images'].shape[::-1]
  unchanged = fixture['clip_unchanged']
  assert unchanged.sum() == 1 and len(unchanged) == 4
  for i, (start, size) in enumerate(fixture['clip_boxes']):
    mine = processor_flow.missing_flow_geometry(start, size, volume, **keys)
    restated = ref.geometry_np(start, size, volume, **keys)
    if unchanged[i]:
      assert mine is None and restated is None
      continue
    mine = ref.geometry_as_dict(mine)
    for k in restated:
      want = fixture[f'clip{i}_geo_{k}']
      assert np.array_equal(mine[k], want), (i, k, mine[k], want)
      assert np.array_equal(restated[k], want), (i, k, restated[k], want)
    assert np.any(mine['out_size'] != size)          # the box was cut


def test_geometry_is_integers_and_slices():
  g = processor_flow.missing_flow_geometry((2, 2, 5), (2, 2, 1), (128, 128, 10), patch_size=16,
                                           stride=16, search_radius=16, delta_z=1, max_delta_z=2)
  # processor/flow_test.py:94-95: flow (2, 2, 5) is image (32, 32, 5)
  assert g.out_start == (2, 2, 5) and g.out_size == (2, 2, 1)
  assert g.load_start == (8, 8, 3) and g.load_size == (64, 64, 3) and g.z0 == 2
  assert g.curr_slice == (slice(16, 48), slice(16, 48))
  assert g.flow_slice == (slice(0, 2), slice(0, 2))
  assert all(type(v) is int for v in g.out_start + g.load_size)
  # its clipped twin (:150): one section of context instead of five
  g = processor_flow.missing_flow_geometry((2, 2, 1), (2, 2, 1), (128, 128, 10), patch_size=16,
                                           stride=16, search_radius=16, delta_z=1, max_delta_z=5)
  assert g.load_start == (8, 8, 0) and g.load_size == (64, 64, 2) and g.z0 == 1


@pytest.mark.parametrize('patch_size, stride, search_radius', [(30, 16, 8), (32, 16, 4)])
def test_patch_that_is_no_multiple_of_the_stride_is_refused(patch_size, stride, search_radius):
  with pytest.raises(ValueError, match='not a multiple'):
    processor_flow.missing_flow_geometry((0, 0, 0), (4, 4, 1), (200, 200, 4),
                                         patch_size=patch_size, stride=stride,
                                         search_radius=search_radius, delta_z=1, max_delta_z=2)
  with pytest.raises(ValueError, match='not a multiple'):
    processor_flow.estimate_missing_flow(
        np.zeros((2, 1, 2, 2), np.float32), np.zeros((3, 64, 64), np.uint8),
        patch_size=patch_size, stride=stride, delta_z=1, max_delta_z=2, max_attempts=1,
        search_radius=search_radius, min_peak_ratio=0, min_peak_sharpness=0, max_magnitude=0)


def test_pair_order_of_estimate_flow():
  """processor/flow.py:213-229."""
  assert processor_flow.flow_pairs(5, 1) == [(0, 1), (1, 2), (2, 3), (3, 4)]
  assert processor_flow.flow_pairs(5, -2) == [(2, 0), (3, 1), (4, 2)]
  assert processor_flow.flow_pairs(5, 1, True) == [(0, 4), (1, 4), (2, 4), (3, 4)]
  assert processor_flow.flow_pairs(5, -1, True) == [(1, 0), (2, 0), (3, 0), (4, 0)]
  for args in ((5, 1, False), (5, -2, False), (5, 2, True), (5, -2, True)):
    assert processor_flow.flow_pairs(*args) == ref.flow_pairs_np(*args)
  assert processor_flow.search_deltas(1, 4) == ref.search_deltas(1, 4) == [2, 3, 4]
  assert processor_flow.search_deltas(-1, -3) == ref.search_deltas(-1, -3) == [-2, -3]
