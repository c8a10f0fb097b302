"""The montage fine-flow stage without a GPU: the per-pair restatement and
`stitch_elastic.aggregate_arrays` on host arrays against the reference's own
output (tests/golden/tile_flows.npz), and the argument checks of
`filter_flow_maps` that come before any device use."""
import numpy as np
import pytest

from tests import tile_flows_ref as ref


def test_restatement_matches_reference_golden(golden):
  g = golden('tile_flows')
  n = 0
  for mname, d, pname, flows, clean, rec, want in ref.filter_cases(g):
    before = {k: v.copy() for k, v in flows.items()}
    got = ref.filter_flow_maps(flows, clean, rec)
    assert list(got) == list(want)
    for k in want:
      assert ref.same(got[k], want[k]), (mname, d, pname, k)
      assert ref.same(flows[k], before[k])
    n += len(want)
  assert n >= 150


def test_golden_covers_the_contract(golden):
  """What the generator asserts about the fixture, as far as the file shows it."""
  g = golden('tile_flows')
  cases = list(ref.filter_cases(g))
  chans = {v.shape[0] for _, _, _, flows, *_ in cases for v in flows.values()}
  assert chans == {2, 4}
  shapes = {v.shape[1:] for _, _, _, flows, *_ in cases for v in flows.values()}
  assert len(shapes) > 8 and (1, 1) in shapes
  by = {(m, d, p): (flows, want) for m, d, p, flows, _, _, want in cases}
  # thresholds <= 0 switch every test off
  for (m, d, p), (flows, want) in by.items():
    if p == 'nonpos':
      for k, v in flows.items():
        assert ref.same(want[k], v[:2])
  # a float64 threshold that float32 cannot hold decides differently
  flows, py = by['m3x2', 'x', 'py_edge']
  _, f64 = by['m3x2', 'x', 'f64_edge']
  for y, x in ((1, 1), (3, 2), (1, 3)):    # magnitude, sharpness, ratio
    assert not np.isnan(py[1, 0][:, y, x]).any() and np.isnan(f64[1, 0][:, y, x]).all()
  _, py = by['m3x2', 'x', 'py_rdev_edge']
  _, f64 = by['m3x2', 'x', 'f64_rdev_edge']
  assert not np.isnan(py[1, 0][:, 3, 0]).any() and np.isnan(f64[1, 0][:, 3, 0]).all()
  # the quirk pair: one partially NaN vector, min_patch_size 3 -> fully NaN
  flows, want = by['m2x2', 'x', 'patch']
  assert np.isnan(flows[0, 1][:2, 2, 3]).sum() == 1 and np.isnan(want[0, 1][:, 2, 3]).all()
  assert np.isnan(want[0, 1]).sum() == 2
  # the padding example of the gradient: 18 border vectors on the pair's own extent
  flows, want = by['m3x2', 'x', 'grad']
  assert flows[0, 1].shape == (2, 6, 5) and np.isnan(want[0, 1][0]).sum() == 18


@pytest.mark.parametrize('name', ['m2x2', 'm3x2', 'm4x1', 'mnone', 'm3d'])
def test_aggregate_arrays_matches_reference_golden(golden, name):
  from sofima_amd import stitch_elastic
  m = ref.montage(golden('tile_flows'), name)
  for fn in (stitch_elastic.aggregate_arrays, ref.aggregate_arrays):
    fx, fy, x, nbors, idx = fn(*ref.aggregate_args(m))
    for got, want in zip((fx, fy, x, nbors), m['want']):
      assert ref.same(got, want), (name, fn.__module__)
    assert fx.dtype == np.float64 and x.dtype == np.float32 and nbors.dtype == np.int64
    assert idx == m['want_idx'] and list(idx) == list(m['want_idx'])
  if name == 'mnone':
    assert fx.shape == fy.shape == (2, 2, 1, 1) and np.isnan(fx).all()
    assert (nbors == -1).all()
  if name == 'm3d':
    assert nbors.shape == (3, 4, 11) and fx.ndim == 5


def test_aggregate_arrays_initialises_no_device(golden, monkeypatch):
  import torch
  from sofima_amd import _abi, _dev, stitch_elastic

  def boom(*a, **k):
    raise AssertionError('aggregate_arrays touched the device')

  monkeypatch.setattr(_dev, 'device', boom)
  monkeypatch.setattr(_abi, 'load', boom)
  monkeypatch.setattr(torch.cuda, 'is_available', boom)
  monkeypatch.setattr(torch.cuda, '_lazy_init', boom)
  m = ref.montage(golden('tile_flows'), 'm3x2')
  fx, *_ = stitch_elastic.aggregate_arrays(*ref.aggregate_args(m))
  assert ref.same(fx, m['want'][0])


@pytest.mark.parametrize('shape', [(3, 4, 5), (2, 1, 4, 5), (4, 1, 4, 5), (2, 0, 5), (4, 3, 0),
                                   (5, 3, 3), (2, 7)])
def test_filter_flow_maps_rejects_before_any_device_use(monkeypatch, shape):
  from sofima_amd import _abi, _dev, stitch_elastic

  def boom(*a, **k):
    raise AssertionError('filter_flow_maps touched the device before checking its input')

  monkeypatch.setattr(_dev, 'device', boom)
  monkeypatch.setattr(_abi, 'load', boom)
  good = np.zeros((2, 3, 3), np.float32)
  with pytest.raises(ValueError):
    stitch_elastic.filter_flow_maps({(0, 0): good, (1, 0): np.zeros(shape, np.float32)},
                                    reconcile=dict(max_gradient=1, max_deviation=1,
                                                   min_patch_size=1))
