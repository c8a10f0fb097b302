"""Host side of processor_mesh.prev_state / relax_sections: the section plan
against the (flow, ref z) pairs the reference loaded, and the claims the GPU
tests lean on, asserted again from tests/golden/prev_state.npz."""
import types

import numpy as np
import pytest

from oracle import mesh_oracle
from sofima_amd import processor_mesh
from tests import prev_state_ref as ref

CASES = ('fwd', 'bwd')


@pytest.fixture(scope='module')
def fixture(golden):
  return golden('prev_state')


@pytest.mark.parametrize('name', CASES)
def test_refs_for_section_equals_the_pairs_the_reference_loaded(fixture, name):
  case = ref.Case(fixture, name)
  flows = case.flow_volumes()
  assert len(case.sections) >= 5
  for z in case.sections:
    got = processor_mesh.refs_for_section(z, flows, case.block_starts, case.backward, case.skip)
    if not case.has_prev(z):
      assert got is None, z
    else:
      assert got == case.pairs(z), z


def test_refs_for_section_keeps_a_flow_whose_lookbacks_all_leave_the_block():
  """processor/mesh.py:353-364: such a flow still counts as a reference, so the
  section gets an (all NaN) state, not None."""
  flow = np.zeros((3, 3, 2, 2), np.float32)
  flow[2] = 2.0                                  # z = 1 looks back to z = -1
  fv = processor_mesh.FlowVolume(flow, 1)
  assert processor_mesh.refs_for_section(1, [fv], [0]) == []
  assert processor_mesh.refs_for_section(0, [fv], [0]) is None
  flow[2, 1, 0, 0] = 1.5                         # fractions, 0 and NaN name no section
  flow[2, 1, 0, 1] = np.nan
  flow[2, 1, 1, 0] = 0.0
  flow[2, 1, 1, 1] = 1.0
  assert processor_mesh.refs_for_section(1, [fv], [0]) == [(0, 0)]


@pytest.mark.parametrize('name', CASES)
def test_fixture_stays_clear_of_the_fold_thresholds(fixture, name):
  case = ref.Case(fixture, name)
  stride = case.cfg['stride']
  masked_more = False
  for z in case.sections:
    if not case.has_prev(z):
      continue
    avg, prev = case.rec(z, 'avg'), case.rec(z, 'prev')
    assert avg.dtype == np.float64 and prev.dtype == np.float64
    margin = ref.threshold_margin(avg, stride, case.min_frac, case.max_frac)
    assert margin > ref.composition_tolerance(avg), (z, margin)
    # prev is mask_irregular of the average, in float64
    want = avg.copy()
    ref.mask_irregular_np(want, stride, case.min_frac, case.max_frac, dilation_iters=1)
    np.testing.assert_array_equal(want.view(np.uint64), prev[:, 0].view(np.uint64))
    masked_more |= bool(np.isnan(prev).sum() > np.isnan(avg).sum())
  assert masked_more        # mask_irregular has something to do


@pytest.mark.parametrize('name', CASES)
def test_fixture_covers_counts_and_lookbacks(fixture, name):
  case = ref.Case(fixture, name)
  f = case.flow_arrays
  vals = f[2][2]
  assert np.isnan(vals).any()
  assert set(np.abs(vals[np.isfinite(vals)]).astype(int)) == {0, 1, 2, 3}
  count0 = count2 = False
  used = set()
  for z in case.sections:
    if not case.has_prev(z):
      continue
    n_ref = np.zeros(vals.shape[1:], int)
    for i, rz in case.pairs(z):
      if i < 2:
        n_ref += np.isfinite(f[i][0, z])
      else:
        n_ref += f[2][2, z] == z - rz
        used.add(abs(z - rz))
    count0 |= bool((np.isnan(case.rec(z, 'avg')[0]) & (n_ref == 0)).any())
    count2 |= bool((n_ref >= 2).any())
  assert count0 and count2 and used >= {1, 2, 3}


@pytest.mark.parametrize('name', CASES)
def test_fixture_outcomes_do_not_hinge_on_prev_within_the_tolerance(fixture, name):
  """Steps, status and NaN pattern of the three-pass driver (the CPU oracle,
  itself pinned to the reference by test_oracle_golden) stay what the reference
  recorded when prev moves by the composition tolerance."""
  case = ref.Case(fixture, name)
  cfg = types.SimpleNamespace(**case.cfg)
  for k, v in dict(fire=True, f_alpha=0.99, f_inc=1.1, f_dec=0.5, alpha=0.1, n_min=5,
                   cap_scale=1.1, cap_upscale_every=100, remove_drift=False).items():
    if not hasattr(cfg, k):
      setattr(cfg, k, v)
  cfg.stride = tuple(cfg.stride)
  rng = np.random.default_rng(3)
  solved = 0
  for z in case.sections:
    if int(case.rec(z, 'status')) == int(processor_mesh.SolutionStatus.UNDEFINED):
      assert int(case.rec(z, 'steps')) == 0 and not case.rec(z, 'x').any()
      continue
    solved += 1
    prev = case.rec(z, 'prev')
    noise = rng.choice([-1.0, 1.0], size=prev.shape) * (2e-5 + 1e-5 * np.abs(prev))
    mask = None if case.mask is None else case.mask[z:z + 1]
    x, _, steps, status = mesh_oracle.relax_mesh_passes(
        np.zeros(prev.shape, np.float32), (prev + noise).astype(np.float32), cfg, mask,
        case.min_frac)
    assert steps == int(case.rec(z, 'steps')) and status == int(case.rec(z, 'status')), z
    np.testing.assert_array_equal(np.isnan(x), np.isnan(case.rec(z, 'x')))
  assert solved >= 3


def test_relax_sections_refuses_a_first_section_that_is_no_block_start():
  flows = [processor_mesh.FlowVolume(np.zeros((2, 6, 3, 4), np.float32), 1)]
  kw = dict(block_starts=[0, 4], mesh_min_frac=0.5, mesh_max_frac=1.5)
  with pytest.raises(ValueError, match='block start'):
    processor_mesh.relax_sections(flows, None, sections=[1, 2], **kw)
  with pytest.raises(ValueError, match='block start'):
    processor_mesh.relax_sections(flows, None, backward=True, **kw)   # starts at z = 5
