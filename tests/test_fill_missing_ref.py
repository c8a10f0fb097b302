"""tests/fill_missing_ref.py, the brute-force statement of what the device
computes, against the reference's own results (tests/golden/fill_missing.npz):
bit for bit wherever the nearest valid node is unique and on every node that is
not filled; on a tied node the value of one of the equidistant candidates (the
reference's pick there is an artefact of SciPy's k-d tree)."""
import numpy as np
import pytest

from tests import fill_missing_ref
from tests.fill_missing_ref import bits, cases


def test_fixture_holds_the_cases_of_the_issue(golden):
  cs = {c['name']: c for c in cases(golden('fill_missing'))}
  assert cs['rot_rect_f32']['map'].shape == (2, 3, 23, 31)
  assert np.isnan(cs['rot_rect_f32']['map'][:, 1]).all()
  assert np.isfinite(cs['rot_rect_f32']['map'][:, 2]).all()
  assert cs['ellipsoid_f32']['map'].shape == (3, 9, 14, 17)
  assert cs['sparse3d_f32']['map'].shape == (3, 9, 14, 17)
  assert cs['rot_rect_f64']['map'].dtype == np.float64
  assert np.isinf(cs['inf_2d_f32']['map']).any()
  assert cs['rot_rect_to_zero']['kw']['invalid_to_zero']
  assert cs['inverse_map_shell_f64']['map'].shape[0] == 3
  for c in cs.values():
    if c['filled'].any():
      assert c['unique'].sum() >= 0.6 * c['filled'].sum(), c['name']
      assert not (c['unique'] & ~c['filled']).any()


def test_brute_force_equals_the_reference(golden):
  for c in cases(golden('fill_missing')):
    m, want = c['map'], c['out']
    before = m.copy()
    got = fill_missing_ref.fill_missing_ref(m, **c['kw'])
    np.testing.assert_array_equal(bits(m), bits(before))
    assert got.dtype == want.dtype and got.shape == want.shape
    tied = c['filled'] & ~c['unique']
    settled = np.broadcast_to(~tied, m.shape)
    np.testing.assert_array_equal(bits(got)[settled], bits(want)[settled], err_msg=c['name'])
    if not tied.any():
      continue
    dim = m.shape[0]
    for node in np.argwhere(tied):
      # the problem of the node: its slice, or the volume
      if dim == 2:
        src, res, p_shape = m[:, node[0]], want[:, node[0]], node[1:]
      else:
        src, res, p_shape = m, want, node
      valid = np.isfinite(src).all(axis=0)
      p = np.ravel_multi_index(tuple(p_shape), valid.shape)
      cands = fill_missing_ref.tied_candidates(valid, p)
      assert len(cands) >= 2
      vals = bits(src).reshape(dim, -1)
      ref_val = bits(res).reshape(dim, -1)[:, p]
      assert any(np.array_equal(vals[:, k], ref_val) for k in cands), (c['name'], node)
      # ... and the statement took the lowest index of them
      assert np.array_equal(bits(got[(slice(None),) + tuple(node)]), vals[:, cands.min()])


def test_tie_rule_and_edges_of_the_statement():
  m = np.full((2, 1, 1, 5), np.nan, np.float32)
  m[:, 0, 0, 0] = (1, 2)
  m[:, 0, 0, 4] = (3, 4)
  got = fill_missing_ref.fill_missing_ref(m, extrapolate=True, interpolate_first=False)
  np.testing.assert_array_equal(got[0, 0, 0], [1, 1, 1, 3, 3])   # the middle: the lower x
  np.testing.assert_array_equal(got[1, 0, 0], [2, 2, 2, 4, 4])
  with pytest.raises(NotImplementedError):
    fill_missing_ref.fill_missing_ref(m)
  whole = np.ones((3, 1, 2, 2))
  whole[0, 0, 0, 0] = np.inf
  np.testing.assert_array_equal(fill_missing_ref.fill_missing_ref(whole), whole)
  none = np.full((2, 2, 2, 2), np.nan)
  none[:, 1] = 7
  none[0, 0, 0, 0] = np.inf
  got = fill_missing_ref.fill_missing_ref(none, extrapolate=True, interpolate_first=False)
  assert np.isnan(got[:, 0]).all() and (got[:, 1] == 7).all()
  got = fill_missing_ref.fill_missing_ref(none, extrapolate=True, invalid_to_zero=True,
                                          interpolate_first=False)
  assert (got[:, 0] == 0).all()
  got = fill_missing_ref.fill_missing_ref(none, interpolate_first=False)
  np.testing.assert_array_equal(bits(got), bits(none))
