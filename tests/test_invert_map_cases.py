"""Host checks of tests/invmap_cases.py: every case tests what it claims, the
references agree with each other, and the committed E_ref table is reproduced."""
import os
import re

import numpy as np
import pytest

from tests import invert_map_scipy as ims
from tests import invmap_cases as ic

pytest.importorskip('scipy')

CONTRACT = ic.names_expecting('contract')
AFFINE = ic.names_expecting('affine')
SMALL_AFFINE = [n for n in AFFINE if n not in ic.LARGE_AFFINE]
REFUSED = ic.names_expecting('refused')
ALL_NAN = ic.names_expecting('all_nan')


def _brute_full(valid):
  h, w = valid.shape
  out = np.zeros((h - 1, w - 1), bool)
  for i in range(h - 1):
    for j in range(w - 1):
      out[i, j] = valid[i, j] and valid[i, j + 1] and valid[i + 1, j] and valid[i + 1, j + 1]
  return out


def _brute_boundary(valid):
  h, w = valid.shape
  full = _brute_full(valid)
  n = 0
  for i in range(h):
    for j in range(w):
      if not valid[i, j]:
        continue
      quads = [(i - 1, j - 1), (i - 1, j), (i, j - 1), (i, j)]
      inner = all(0 <= a < h - 1 and 0 <= b < w - 1 and full[a, b] for a, b in quads)
      n += not inner
  return n


TINY = {
    'full_4x5': np.ones((4, 5), bool),
    'hole_and_notch': np.array([[1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1],
                                [1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1]], bool),
    'checker_5x5': (np.add.outer(np.arange(5), np.arange(5)) % 2 == 0),
}


@pytest.mark.parametrize('name', list(TINY))
def test_boundary_count_and_full_quads_against_a_loop(name):
  valid = TINY[name]
  assert np.array_equal(ic.full_quads(valid), _brute_full(valid))
  assert ic.boundary_count(valid) == _brute_boundary(valid)
  if name == 'full_4x5':
    assert ic.boundary_count(valid) == 14
  if name == 'checker_5x5':
    assert ic.boundary_count(valid) == 13 and not ic.full_quads(valid).any()


def _slice_points(pos, valid, k):
  return np.stack([pos[0, k][valid[k]], pos[1, k][valid[k]]], axis=1)


@pytest.mark.parametrize('name', CONTRACT + ALL_NAN)
def test_contract_cases_hold_their_claims(name):
  _, cm, src, dst, stride, expect = ic.case(name)
  pos, _, qry, (sy, sx) = ims.slice_geometry(cm, src, dst, stride)
  valid = np.all(np.isfinite(pos), axis=0)
  want = ims.invert_restated(cm, src, dst, stride)
  if expect == 'all_nan':
    assert np.isnan(want).all()
  claim = ic.CLAIMS.get(name)
  if claim is None:
    return
  q = np.stack([qry[1].ravel(), qry[0].ravel()], axis=1).astype(np.float64)
  for k in range(cm.shape[1]):
    assert int(valid[k].sum()) == claim['nvalid'][k], k
    assert (not ic.full_quads(valid[k]).any()) == claim['r_empty'][k], k
    if 'boundary' in claim:
      assert ic.boundary_count(valid[k]) == claim['boundary'][k], k
    if claim['degenerate'][k]:
      # fewer than three nodes, collinear or coincident: Qhull has no answer
      assert np.isnan(want[:, k]).all(), k
      continue
    assert np.isfinite(want[:, k]).any(), k
    if k in claim['on_hull']:
      continue
    # no query within 1e-3 px of the hull: the NaN masks must agree exactly
    near = ic.in_hull(_slice_points(pos, valid, k), q, 1e-3) == 0
    assert not near.any(), (k, int(near.sum()))


def test_the_mixes_cover_every_degenerate_kind():
  for mix in (ic.MIX_37, ic.MIX_300):
    kinds = set(mix.values())
    assert {'empty', 'one', 'two', 'row', 'coincident', 'three', 'four22'} <= kinds
  # a wave of 64 lanes spans several slices, and the second init workgroup runs
  assert 5 * 7 < 64 and 3 * 3 * 7 < 64 and 300 > 256 and (2 - 1) * (40 - 1) < 64


def _affine_error(name):
  _, cm, src, dst, stride, _ = ic.case(name)
  claim = ic.CLAIMS[name]
  want = ic.affine_inverse(claim['A'], claim['t'], src, dst, stride)
  valid = ic.valid_nodes(cm, src, dst, stride)[0]
  pts = ic.affine_points(claim['A'], claim['t'], valid, src, stride)
  side = ic.in_hull(pts, ic.dst_queries(dst, stride), 1e-7 * stride).reshape(want.shape[2:])
  return want, side


@pytest.mark.parametrize('name', AFFINE)
def test_affine_cases_hold_their_claims(name):
  _, cm, src, dst, stride, _ = ic.case(name)
  claim = ic.CLAIMS[name]
  valid = ic.valid_nodes(cm, src, dst, stride)[0]
  assert ic.boundary_count(valid) == claim['boundary'][0] <= ic.MAX_B
  assert int(valid.sum()) == claim['nvalid'][0]
  assert float(stride) == int(stride)
  want, side = _affine_error(name)
  # the queries that may be either NaN or finite stay below 1 %
  assert (side == 0).mean() < 0.01
  assert (side > 0).any() and (side < 0).any()
  # the map really is the affine image of the lattice
  pos = ims.slice_geometry(cm, src, dst, stride)[0]
  pts = ic.affine_points(claim['A'], claim['t'], valid, src, stride)
  frame = np.array([dst.start[0], dst.start[1]]) * float(stride)
  got = np.stack([pos[0, 0][valid], pos[1, 0][valid]], axis=1) + frame
  assert np.abs(got - pts).max() <= 4 * np.spacing(claim['max_coord'])
  tol = ic.affine_tolerance(name, claim['max_coord'])
  assert 64 * np.spacing(claim['max_coord']) <= tol <= 1e-6


def test_the_cap_cases_sit_on_the_cap():
  for name in ('cap_strip_7936', 'cap_strip_two_holes_7936', 'cap_band_7936'):
    ic.case(name)
    assert ic.CLAIMS[name]['boundary'] == [ic.MAX_B]
  ic.case('cap_strip_one_hole_7937')
  assert ic.CLAIMS['cap_strip_one_hole_7937']['boundary'] == [ic.MAX_B + 1]
  assert not ic.CLAIMS['cap_band_7936']['r_empty'][0]
  _, cm, src, dst, stride, _ = ic.case('status_cap_1_fold_2')
  valid = ic.valid_nodes(cm, src, dst, stride)
  assert [ic.boundary_count(v) for v in valid] == ic.CLAIMS['status_cap_1_fold_2']['boundary']


def test_node_id_cases_sit_on_the_width():
  _, cm, _, _, _, _ = ic.case('nodeid_2p21')
  assert cm.shape[2] * cm.shape[3] == 1 << ic.NODE_BITS
  valid = np.isfinite(cm[0, 0])
  # blobs whose jagged rims need completion triangles at both ends of the id range
  assert not valid[0, 0] and not valid[-1, -1] and valid[8, 0] and valid[-9, -1]
  assert not valid[-1, -160:].any() and valid[-8, -160:].any()


@pytest.mark.parametrize('name', SMALL_AFFINE)
def test_affine_cases_match_the_restatement(name):
  """The source of invmap_cases.E_REF: the SciPy statement against the analytic
  inverse on the queries inside the hull."""
  _, cm, src, dst, stride, _ = ic.case(name)
  ref = ims.invert_restated(cm, src, dst, stride)
  want, side = _affine_error(name)
  inside = side > 0
  assert np.isfinite(ref[:, 0][:, inside]).all()
  assert np.isnan(ref[:, 0][:, side < 0]).all()
  err = float(np.abs(ref[:, 0] - want[:, 0])[:, inside].max())
  print(f'{name}: E_ref {err:.3e} (committed {ic.E_REF[name]:.3e})')
  assert err <= ic.E_REF[name]
  assert 16 * ic.E_REF[name] <= 1e-6


@pytest.mark.parametrize('name', ['status_fold_1_4', 'status_cap_1_fold_2'])
def test_fold_cases_have_a_non_positive_triangle(name):
  _, cm, src, dst, stride, expect = ic.case(name)
  pos = ims.slice_geometry(cm, src, dst, stride)[0]
  folds = [k for k in range(cm.shape[1]) if ic.has_fold(pos[:, k])]
  assert folds == ic.CLAIMS[name]['folds']
  assert expect[0] == 'refused' and re.compile(expect[1])


def test_disjoint_boxes_are_far_from_the_map():
  for name in ALL_NAN:
    if not name.startswith('disjoint'):
      continue
    _, cm, src, dst, stride, _ = ic.case(name)
    d = np.array(dst.start[:2]) - np.array(src.start[:2])
    assert sorted(np.abs(d)) == [0, 100000] and dst.size[:2] == (64, 64)


def test_golden_cases_need_no_exception_on_the_host():
  """The SciPy statement against the reference's own output needs neither
  exception, so the device tests can assert a diagonal count of 0."""
  g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                           'invert_map.npz'))
  n = len([k for k in g.files if k.endswith('_name')])
  for i in range(n):
    k = f'{i:02d}'
    cm, src, dst = g[k + '_map'], ims.box(*g[k + '_src']), ims.box(*g[k + '_dst'])
    stride = tuple(float(v) for v in g[k + '_stride'])
    got = ims.invert_restated(cm, src, dst, stride)
    counts = ims.check_contract_counts(cm, src, dst, stride, got, g[k + '_out'])
    assert counts == (0, 0), (str(g[k + '_name']), counts)
