"""map_utils.compose_maps and the cross-block reconcile without a device: the
SciPy restatement reproduces the goldens of the unmodified reference, the
brute-force contract checker accepts the reference itself, the C entry points
and their argument checks, and the block ranges of the reconcile."""
import ctypes
import os
import re

import numpy as np
import pytest

from sofima_amd import _abi, _build
from tests import compose_maps_scipy as cms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'compose_maps_tri.npz')
GOLDEN_XBLOCK = os.path.join(ROOT, 'tests', 'golden', 'reconcile_cross_block.npz')
ENTRY_POINTS = ('sfm_compose_maps_tri_workspace_bytes', 'sfm_compose_maps_tri')


def golden_cases():
  g = np.load(GOLDEN)
  n = len([k for k in g.files if k.endswith('_name')])
  for i in range(n):
    k = f'{i:02d}'
    s = g[k + '_strides']
    yield (str(g[k + '_name']), g[k + '_map1'], cms.box(*g[k + '_box1']), float(s[0]),
           g[k + '_map2'], cms.box(*g[k + '_box2']), float(s[1]), g[k + '_out'])


CASES = list(golden_cases())
AFFINE = [c for c in CASES if 'affine' in c[0]]


def test_the_goldens_hold_the_cases():
  names = [c[0] for c in CASES]
  for name in ('generic', 'generic_holes', 'affine', 'affine_holes', 'generic_holes_f32',
               'affine_holes_f32', 'affine_holes_f32_f64', 'generic_holes_f64_f32',
               'affine_holes_f32_far', 'boxes_strides', 'boxes_strides_affine', 'map1_nan_inf',
               'map2_nan_channel1', 'map1_zero', 'hole_query', 'one_quad', 'three_corners',
               'two_valid', 'collinear', 'multi_slice'):
    assert name in names
  assert len(AFFINE) >= 5


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_restatement_reproduces_the_goldens(case):
  pytest.importorskip('scipy')
  _, m1, b1, s1, m2, b2, s2, want = case
  got = cms.compose_restated(m1, b1, s1, m2, b2, s2)
  assert got.dtype == want.dtype == m1.dtype and got.shape == m1.shape
  assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_reference_is_admissible(case):
  """The checker on the reference alone: every golden value is the interpolant
  of an admissible triangle (1e-6 for float64, plus two float32 spacings for a
  float32 map1), NaN exactly where none exists, and with an affine map2 every
  query in the hull has one admissible value."""
  pytest.importorskip('scipy')
  name, m1, b1, s1, m2, b2, s2, want = case
  counts = cms.check_contract(m1, b1, s1, m2, b2, s2, want, want)
  if name in ('two_valid', 'collinear'):
    assert counts['in_hull'] == 0 and np.isnan(want).all()
  else:
    assert counts['in_hull'] > 0
  if 'affine' in name:
    assert counts['single'] == counts['in_hull']
  if name == 'map1_nan_inf':
    assert counts['queries'] == want[0].size - 4
  if name == 'hole_query':
    assert np.isfinite(want[:, 0, 2:4, 3:5]).all()


def test_tolerance():
  b = cms.box((0, 0, 0), (2, 2, 1))
  z64, z32 = np.zeros((2, 1, 2, 2)), np.zeros((2, 1, 2, 2), np.float32)
  assert cms.tolerance(z64, b, 4, z32, b, 4) == 1e-6
  # the largest absolute coordinate is 4: two spacings of 2^-21
  assert cms.tolerance(z32, b, 4, z64, b, 4) == 1e-6 + 2 * 2.0**-21
  far = cms.box((500, 0, 0), (2, 2, 1))
  assert cms.tolerance(z32, b, 4, z64, far, 4) == 1e-6 + 2 * 2.0**-13


def test_bd_cells_on_one_quad():
  """The documented diagonal: from (i, j + 1) to (i + 1, j)."""
  b2 = cms.box((0, 0, 0), (2, 2, 1))
  m2 = np.zeros((2, 1, 2, 2))
  m2[0, 0, 1, 1] = 4.0                         # corner c alone is displaced
  b1 = cms.box((1, 1, 0), (1, 1, 1))
  m1 = np.zeros((2, 1, 1, 1))                  # the query (1, 1): below the diagonal x + y = 2
  val, mask = cms.bd_cells(m1, b1, 1, m2, b2, 2)
  assert mask.all() and val[0, 0, 0, 0] == 0.0
  m1[:] = 0.5                                  # (1.5, 1.5): in b-c-d, a quarter of c's weight
  val, mask = cms.bd_cells(m1, b1, 1, m2, b2, 2)
  assert mask.all() and val[0, 0, 0, 0] == 0.5 + 0.5 * 4.0


# -- the cross-block reconcile: block ranges ------------------------------------


def test_block_ranges_match_the_reference():
  from sofima_amd import processor_maps
  g = np.load(GOLDEN_XBLOCK)
  sorted_z = sorted(int(k) for k, _ in g['z_map'])
  for z, s, e in g['z_range_of']:
    assert processor_maps._get_z_range(sorted_z, int(z)) == (int(s), int(e))
  for name in g['names']:
    start, size = g[f'{name}_box']
    got = processor_maps.block_ranges(sorted_z, int(start[2]), int(start[2] + size[2]))
    assert got == [tuple(int(v) for v in r) for r in g[f'{name}_ranges']]
  assert processor_maps.block_ranges([0, 4, 8], 0, 9) == [(0, 0), (0, 4), (4, 8)]
  assert processor_maps.block_ranges([0, 4, 8], 2, 7) == [(0, 4), (4, 8)]


def test_cross_block_golden_is_not_nan_alone():
  g = np.load(GOLDEN_XBLOCK)
  sorted_z = sorted(int(k) for k, _ in g['z_map'])
  for name in g['names']:
    out, z0 = g[f'{name}_out'], int(g[f'{name}_box'][0][2])
    for k in range(out.shape[1]):
      if z0 + k not in sorted_z:
        assert np.isfinite(out[:, k]).all(axis=0).mean() >= 0.55 and np.isnan(out[:, k]).any()


# -- the C entry points -------------------------------------------------------


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_struct_layout_matches_header():
  body = re.search(r'typedef struct SfmComposeTriDesc \{(.*?)\} SfmComposeTriDesc;', _header(),
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    for part in decl.split(','):
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$',
                             part.strip()).group(1))
  d = _abi.SfmComposeTriDesc
  assert names == [f[0] for f in d._fields_]
  # ten ints, two doubles, the two flags, then seven pointer-sized members
  assert d.stride1.offset == 40 and d.f64_1.offset == 56 and d.f64_2.offset == 60
  assert d.map1.offset == 64 and ctypes.sizeof(d) == 64 + 7 * 8


def test_entry_points_and_version(lib):
  text = _header()
  assert re.search(r'\bsize_t sfm_compose_maps_tri_workspace_bytes\s*\(', text)
  assert re.search(r'\bint sfm_compose_maps_tri\s*\(', text)
  for name in ENTRY_POINTS:
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1)) == 9
  comment = re.search(r'#define SFM_ABI_VERSION 9\s*/\*(.*?)\*/', open(HEADER).read(),
                      re.S).group(1)
  for name in ENTRY_POINTS:
    assert name in comment


def _desc(shape1, shape2, stride1=4.0, stride2=4.0):
  d = _abi.SfmComposeTriDesc()
  d.shape1 = (ctypes.c_int32 * 3)(*shape1)
  d.shape2 = (ctypes.c_int32 * 3)(*shape2)
  d.stride1, d.stride2 = stride1, stride2
  return d


def _armed(*args, **kwargs):
  d = _desc(*args, **kwargs)
  d.map1, d.map2, d.status = 1024, 2048, 4096
  return d


def test_workspace_query(lib):
  query = lib.sfm_compose_maps_tri_workspace_bytes
  sizes = [query(ctypes.byref(_desc(s1, s2))) for s1, s2 in (
      ((1, 1, 1), (1, 2, 2)), ((1, 3, 4), (1, 5, 7)), ((1, 30, 40), (1, 5, 7)),
      ((1, 30, 40), (1, 50, 70)), ((9, 30, 40), (1, 50, 70)), ((9, 30, 40), (9, 50, 70)),
      ((64, 101, 101), (64, 101, 101)))]
  assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
  # per query a key, a quantized position and a list entry; per node of map2 a
  # double2 and an int64 pair
  assert sizes[1] >= 28 * 12 + 32 * 35
  assert sizes[-1] >= 64 * 101 * 101 * (28 + 32)
  assert query(None) == 0
  assert query(ctypes.byref(_desc((0, 3, 4), (1, 5, 7)))) == 0
  assert query(ctypes.byref(_desc((1, 3, 4), (1, 5, 0)))) == 0


def test_rejections_before_any_launch(lib):
  """Every argument error returns its code without a launch: no device needed."""
  call = lib.sfm_compose_maps_tri
  out = ctypes.c_void_p(8192)
  assert call(None, None) == -1
  assert b'NULL' in lib.sfm_last_error()
  for field in ('map1', 'map2', 'status'):
    d = _armed((1, 3, 4), (1, 5, 7))
    setattr(d, field, None)
    assert call(ctypes.byref(d), out) == -1
    assert b'NULL' in lib.sfm_last_error()
  assert call(ctypes.byref(_armed((1, 3, 4), (1, 5, 7))), None) == -1
  assert b'NULL' in lib.sfm_last_error()
  for s1, s2 in (((0, 3, 4), (1, 5, 7)), ((1, 3, -1), (1, 5, 7)), ((1, 3, 4), (1, 0, 7)),
                 ((1, 3, 4), (0, 5, 7))):
    assert call(ctypes.byref(_armed(s1, s2)), out) == -1
    assert b'bad shape' in lib.sfm_last_error()
  for bad in (0.0, -1.0, float('inf'), float('nan')):
    for field in ('stride1', 'stride2'):
      d = _armed((1, 3, 4), (1, 5, 7))
      setattr(d, field, bad)
      assert call(ctypes.byref(d), out) == -1
      assert b'strides' in lib.sfm_last_error()
  assert call(ctypes.byref(_armed((1, 3, 4), (1, 2048, 1025))), out) == -1   # 2^21 + 2048 nodes
  assert b'2^21' in lib.sfm_last_error()
  assert call(ctypes.byref(_armed((1024, 3, 4), (1024, 2048, 1024))), out) == -1
  assert b'2^31' in lib.sfm_last_error()
  assert call(ctypes.byref(_armed((2, 40000, 40000), (2, 3, 4))), out) == -1   # 2^31 queries
  assert b'2^31' in lib.sfm_last_error()
  assert call(ctypes.byref(_armed((3, 3, 4), (2, 5, 7))), out) == -1
  assert b'z slices' in lib.sfm_last_error()
  d = _armed((3, 3, 4), (1, 5, 7))                       # one shared slice: accepted so far
  assert call(ctypes.byref(d), out) == -3                # SFM_ERR_WORKSPACE
  assert b'workspace' in lib.sfm_last_error()
  need = lib.sfm_compose_maps_tri_workspace_bytes(ctypes.byref(d))
  d.workspace, d.workspace_bytes = 16384, need - 1
  assert call(ctypes.byref(d), out) == -3
