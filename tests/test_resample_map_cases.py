"""map_utils.resample_map without a device: the SciPy restatement reproduces the
goldens of the unmodified reference, the brute-force contract checker accepts
the reference itself, the nearest rule of the upsampling epilogue against
SciPy, and the C entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from sofima_amd import _abi, _build, processor_flow
from tests import resample_map_scipy as rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'resample_map.npz')
ENTRY_POINTS = ('sfm_resample_map_workspace_bytes', 'sfm_resample_map')


def golden_cases():
  g = np.load(GOLDEN)
  n = len([k for k in g.files if k.endswith('_name')])
  for i in range(n):
    k = f'{i:02d}'
    s = g[k + '_strides']
    yield (str(g[k + '_name']), g[k + '_map'], rms.box(*g[k + '_src']), rms.box(*g[k + '_dst']),
           float(s[0]), float(s[1]), g[k + '_out'])


CASES = list(golden_cases())


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_restatement_reproduces_the_goldens(case):
  pytest.importorskip('scipy')
  _, cm, src, dst, s0, s1, want = case
  got = rms.resample_restated(cm, src, dst, s0, s1)
  assert got.dtype == want.dtype == cm.dtype
  assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c[0])
def test_reference_is_admissible(case):
  """The checker on the reference alone: every golden value is the interpolant
  of an admissible triangle, and NaN exactly where none exists."""
  pytest.importorskip('scipy')
  name, cm, src, dst, s0, s1, want = case
  # (a float32 golden is its float64 value rounded: 1.2e-7 at |v| < 4)
  counts, _ = rms.check_contract(cm, src, dst, s0, s1, want, want, hull_exception=False)
  if name != 'dst_disjoint':
    assert counts['in_hull'] > 0
  # nodes and cell edges at the least: all triangulations agree somewhere
  assert counts['single'] > 0 or counts['in_hull'] == 0


def test_admissible_values_of_one_quad():
  """A unit square: both diagonals are admissible at the centre, one value on
  the edges, none outside."""
  pos = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float64)
  val = np.array([[0, 0], [1, 0], [0, 1], [5, 1]], np.float64)
  qry = np.array([[.5, .5], [.5, 0], [.25, .5], [1.5, .5]])
  adm = rms.admissible_values(np.ones(4, bool), val, pos, qry)
  assert sorted(set(np.round(adm[0][:, 0], 12))) == [0.5, 2.5]
  assert np.ptp(adm[1][:, 0]) < 1e-12 and abs(adm[1][0, 0] - .5) < 1e-12
  assert sorted(set(np.round(adm[2][:, 0], 12))) == [0.25, 1.25]
  assert len(adm[3]) == 0


@pytest.mark.parametrize('n,start,scale,q_start,q_n', [
    (6, 2, 0.5, 3, 12),          # halfway queries: ties
    (5, -3, 0.25, -14, 30),      # negative starts, queries beyond both ends
    (4, 0, 1 / 3, -2, 15),       # a scale that is not exact in binary
    (7, 1, 0.5, 0, 20),
    (2, 5, 0.5, 9, 5),           # the smallest grid SciPy takes
])
def test_nearest_nodes_against_scipy(n, start, scale, q_start, q_n):
  interpolate = pytest.importorskip('scipy.interpolate')
  idx, outside = processor_flow.nearest_nodes(n, start, scale, q_start, q_n)
  grid = ((np.arange(n) + start) / scale).ravel()
  other = np.array([0.0, 1.0])
  rgi = interpolate.RegularGridInterpolator(
      (grid, other), np.stack([np.arange(n, dtype=np.float64)] * 2, 1), method='nearest',
      bounds_error=False)
  q = np.arange(q_n) + q_start
  want = rgi((q[:, None], np.zeros((1, 1))))[:, 0]
  assert np.array_equal(np.isnan(want), outside)
  assert np.array_equal(want[~outside], idx[~outside])
  if scale == 0.5:
    # a query halfway between two nodes reads the lower one
    half = (~outside) & ((q - start / scale) % 2 == 1)
    assert half.any() and np.array_equal(idx[half], ((q[half] * scale - start) // 1))


def test_nearest_nodes_single_node():
  idx, outside = processor_flow.nearest_nodes(1, 3, 0.5, 4, 5)
  assert idx.tolist() == [0] * 5 and outside.tolist() == [True, True, False, True, True]


# -- the C entry points -------------------------------------------------------


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_struct_layout_matches_header():
  body = re.search(r'typedef struct SfmResampleMapDesc \{(.*?)\} SfmResampleMapDesc;', _header(),
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    for part in decl.split(','):
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$',
                             part.strip()).group(1))
  d = _abi.SfmResampleMapDesc
  assert names == [f[0] for f in d._fields_]
  # nine ints padded to the doubles, the flag padded to the pointers
  assert d.src_stride.offset == 40 and d.f64.offset == 56 and d.coord_map.offset == 64
  assert ctypes.sizeof(d) == 64 + 5 * 8


def test_entry_points_and_version(lib):
  text = _header()
  assert re.search(r'\bsize_t sfm_resample_map_workspace_bytes\s*\(', text)
  assert re.search(r'\bint sfm_resample_map\s*\(', text)
  for name in ENTRY_POINTS:
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1)) == 9
  comment = re.search(r'#define SFM_ABI_VERSION 9\s*/\*(.*?)\*/', open(HEADER).read(),
                      re.S).group(1)
  for name in ENTRY_POINTS:
    assert name in comment


def _desc(shape, dst_shape, src_stride=2.0, dst_stride=1.0):
  d = _abi.SfmResampleMapDesc()
  d.shape = (ctypes.c_int32 * 3)(*shape)
  d.dst_shape = (ctypes.c_int32 * 2)(*dst_shape)
  d.src_stride, d.dst_stride = src_stride, dst_stride
  return d


def test_workspace_query_and_rejections(lib):
  query = lib.sfm_resample_map_workspace_bytes
  small = query(ctypes.byref(_desc((1, 3, 4), (5, 7))))
  big = query(ctypes.byref(_desc((64, 101, 101), (201, 201))))
  # a double2 and an int64 pair per node, an 8-byte key per query
  assert 32 * 12 + 8 * 35 <= small < big
  assert big >= 64 * (32 * 101 * 101 + 8 * 201 * 201)
  # the engine's own layout: the same bytes as an inversion of these shapes
  inv = _abi.SfmInvertMapDesc()
  inv.shape = (ctypes.c_int32 * 3)(64, 101, 101)
  inv.dst_shape = (ctypes.c_int32 * 2)(201, 201)
  assert lib.sfm_invert_map_workspace_bytes(ctypes.byref(inv)) == big
  assert query(None) == 0
  assert query(ctypes.byref(_desc((0, 3, 4), (5, 7)))) == 0
  assert query(ctypes.byref(_desc((1, 3, 4), (-1, 7)))) == 0
  assert query(ctypes.byref(_desc((1, 3, 4), (0, 7)))) > 0

  call = lib.sfm_resample_map
  assert call(None, None) == -1
  assert b'NULL' in lib.sfm_last_error()
  # checked before anything is launched: no device needed
  d = _desc((1, 3, 4), (5, 7))
  d.coord_map, d.status = 1024, 4096
  assert call(ctypes.byref(d), None) == -1             # an output lattice without an output
  assert b'NULL' in lib.sfm_last_error()
  out = ctypes.c_void_p(8192)
  d.shape[1] = 0
  assert call(ctypes.byref(d), out) == -1
  assert b'bad shape' in lib.sfm_last_error()
  d.shape[1] = 3
  d.dst_shape[0] = -1
  assert call(ctypes.byref(d), out) == -1
  assert b'output shape' in lib.sfm_last_error()
  d.dst_shape[0] = 5
  for bad in (0.0, -1.0, float('inf'), float('nan')):
    for field in ('src_stride', 'dst_stride'):
      e = _desc((1, 3, 4), (5, 7))
      e.coord_map, e.status = 1024, 4096
      setattr(e, field, bad)
      assert call(ctypes.byref(e), out) == -1
      assert b'strides' in lib.sfm_last_error()
  e = _desc((1, 2048, 1025), (5, 7))                   # 2^21 + 2048 nodes per slice
  e.coord_map, e.status = 1024, 4096
  assert call(ctypes.byref(e), out) == -1
  assert b'2^21' in lib.sfm_last_error()
  e = _desc((1024, 2048, 1024), (5, 7))                # 2^31 nodes
  e.coord_map, e.status = 1024, 4096
  assert call(ctypes.byref(e), out) == -1
  assert b'2^31' in lib.sfm_last_error()
  e = _desc((2, 3, 4), (40000, 40000))                 # 2^31 queries
  e.coord_map, e.status = 1024, 4096
  assert call(ctypes.byref(e), out) == -1
  assert b'2^31' in lib.sfm_last_error()
  assert call(ctypes.byref(d), out) == -3              # SFM_ERR_WORKSPACE
  assert b'workspace' in lib.sfm_last_error()
  d.workspace, d.workspace_bytes = 16384, small - 1
  assert call(ctypes.byref(d), out) == -3
