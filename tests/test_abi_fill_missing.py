"""The fill_missing entry point: the ctypes struct in the header's field order, the
two calls exported and listed in the version comment, the workspace query."""
import ctypes
import os
import re

import pytest

from sofima_amd import _abi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
ENTRY_POINTS = ('sfm_fill_missing_nearest_workspace_bytes', 'sfm_fill_missing_nearest')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_struct_layout_matches_header():
  body = re.search(r'typedef struct SfmFillMissingDesc \{(.*?)\} SfmFillMissingDesc;', _header(),
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    for part in decl.split(','):
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$',
                             part.strip()).group(1))
  assert names == [f[0] for f in _abi.SfmFillMissingDesc._fields_]
  # ncomp, f64, shape[3], two flags: 7 ints, padded to the pointers
  assert _abi.SfmFillMissingDesc.coord_map.offset == 32
  assert ctypes.sizeof(_abi.SfmFillMissingDesc) == 32 + 6 * 8


def test_entry_points_version_and_limit(lib):
  text = _header()
  assert re.search(r'\bsize_t sfm_fill_missing_nearest_workspace_bytes\s*\(', text)
  assert re.search(r'\bint sfm_fill_missing_nearest\s*\(', text)
  for name in ENTRY_POINTS:
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1)) == 9
  comment = re.search(r'#define SFM_ABI_VERSION 9\s*/\*(.*?)\*/', open(HEADER).read(),
                      re.S).group(1)
  for name in ENTRY_POINTS:
    assert name in comment
  assert int(re.search(r'#define SFM_FILL_MISSING_MAX_AXIS (\d+)', text).group(1)) == \
      _abi.FILL_MISSING_MAX_AXIS


def _desc(ncomp, shape):
  d = _abi.SfmFillMissingDesc()
  d.ncomp = ncomp
  d.shape = (ctypes.c_int32 * 3)(*shape)
  return d


def test_workspace_query_and_rejections(lib):
  query = lib.sfm_fill_missing_nearest_workspace_bytes
  small = query(ctypes.byref(_desc(3, (2, 3, 4))))
  big = query(ctypes.byref(_desc(3, (130, 74, 74))))
  # two int32 source indices per node and the per-problem flags
  assert 2 * 4 * 24 <= small < big
  assert 2 * 4 * 130 * 74 * 74 <= big <= 2 * 4 * 130 * 74 * 74 + 1024
  assert query(ctypes.byref(_desc(2, (64, 410, 410)))) >= 2 * 4 * 64 * 410 * 410 + 4 * 64
  assert query(None) == 0
  assert query(ctypes.byref(_desc(4, (2, 3, 4)))) == 0
  assert query(ctypes.byref(_desc(2, (0, 3, 4)))) == 0
  assert query(ctypes.byref(_desc(2, (1, _abi.FILL_MISSING_MAX_AXIS + 1, 4)))) == 0
  assert query(ctypes.byref(_desc(2, (1, _abi.FILL_MISSING_MAX_AXIS, 4)))) > 0
  assert query(ctypes.byref(_desc(3, (16384, 16384, 8)))) == 0       # 2^31 nodes
  assert lib.sfm_fill_missing_nearest(None) == -1
  assert b'NULL' in lib.sfm_last_error()
  # checked before anything is launched: no device needed
  d = _desc(3, (2, 3, 4))
  d.coord_map, d.out, d.has_nan = 1024, 4096, 8192
  d.ncomp = 5
  assert lib.sfm_fill_missing_nearest(ctypes.byref(d)) == -1
  assert b'ncomp' in lib.sfm_last_error()
  d.ncomp = 3
  d.shape[2] = _abi.FILL_MISSING_MAX_AXIS + 1
  assert lib.sfm_fill_missing_nearest(ctypes.byref(d)) == -1
  assert b'16384' in lib.sfm_last_error()
  d.shape[2] = 4
  assert lib.sfm_fill_missing_nearest(ctypes.byref(d)) == -3         # SFM_ERR_WORKSPACE
  assert b'workspace' in lib.sfm_last_error()
