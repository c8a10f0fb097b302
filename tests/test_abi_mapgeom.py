"""The map geometry entry points: ctypes structs in the header's field order, the
four calls exported, and the version the library reports is the header's."""
import os
import re

import pytest

from sofima_amd import _abi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
ENTRY_POINTS = ('sfm_map_shift', 'sfm_map_extents', 'sfm_affine_map', 'sfm_warp_points')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize('cname', ['SfmMapShiftDesc', 'SfmMapExtentsDesc', 'SfmAffineMapDesc',
                                   'SfmWarpPointsDesc'])
def test_struct_layouts_match_header(cname):
  body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (cname, cname), _header(),
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    for part in decl.split(','):
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$',
                             part.strip()).group(1))
  assert names == [f[0] for f in getattr(_abi, cname)._fields_]


def test_entry_points_and_version(lib):
  text = _header()
  for name in ENTRY_POINTS:
    assert re.search(r'\bint %s\s*\(' % name, text), name
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1))
  consts = dict(re.findall(r'#define (SFM_(?:SHIFT|EXTENTS|POINT)_\w+) (\d+)', text))
  assert int(consts['SFM_SHIFT_TO_RELATIVE']) == _abi.SHIFT_TO_RELATIVE
  assert int(consts['SFM_EXTENTS_INNER']) == _abi.EXTENTS_INNER
  assert [int(consts['SFM_POINT_' + k]) for k in ('F32', 'F64', 'I32', 'I64')] == [
      _abi.POINT_F32, _abi.POINT_F64, _abi.POINT_I32, _abi.POINT_I64]
  ws = re.search(r'#define SFM_MAP_EXTENTS_WORKSPACE_BYTES \((.*?)\)', text).group(1)
  assert eval(ws) == _abi.MAP_EXTENTS_WORKSPACE_BYTES   # a product of integer literals


def test_null_descriptors_are_rejected(lib):
  for name in ENTRY_POINTS:
    assert getattr(lib, name)(None) == -1
    assert b'NULL' in lib.sfm_last_error()
