"""The batched tile-pair filter at the C boundary: the ctypes struct in the
header's field order, both calls declared, bound and exported, and the entry
point's rejections (host arithmetic only: nothing here needs a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from sofima_amd import _abi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
ENTRY_POINTS = ('sfm_filter_tile_flows', 'sfm_filter_tile_flows_max_nodes')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_struct_layout_matches_header():
  body = re.search(r'typedef struct SfmTileFlowsDesc \{(.*?)\} SfmTileFlowsDesc;', _header(),
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if decl:
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$', decl).group(1))
  assert names == [f[0] for f in _abi.SfmTileFlowsDesc._fields_]


def test_entry_points_and_version(lib):
  text = _header()
  for name in ENTRY_POINTS:
    assert re.search(r'\bint %s\s*\(' % name, text), name
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  # the change only adds symbols
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1))


def test_max_nodes(lib):
  cap = lib.sfm_filter_tile_flows_max_nodes()
  assert cap >= 8192
  # two float channels and one int per vector fit the 160 KB of LDS of a CU
  assert cap * 12 <= 160 * 1024 < (cap + 64) * 12


def _desc(extents, channels=2, padded=None, n=None):
  ext = np.ascontiguousarray(extents, np.int32).reshape(-1, 2)
  d = _abi.SfmTileFlowsDesc()
  d.channels = channels
  d.n = len(ext) if n is None else n
  d.padded_shape = (ctypes.c_int32 * 2)(*(padded or ext.max(axis=0)))
  d.extents = ext.ctypes.data
  # never dereferenced by a call that is rejected
  d.extents_device = 1
  d.flows = 1
  d.do_clean = d.do_reconcile = 1
  return d, ext


def test_rejections_carry_a_message(lib):
  assert lib.sfm_filter_tile_flows(None, None) == -1
  assert b'NULL' in lib.sfm_last_error()
  d, keep = _desc([(3, 4)])
  assert lib.sfm_filter_tile_flows(ctypes.byref(d), None) == -1
  assert b'NULL' in lib.sfm_last_error()
  d.extents = None
  assert lib.sfm_filter_tile_flows(ctypes.byref(d), 1) == -1
  assert b'NULL' in lib.sfm_last_error()
  cap = lib.sfm_filter_tile_flows_max_nodes()
  for kwargs, word in ((dict(extents=[(3, 4)], channels=3), b'channels'),
                       (dict(extents=[(3, 4)], channels=5), b'channels'),
                       (dict(extents=[(3, 4), (0, 4)]), b'extent'),
                       (dict(extents=[(3, 4), (3, -1)]), b'extent'),
                       (dict(extents=[(3, 4), (5, 4)], padded=(4, 4)), b'extent'),
                       (dict(extents=[(3, 4), (3, 5)], padded=(3, 4)), b'extent'),
                       (dict(extents=[(3, 4)], padded=(0, 4)), b'padded'),
                       (dict(extents=[(3, 4)], n=-1), b'batch size'),
                       (dict(extents=[(2, 2), (cap // 64 + 1, 64)]), b'vectors')):
    d, keep = _desc(**kwargs)
    assert lib.sfm_filter_tile_flows(ctypes.byref(d), 1) == -1, kwargs
    assert word in lib.sfm_last_error(), (kwargs, lib.sfm_last_error())
  # an empty batch is no launch
  d, keep = _desc([(3, 4)], n=0)
  assert lib.sfm_filter_tile_flows(ctypes.byref(d), 1) == 0
