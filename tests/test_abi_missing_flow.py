"""The missing-flow entry points: ctypes structs in the header's field order,
the two calls exported, NULL arguments and bad shapes rejected."""
import ctypes as C
import os
import re

import pytest

from sofima_amd import _abi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
ENTRY_POINTS = ('sfm_flow_select', 'sfm_missing_flow_update')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize('cname', ['SfmFlowSelectDesc', 'SfmMissingFlowDesc'])
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


def test_struct_sizes():
  # LP64, natural alignment: the offsets the C side computes
  s = _abi.SfmFlowSelectDesc
  assert (s.selection.offset, s.pre_counts.offset, s.pre_max_masked.offset) == (16, 40, 56)
  assert (s.post_counts.offset, s.positions.offset, C.sizeof(s)) == (80, 96, 120)
  m = _abi.SfmMissingFlowDesc
  assert (m.field.offset, m.out.offset, m.min_peak_ratio.offset) == (16, 24, 64)
  assert (m.delta_z.offset, m.filled.offset, C.sizeof(m)) == (88, 96, 112)


def test_entry_points_and_version(lib):
  text = _header()
  for name in ENTRY_POINTS:
    assert re.search(r'\bint %s\s*\(' % name, text), name
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1))


def _select(**kw):
  d = _abi.SfmFlowSelectDesc()
  d.grid = (C.c_int32 * 2)(4, 6)
  d.batch_size = 5
  d.capacity = 25
  d.selection = d.positions = d.counts = 8       # never dereferenced on the host
  d.selection_pitch = 6
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def _update(**kw):
  d = _abi.SfmMissingFlowDesc()
  d.shape = (C.c_int32 * 2)(4, 6)
  d.field_shape = (C.c_int32 * 2)(4, 6)
  d.field = d.mask = d.attempts = d.filled = 8
  d.out = (C.c_void_p * 3)(8, 8, 8)
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def test_null_and_malformed_descriptors_are_rejected(lib):
  """Argument checks run on the host, before anything is launched."""
  for fn in (lib.sfm_flow_select, lib.sfm_missing_flow_update):
    assert fn(None) == -1
    assert b'NULL' in lib.sfm_last_error()
  for kw in (dict(selection=None), dict(positions=None), dict(counts=None)):
    assert lib.sfm_flow_select(C.byref(_select(**kw))) == -1, kw
    assert b'NULL' in lib.sfm_last_error()
  counts = dict(pre_counts=8, pre_grid=(C.c_int32 * 2)(4, 6), pre_pitch=6, pre_area=16)
  for kw, word in ((dict(grid=(C.c_int32 * 2)(0, 6)), b'grid'),
                   (dict(grid=(C.c_int32 * 2)(1 << 16, 1 << 16)), b'grid'),
                   (dict(batch_size=0), b'batch'),
                   (dict(selection_pitch=5), b'pitch'),
                   (dict(capacity=24), b'capacity'),
                   (dict(counts, pre_grid=(C.c_int32 * 2)(3, 6)), b'smaller than the grid'),
                   (dict(counts, pre_grid=(C.c_int32 * 2)(4, 5)), b'smaller than the grid'),
                   (dict(counts, pre_pitch=5), b'pitch'),
                   (dict(counts, pre_area=0), b'area'),
                   (dict(post_counts=8, post_grid=(C.c_int32 * 2)(4, 5), post_pitch=6,
                         post_area=4), b'smaller than the grid')):
    assert lib.sfm_flow_select(C.byref(_select(**kw))) == -1, kw
    assert word in lib.sfm_last_error(), (kw, lib.sfm_last_error())
  for kw in (dict(field=None), dict(mask=None), dict(attempts=None), dict(filled=None),
             dict(out=(C.c_void_p * 3)(8, None, 8))):
    assert lib.sfm_missing_flow_update(C.byref(_update(**kw))) == -1, kw
    assert b'NULL' in lib.sfm_last_error()
  for kw, word in ((dict(shape=(C.c_int32 * 2)(0, 6)), b'shape'),
                   (dict(field_shape=(C.c_int32 * 2)(5, 6)), b'outside the section'),
                   (dict(field_shape=(C.c_int32 * 2)(4, 7)), b'outside the section'),
                   (dict(field_shape=(C.c_int32 * 2)(0, 6)), b'outside the section')):
    assert lib.sfm_missing_flow_update(C.byref(_update(**kw))) == -1, kw
    assert word in lib.sfm_last_error(), (kw, lib.sfm_last_error())
