"""The reference-position entry points: ctypes structs in the header's field
order, the two calls exported, NULL arguments rejected."""
import ctypes as C
import os
import re

import pytest

from sofima_amd import _abi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
ENTRY_POINTS = ('sfm_prev_state', 'sfm_mask_irregular_f64')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize('cname', ['SfmPrevFlow', 'SfmPrevStateDesc'])
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


def test_struct_sizes_and_limits():
  consts = dict(re.findall(r'#define (SFM_PREV_MAX_\w+) (\d+)', _header()))
  assert int(consts['SFM_PREV_MAX_FLOWS']) == _abi.PREV_MAX_FLOWS == 8
  assert int(consts['SFM_PREV_MAX_REFS']) == _abi.PREV_MAX_REFS == 16
  # int32 x 2, pointer, int64 x 2, int32[16], pointer[16]: no padding on LP64
  assert C.sizeof(_abi.SfmPrevFlow) == 8 + 8 + 16 + 64 + 128
  assert C.sizeof(_abi.SfmPrevStateDesc) == 24 + 8 * C.sizeof(_abi.SfmPrevFlow) + 8
  assert _abi.SfmPrevStateDesc.flows.offset == 24


def test_entry_points_and_version(lib):
  text = _header()
  for name in ENTRY_POINTS:
    assert re.search(r'\bint %s\s*\(' % name, text), name
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1))


def test_null_and_malformed_descriptors_are_rejected(lib):
  """Argument checks run on the host, before anything is launched."""
  assert lib.sfm_prev_state(None, None) == -1
  assert b'NULL' in lib.sfm_last_error()
  d = _abi.SfmPrevStateDesc()
  assert lib.sfm_prev_state(C.byref(d), None) == -1
  assert b'NULL' in lib.sfm_last_error()
  assert lib.sfm_mask_irregular_f64(None, None, None, None) == -1
  assert b'NULL' in lib.sfm_last_error()
  m = _abi.SfmMaskIrregularDesc()
  assert lib.sfm_mask_irregular_f64(C.byref(m), 8, 8, None) == -1    # no counter
  assert b'NULL' in lib.sfm_last_error()

  def desc(**kw):
    d = _abi.SfmPrevStateDesc()
    d.shape = (C.c_int32 * 2)(4, 4)
    d.n_flows = 1
    d.stride = (C.c_float * 2)(40, 40)
    fl = d.flows[0]
    fl.channels, fl.n_refs, fl.flow = 2, 1, 8           # never dereferenced on the host
    fl.flow_channel_stride = fl.mesh_channel_stride = 16
    fl.mesh[0] = 8
    for k, v in kw.items():
      obj, _, field = k.rpartition('__')
      setattr(d.flows[0] if obj == 'flow' else d, field, v)
    return d

  for kw, word in ((dict(n_flows=0), b'flows'), (dict(n_flows=9), b'flows'),
                   (dict(shape=(C.c_int32 * 2)(0, 4)), b'shape'),
                   (dict(stride=(C.c_float * 2)(0, 40)), b'stride'),
                   (dict(flow__channels=4), b'channels'),
                   (dict(flow__n_refs=2), b'reference'),
                   (dict(flow__channels=3, flow__n_refs=17), b'reference'),
                   (dict(flow__channels=3), b'offset 0'),        # delta_z[0] == 0
                   (dict(flow__flow=None), b'NULL flow'),
                   (dict(flow__flow_channel_stride=15), b'overlapping'),
                   (dict(flow__mesh_channel_stride=15), b'overlapping'),
                   (dict(flow__mesh=(C.c_void_p * 16)()), b'NULL reference')):
    assert lib.sfm_prev_state(C.byref(desc(**kw)), 8) == -1, kw
    assert word in lib.sfm_last_error(), (kw, lib.sfm_last_error())
