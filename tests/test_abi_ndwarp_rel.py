"""The entry point that reads a relative coordinate map, `sfm_ndimage_warp_rel`: the
ctypes struct in the header's field order and of the C compiler's size and offsets, the
call declared, bound and exported without a version bump, and NULL or invalid
descriptors rejected with a message before anything is launched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from sofima_amd import _abi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_struct_layout_matches_header():
  body = re.search(r'typedef struct SfmNdWarpRelDesc \{(.*?)\} SfmNdWarpRelDesc;', _header(),
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    for part in decl.split(','):
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$',
                             part.strip()).group(1))
  assert names == [f[0] for f in _abi.SfmNdWarpRelDesc._fields_]


def test_struct_size_matches_the_c_compiler(tmp_path):
  cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
  cmd = [cc] if cc else [_build._hipcc(), '-x', 'c']
  fields = [f[0] for f in _abi.SfmNdWarpRelDesc._fields_]
  src = tmp_path / 'sizes.c'
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sofima_amd.h"\n'
                 'int main(void) { printf("%zu", sizeof(SfmNdWarpRelDesc));\n' +
                 ''.join(f'printf(" %zu", offsetof(SfmNdWarpRelDesc, {f}));\n' for f in fields) +
                 'return 0; }\n')
  exe = tmp_path / 'sizes'
  subprocess.run(cmd + ['-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
  got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
  assert got == [C.sizeof(_abi.SfmNdWarpRelDesc)] + [
      getattr(_abi.SfmNdWarpRelDesc, f).offset for f in fields]


def test_entry_point_without_a_version_bump(lib):
  text = _header()
  assert re.search(r'\bint sfm_ndimage_warp_rel\s*\(\s*const SfmNdWarpRelDesc\s*\*', text)
  assert 'sfm_ndimage_warp_rel' in _abi.SIGNATURES and hasattr(lib, 'sfm_ndimage_warp_rel')
  assert lib.sfm_version() == 9
  comment = re.search(r'#define SFM_ABI_VERSION 9\s*/\*(.*?)\*/', open(HEADER).read(), re.S).group(1)
  for name in ('sfm_ndimage_warp_rel', 'sfm_ndimage_warp_mode', 'sfm_affine_warp',
               'sfm_ndimage_warp_spline', 'sfm_warp_points'):
    assert name in comment
  # the absolute-map descriptor and its calls are what they were
  assert [f[0] for f in _abi.SfmNdWarpDesc._fields_] == [
      'ndim', 'dtype', 'order', 'image_shape', 'map_shape', 'out_shape', 'stride', 'offset',
      'image', 'src_map', 'out', 'stream']
  assert C.sizeof(_abi.SfmNdWarpDesc) == 128


def _desc(dim=2):
  """Consistent but for the pointers, which are never reached: every check below
  fails first."""
  d = _abi.SfmNdWarpRelDesc()
  d.ndim, d.dtype, d.order = dim, _abi.DTYPE_U8, 1
  shape = (1, 4, 5) if dim == 2 else (3, 4, 5)
  d.image_shape = d.map_shape = d.out_shape = (C.c_int32 * 3)(*shape)
  d.stride = (C.c_double * 3)(1.0, 2.0, 2.5)
  d.scale = (C.c_double * 3)(1.0, 1.0, 1.0)
  d.image = d.rel_map = d.out = 1
  return d


def test_null_arguments_are_rejected(lib):
  assert lib.sfm_ndimage_warp_rel(None) == -1
  assert b'NULL' in lib.sfm_last_error()
  for field in ('image', 'rel_map', 'out'):
    for f64 in (0, 1):
      d = _desc()
      d.map_f64 = f64
      setattr(d, field, None)
      assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1, field
      assert b'NULL' in lib.sfm_last_error(), field


def test_bad_descriptors_are_rejected(lib):
  for field, value, word in (('ndim', 1, b'ndim'), ('ndim', 4, b'ndim'), ('order', 6, b'order'),
                             ('order', -1, b'order'), ('dtype', _abi.DTYPE_I32, b'dtype')):
    d = _desc()
    setattr(d, field, value)
    assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1, field
    assert word in lib.sfm_last_error(), (field, lib.sfm_last_error())
  for field in ('image_shape', 'map_shape', 'out_shape'):
    d = _desc()
    setattr(d, field, (C.c_int32 * 3)(1, 0, 5))
    assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1
    assert b'shape' in lib.sfm_last_error()
    d = _desc()
    setattr(d, field, (C.c_int32 * 3)(2, 4, 5))      # a 2-d array with a z extent
    assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1
    assert b'shape' in lib.sfm_last_error()
  for dim, axis in ((2, 1), (2, 2), (3, 0)):
    d = _desc(dim)
    d.stride[axis] = 0.0
    assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1
    assert b'stride' in lib.sfm_last_error()


def test_bad_boundaries_are_rejected(lib):
  for mode in (-1, 7):
    d = _desc()
    d.has_boundary, d.mode = 1, mode
    assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1
    assert b'mode' in lib.sfm_last_error()
  for cval in (float('nan'), float('inf')):
    d = _desc()
    d.has_boundary, d.cval = 1, cval
    assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1
    assert b'cval' in lib.sfm_last_error()
  # orders 2 .. 5 take constant, mirror and wrap alone
  for order in (2, 3, 4, 5):
    for mode in ('grid-constant', 'nearest', 'reflect', 'grid-wrap'):
      d = _desc()
      d.order, d.has_boundary, d.mode = order, 1, _abi.MODES[mode]
      assert lib.sfm_ndimage_warp_rel(C.byref(d)) == -1
      assert b'mode' in lib.sfm_last_error()
