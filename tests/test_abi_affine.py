"""The entry points of the boundary modes and of the fused affine warp: the ctypes struct
in the header's field order and of the C compiler's size, the calls exported without a
version bump, the mode numbers of header, library and binding, and bad descriptors
rejected with a message."""
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
  body = re.search(r'typedef struct SfmAffineWarpDesc \{(.*?)\} SfmAffineWarpDesc;', _header(),
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if not decl:
      continue
    for part in decl.split(','):
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$',
                             part.strip()).group(1))
  assert names == [f[0] for f in _abi.SfmAffineWarpDesc._fields_]


def test_struct_size_matches_the_c_compiler(tmp_path):
  cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
  cmd = [cc] if cc else [_build._hipcc(), '-x', 'c']
  fields = ('mode', 'shape', 'matrix', 'offset', 'cval', 'image', 'out', 'stream')
  src = tmp_path / 'sizes.c'
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sofima_amd.h"\n'
                 'int main(void) { printf("%zu", sizeof(SfmAffineWarpDesc));\n' +
                 ''.join(f'printf(" %zu", offsetof(SfmAffineWarpDesc, {f}));\n' for f in fields) +
                 'return 0; }\n')
  exe = tmp_path / 'sizes'
  subprocess.run(cmd + ['-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
  got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
  assert got == [C.sizeof(_abi.SfmAffineWarpDesc)] + [
      getattr(_abi.SfmAffineWarpDesc, f).offset for f in fields]


def test_entry_points_without_a_version_bump(lib):
  text = _header()
  for name in ('sfm_ndimage_warp_mode', 'sfm_affine_warp'):
    assert re.search(r'\bint %s\s*\(' % name, text)
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == 9
  comment = re.search(r'#define SFM_ABI_VERSION 9\s*/\*(.*?)\*/', open(HEADER).read(), re.S).group(1)
  assert 'sfm_ndimage_warp_mode' in comment and 'sfm_affine_warp' in comment


def test_mode_numbers_agree():
  text = _header()
  for name, value in _abi.MODES.items():
    macro = 'SFM_MODE_' + ('REFLECT' if name == 'grid-mirror' else name.upper().replace('-', '_'))
    assert int(re.search(r'#define %s (\d+)' % macro, text).group(1)) == value
  assert sorted(set(_abi.MODES.values())) == list(range(7))


def _affine_desc():
  d = _abi.SfmAffineWarpDesc()
  d.ndim, d.dtype, d.order, d.mode = 2, _abi.DTYPE_U8, 1, _abi.MODES['constant']
  d.shape = (C.c_int32 * 3)(1, 4, 5)
  d.image = d.out = 1         # never reached: every check below fails first
  return d


def test_bad_affine_descriptors_are_rejected(lib):
  assert lib.sfm_affine_warp(None) == -1
  assert b'NULL' in lib.sfm_last_error()
  d = _affine_desc()
  d.image = None
  assert lib.sfm_affine_warp(C.byref(d)) == -1
  assert b'NULL' in lib.sfm_last_error()
  for field, value, word in (('ndim', 1, b'ndim'), ('ndim', 4, b'ndim'), ('order', 6, b'order'),
                             ('order', -1, b'order'), ('mode', 7, b'mode'), ('mode', -1, b'mode'),
                             ('dtype', _abi.DTYPE_I32, b'dtype'), ('cval', float('nan'), b'cval'),
                             ('cval', float('inf'), b'cval')):
    d = _affine_desc()
    setattr(d, field, value)
    assert lib.sfm_affine_warp(C.byref(d)) == -1, field
    assert word in lib.sfm_last_error(), (field, lib.sfm_last_error())
  d = _affine_desc()
  d.shape = (C.c_int32 * 3)(1, 0, 5)
  assert lib.sfm_affine_warp(C.byref(d)) == -1
  assert b'shape' in lib.sfm_last_error()
  d.shape = (C.c_int32 * 3)(2, 4, 5)        # a 2-d array with a z extent
  assert lib.sfm_affine_warp(C.byref(d)) == -1
  assert b'shape' in lib.sfm_last_error()
  # orders 2 .. 5 take constant, mirror and wrap alone
  for order in (2, 3, 4, 5):
    for mode in ('grid-constant', 'nearest', 'reflect', 'grid-wrap'):
      d = _affine_desc()
      d.order, d.mode = order, _abi.MODES[mode]
      assert lib.sfm_affine_warp(C.byref(d)) == -1
      assert b'mode' in lib.sfm_last_error()


def test_bad_mode_descriptors_are_rejected(lib):
  assert lib.sfm_ndimage_warp_mode(None, 0, 0.0) == -1
  assert b'NULL' in lib.sfm_last_error()
  d = _abi.SfmNdWarpDesc()
  d.ndim, d.dtype, d.order = 2, _abi.DTYPE_U8, 1
  d.image = d.src_map = d.out = 1            # never reached
  for mode in (-1, 7):
    assert lib.sfm_ndimage_warp_mode(C.byref(d), mode, 0.0) == -1
    assert b'mode' in lib.sfm_last_error()
  assert lib.sfm_ndimage_warp_mode(C.byref(d), 0, float('nan')) == -1
  assert b'cval' in lib.sfm_last_error()
  for order in (-1, 6):
    d.order = order
    assert lib.sfm_ndimage_warp_mode(C.byref(d), 0, 0.0) == -1
    assert b'order' in lib.sfm_last_error()
  d.order = 3
  assert lib.sfm_ndimage_warp_mode(C.byref(d), _abi.MODES['nearest'], 0.0) == -1
  assert b'mode' in lib.sfm_last_error()
  # consistent so far, inconsistent shapes: the checks of sfm_ndimage_warp apply
  d.order = 1
  assert lib.sfm_ndimage_warp_mode(C.byref(d), _abi.MODES['mirror'], 0.0) == -1
  assert b'shape' in lib.sfm_last_error()
  d.src_map = None
  assert lib.sfm_ndimage_warp_mode(C.byref(d), _abi.MODES['mirror'], 0.0) == -1
  assert b'NULL' in lib.sfm_last_error()
