"""The tile renderer's entry point: ctypes structs in the header's field order and
of the C compiler's size, the call exported, the version the library reports is
the header's, bad descriptors rejected with a message."""
import ctypes as C
import os
import re
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


@pytest.mark.parametrize('cname', ['SfmRenderTile', 'SfmRenderTilesDesc'])
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


def test_struct_sizes_match_the_c_compiler(tmp_path):
  """The device reads the table as an array of SfmRenderTile: size and the offsets
  of the first and last members as a C compiler lays them out."""
  import shutil
  cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
  cmd = [cc] if cc else [_build._hipcc(), '-x', 'c']   # (the build's own compiler, as C)
  src = tmp_path / 'sizes.c'
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sofima_amd.h"\n'
                 'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(SfmRenderTile), '
                 'offsetof(SfmRenderTile, shift), offsetof(SfmRenderTile, offset), '
                 'sizeof(SfmRenderTilesDesc), offsetof(SfmRenderTilesDesc, tiles)); return 0; }\n')
  exe = tmp_path / 'sizes'
  subprocess.run(cmd + ['-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
  got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
  assert got == [C.sizeof(_abi.SfmRenderTile), _abi.SfmRenderTile.shift.offset,
                 _abi.SfmRenderTile.offset.offset, C.sizeof(_abi.SfmRenderTilesDesc),
                 _abi.SfmRenderTilesDesc.tiles.offset]


def test_entry_point_and_version(lib):
  text = _header()
  assert re.search(r'\bint sfm_render_tiles3d\s*\(', text)
  assert 'sfm_render_tiles3d' in _abi.SIGNATURES and hasattr(lib, 'sfm_render_tiles3d')
  assert lib.sfm_version() == int(re.search(r'#define SFM_ABI_VERSION (\d+)', text).group(1))


def test_bad_descriptors_are_rejected(lib):
  assert lib.sfm_render_tiles3d(None) == -1
  assert b'NULL' in lib.sfm_last_error()
  d = _abi.SfmRenderTilesDesc()          # out is NULL
  assert lib.sfm_render_tiles3d(C.byref(d)) == -1
  assert b'NULL' in lib.sfm_last_error()
  d.out = 1                              # never reached: the checks below fail first
  d.n_tiles = 1                          # ... without a table
  assert lib.sfm_render_tiles3d(C.byref(d)) == -1
  assert b'table' in lib.sfm_last_error()
  d.n_tiles = 0
  d.order = 3
  assert lib.sfm_render_tiles3d(C.byref(d)) == -1
  assert b'order' in lib.sfm_last_error()
  d.order = 1
  d.dtype, d.out_dtype = _abi.DTYPE_F32, _abi.DTYPE_U8
  assert lib.sfm_render_tiles3d(C.byref(d)) == -1
  assert b'out_dtype' in lib.sfm_last_error()
  d.dtype, d.out_dtype = _abi.DTYPE_U8, _abi.DTYPE_F32
  d.stride = (C.c_double * 3)(2.0, 2.0, 2.0)
  d.out_shape = (C.c_int32 * 3)(4, 0, 4)
  assert lib.sfm_render_tiles3d(C.byref(d)) == -1
  assert b'out_shape' in lib.sfm_last_error()
  # a data_box that leaves its tile is caught on the host copy of the table
  d.out_shape = (C.c_int32 * 3)(4, 4, 4)
  table = (_abi.SfmRenderTile * 1)()
  r = table[0]
  r.image = r.abs_map = r.weights = 1
  for name in ('tile_shape', 'map_shape', 'data_size', 'sub_size'):
    setattr(r, name, (C.c_int32 * 3)(2, 2, 2))
  r.data_start = (C.c_int32 * 3)(0, 1, 0)
  d.n_tiles, d.tiles_host, d.tiles = 1, table, 1
  assert lib.sfm_render_tiles3d(C.byref(d)) == -1
  assert b'data_box' in lib.sfm_last_error()
  r.data_start = (C.c_int32 * 3)(0, 0, 0)
  r.sub_start = (C.c_int32 * 3)(0, 0, 3)
  assert lib.sfm_render_tiles3d(C.byref(d)) == -1
  assert b'sub_box' in lib.sfm_last_error()
