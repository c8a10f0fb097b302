"""The entry points of the spline orders: ctypes structs in the header's field order
and of the C compiler's size, the calls exported, bad descriptors rejected with a
message; the entry points of orders 0 and 1 still reject the higher orders."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from sofima_amd import _abi, _build, _spline
from tests import ndwarp_spline_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


@pytest.mark.parametrize('cname', ['SfmSplineItem', 'SfmSplinePrefilterDesc'])
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
  """The device reads the table as an array of SfmSplineItem."""
  cc = next((c for c in ('cc', 'gcc', 'clang') if shutil.which(c)), None)
  cmd = [cc] if cc else [_build._hipcc(), '-x', 'c']
  src = tmp_path / 'sizes.c'
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sofima_amd.h"\n'
                 'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(SfmSplineItem), '
                 'offsetof(SfmSplineItem, coeff_offset), offsetof(SfmSplineItem, shape), '
                 'offsetof(SfmSplineItem, zn), sizeof(SfmSplinePrefilterDesc), '
                 'offsetof(SfmSplinePrefilterDesc, coeffs_len)); return 0; }\n')
  exe = tmp_path / 'sizes'
  subprocess.run(cmd + ['-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
  got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                        check=True).stdout.split()]
  assert got == [C.sizeof(_abi.SfmSplineItem), _abi.SfmSplineItem.coeff_offset.offset,
                 _abi.SfmSplineItem.shape.offset, _abi.SfmSplineItem.zn.offset,
                 C.sizeof(_abi.SfmSplinePrefilterDesc),
                 _abi.SfmSplinePrefilterDesc.coeffs_len.offset]


def test_entry_points_without_a_version_bump(lib):
  text = _header()
  for name in ('sfm_spline_prefilter', 'sfm_ndimage_warp_spline', 'sfm_render_tiles3d_spline'):
    assert re.search(r'\bint %s\s*\(' % name, text)
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == 9


def test_poles_are_the_restatement_s(lib):
  assert _spline._POLES == ref.POLES and _spline.ORDERS == tuple(ref.POLES)


def test_bad_prefilter_descriptors_are_rejected(lib):
  assert lib.sfm_spline_prefilter(None) == -1
  assert b'NULL' in lib.sfm_last_error()
  d = _abi.SfmSplinePrefilterDesc()
  for order in (0, 1, 6):
    d.order = order
    assert lib.sfm_spline_prefilter(C.byref(d)) == -1
    assert b'order' in lib.sfm_last_error()
  d.order = 3
  d.dtype = _abi.DTYPE_I32
  assert lib.sfm_spline_prefilter(C.byref(d)) == -1
  assert b'dtype' in lib.sfm_last_error()
  d.dtype = _abi.DTYPE_U8
  assert lib.sfm_spline_prefilter(C.byref(d)) == 0        # an empty table is no work
  d.n_items = 1
  assert lib.sfm_spline_prefilter(C.byref(d)) == -1
  assert b'NULL' in lib.sfm_last_error()
  table = (_abi.SfmSplineItem * 1)()
  d.items_host, d.items, d.coeffs, d.coeffs_len = table, 1, 1, 23
  assert lib.sfm_spline_prefilter(C.byref(d)) == -1
  assert b'NULL image' in lib.sfm_last_error()
  table[0].image = 1
  table[0].shape = (C.c_int32 * 3)(2, 0, 3)
  assert lib.sfm_spline_prefilter(C.byref(d)) == -1
  assert b'shape' in lib.sfm_last_error()
  # an item that leaves the coefficient buffer is caught on the host copy of the table
  table[0].shape = (C.c_int32 * 3)(2, 4, 3)
  assert lib.sfm_spline_prefilter(C.byref(d)) == -1
  assert b'leaves' in lib.sfm_last_error()
  d.coeffs_len = 24
  table[0].coeff_offset = 1
  assert lib.sfm_spline_prefilter(C.byref(d)) == -1
  assert b'leaves' in lib.sfm_last_error()
  table[0].coeff_offset = -1
  assert lib.sfm_spline_prefilter(C.byref(d)) == -1
  assert b'leaves' in lib.sfm_last_error()


def test_orders_belong_to_their_entry_points(lib):
  nd = _abi.SfmNdWarpDesc()
  nd.ndim = 2
  nd.image = nd.src_map = nd.out = 1       # never reached: the order check fails first
  for order, call in ((3, lib.sfm_ndimage_warp), (1, lib.sfm_ndimage_warp_spline),
                      (6, lib.sfm_ndimage_warp_spline)):
    nd.order = order
    assert call(C.byref(nd)) == -1
    assert b'order' in lib.sfm_last_error()
  assert lib.sfm_ndimage_warp_spline(None) == -1
  rd = _abi.SfmRenderTilesDesc()
  rd.out = 1
  for order in (0, 1, 6):
    rd.order = order
    assert lib.sfm_render_tiles3d_spline(C.byref(rd), None) == -1
    assert b'order' in lib.sfm_last_error()
  assert lib.sfm_render_tiles3d_spline(None, None) == -1
  # a table without coefficients
  rd.order = 3
  table = (_abi.SfmRenderTile * 1)()
  rd.n_tiles, rd.tiles_host, rd.tiles = 1, table, 1
  assert lib.sfm_render_tiles3d_spline(C.byref(rd), None) == -1
  assert b'coefficients' in lib.sfm_last_error()


def test_orders_above_1_are_opt_in(lib):
  """_spline.check_order: orders 0 and 1 always, 2 to 5 with SFM_SPLINE_ORDERS=1 only."""
  assert _abi.get_option(_spline.OPTION) in (None, '0')
  for order in (0, 1):
    _spline.check_order(order, 'f')
  for order in _spline.ORDERS:
    with pytest.raises(NotImplementedError, match=_spline.OPTION):
      _spline.check_order(order, 'f')
    with _abi.option(_spline.OPTION, 1):
      _spline.check_order(order, 'f')
      with _abi.option(_spline.OPTION, 0):
        with pytest.raises(NotImplementedError, match=_spline.OPTION):
          _spline.check_order(order, 'f')
  with _abi.option(_spline.OPTION, 1):
    for order in (6, -1, 1.5):
      with pytest.raises(NotImplementedError, match='0 to 5'):
        _spline.check_order(order, 'f')
