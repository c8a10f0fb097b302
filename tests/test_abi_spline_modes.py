"""The entry points of the spline boundary modes: header, exports and binding agree on
the additions, nothing existing changed, bad descriptors are rejected with a message,
and with the switch SFM_SPLINE_MODES off the library still rejects the modes."""
import ctypes as C
import os
import re

import pytest

from sofima_amd import _abi, _build, _spline
from tests import spline_modes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
NEW = ('sfm_spline_prefilter_mode', 'sfm_spline_mode_pad')
ORDERS = (2, 3, 4, 5)


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _header():
  return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_entry_points_without_a_version_bump(lib):
  text = _header()
  for name in NEW:
    assert re.search(r'\bint %s\s*\(' % name, text)
    assert name in _abi.SIGNATURES and hasattr(lib, name)
  assert lib.sfm_version() == 9
  raw = open(HEADER).read()
  comment = re.search(r'#define SFM_ABI_VERSION 9\s*/\*(.*?)\*/', raw, re.S).group(1)
  assert all(name in comment for name in NEW)
  assert 'SFM_SPLINE_MODES' in raw


def test_signatures_match_the_header():
  text = _header()
  args = re.search(r'\bint sfm_spline_prefilter_mode\s*\((.*?)\)', text, re.S).group(1)
  assert [a.split()[0] for a in args.split(',')] == ['const', 'int32_t', 'int32_t', 'double']
  assert _abi.SIGNATURES['sfm_spline_prefilter_mode'] == (
      C.c_int, [C.POINTER(_abi.SfmSplinePrefilterDesc), C.c_int32, C.c_int32, C.c_double])
  args = re.search(r'\bint sfm_spline_mode_pad\s*\((.*?)\)', text, re.S).group(1)
  assert args.split()[0] == 'int32_t'
  assert _abi.SIGNATURES['sfm_spline_mode_pad'] == (C.c_int, [C.c_int32])


def test_pad_and_classes_are_the_restatement_s(lib):
  for mode, number in _abi.MODES.items():
    assert lib.sfm_spline_mode_pad(number) == (ref.PAD if mode in ref.PADDED else 0), mode
    assert (mode in _spline.MIRROR_MODES) == (ref.INIT[mode] == 'mirror' and
                                              mode not in ref.PADDED)
    assert (mode in _spline._REFLECT_MODES) == (ref.INIT[mode] == 'reflect')
  for number in (-1, 7):
    assert lib.sfm_spline_mode_pad(number) == -1
    assert b'mode' in lib.sfm_last_error()
  assert set(ref.NEW_MODES) == set(_abi.MODES) - set(_spline.MIRROR_MODES)


def test_pad_value_is_np_pad_s(lib):
  import numpy as np
  with np.errstate(all='ignore'):
    for dtype in (np.uint8, np.uint16, np.float32):
      for cval in (-3.0, 1.5, 300.0, 70000.25, 0.1):
        want = np.pad(np.zeros((1, 1), dtype), 1, mode='constant', constant_values=cval)[0, 0]
        assert _spline.pad_value(cval, dtype) == float(want), (dtype, cval)


def _desc(order=3):
  d = _abi.SfmSplinePrefilterDesc()
  d.order, d.dtype = order, _abi.DTYPE_U8
  return d


def test_bad_prefilter_mode_descriptors_are_rejected(lib):
  reflect = _abi.MODES['reflect']
  with _abi.option(_spline.MODES_OPTION, 1):
    assert lib.sfm_spline_prefilter_mode(None, reflect, 2, 0.0) == -1
    assert b'NULL' in lib.sfm_last_error()
    for mode in (-1, 7):
      assert lib.sfm_spline_prefilter_mode(_desc(), mode, 2, 0.0) == -1
      assert b'mode' in lib.sfm_last_error()
    for ndim in (1, 4):
      assert lib.sfm_spline_prefilter_mode(_desc(), reflect, ndim, 0.0) == -1
      assert b'ndim' in lib.sfm_last_error()
    for order in (0, 1, 6):
      assert lib.sfm_spline_prefilter_mode(_desc(order), reflect, 2, 0.0) == -1
      assert b'order' in lib.sfm_last_error()
    d = _desc()
    d.dtype = _abi.DTYPE_I32
    assert lib.sfm_spline_prefilter_mode(d, reflect, 2, 0.0) == -1
    assert b'dtype' in lib.sfm_last_error()
    for value in (float('nan'), float('inf')):
      assert lib.sfm_spline_prefilter_mode(_desc(), _abi.MODES['grid-constant'], 2, value) == -1
      assert b'pad value' in lib.sfm_last_error()
    for mode in _abi.MODES.values():
      assert lib.sfm_spline_prefilter_mode(_desc(), mode, 3, 0.0) == 0   # an empty table
    d = _desc()
    d.n_items = 1
    assert lib.sfm_spline_prefilter_mode(d, reflect, 2, 0.0) == -1
    assert b'NULL' in lib.sfm_last_error()
    table = (_abi.SfmSplineItem * 1)()
    d.items_host, d.items, d.coeffs = table, 1, 1
    table[0].image = 1
    # the coefficients of a padded mode are counted in the padded shape
    table[0].shape = (C.c_int32 * 3)(1, 4, 3)
    d.coeffs_len = 12
    nearest = _abi.MODES['nearest']
    assert lib.sfm_spline_prefilter_mode(d, nearest, 2, 0.0) == -1
    assert b'leaves' in lib.sfm_last_error()
    d.coeffs_len = 28 * 27 - 1
    assert lib.sfm_spline_prefilter_mode(d, nearest, 2, 0.0) == -1
    assert b'leaves' in lib.sfm_last_error()
    d.coeffs_len = 25 * 28 * 27 - 1      # ... and a 3-d item is padded on its axis of 1 too
    assert lib.sfm_spline_prefilter_mode(d, nearest, 3, 0.0) == -1
    assert b'leaves' in lib.sfm_last_error()
    # a 2-d table with a z extent
    table[0].shape = (C.c_int32 * 3)(2, 4, 3)
    d.coeffs_len = 1 << 20
    assert lib.sfm_spline_prefilter_mode(d, nearest, 2, 0.0) == -1
    assert b'shape' in lib.sfm_last_error()
    table[0].shape = (C.c_int32 * 3)(1, 0, 3)
    assert lib.sfm_spline_prefilter_mode(d, reflect, 2, 0.0) == -1
    assert b'shape' in lib.sfm_last_error()


def test_the_library_rejects_the_modes_without_the_switch(lib):
  assert _abi.get_option(_spline.MODES_OPTION) in (None, '0')
  nd = _abi.SfmNdWarpDesc()
  nd.ndim, nd.dtype = 2, _abi.DTYPE_U8
  nd.image = nd.src_map = nd.out = 1            # never reached
  rel = _abi.SfmNdWarpRelDesc()
  rel.ndim, rel.dtype, rel.has_boundary = 2, _abi.DTYPE_U8, 1
  rel.image = rel.rel_map = rel.out = 1
  aff = _abi.SfmAffineWarpDesc()
  aff.ndim, aff.dtype = 2, _abi.DTYPE_U8
  aff.shape = (C.c_int32 * 3)(1, 4, 5)
  aff.image = aff.out = 1
  for order in ORDERS:
    for mode in ref.NEW_MODES:
      number = _abi.MODES[mode]
      word = f'mode {number} at order {order}'.encode()
      nd.order = rel.order = aff.order = order
      rel.mode = aff.mode = number
      for call in (lambda: lib.sfm_ndimage_warp_mode(nd, number, 0.0),
                   lambda: lib.sfm_ndimage_warp_rel(rel), lambda: lib.sfm_affine_warp(aff),
                   lambda: lib.sfm_spline_prefilter_mode(_desc(order), number, 2, 0.0)):
        assert call() == -1
        assert word in lib.sfm_last_error() and b'SFM_SPLINE_MODES' in lib.sfm_last_error()
        with _abi.option(_spline.MODES_OPTION, 0):
          assert call() == -1
          assert word in lib.sfm_last_error()
      with pytest.raises(NotImplementedError, match=f'{mode}.*{order}'):
        _spline.check_mode(mode, order, 'f')
    # with the switch the mode check passes and the next one fails
    with _abi.option(_spline.MODES_OPTION, 1):
      assert lib.sfm_ndimage_warp_mode(nd, _abi.MODES['nearest'], 0.0) == -1
      assert b'shape' in lib.sfm_last_error()
      _spline.check_mode('nearest', order, 'f')
  # the three modes of the default prefilter pass through the new entry point
  for mode in _spline.MIRROR_MODES:
    assert lib.sfm_spline_prefilter_mode(_desc(), _abi.MODES[mode], 2, 0.0) == 0
    _spline.check_mode(mode, 3, 'f')
  for mode in ref.NEW_MODES:
    _spline.check_mode(mode, 1, 'f')             # orders 0 and 1 take every mode
