"""Spline orders 2 to 5 under SciPy's remaining boundary modes on the device (-m gpu):
'nearest', 'reflect' (and its synonym 'grid-mirror'), 'grid-constant' and 'grid-wrap'.

  * the coefficients of `_spline.prefilter(mode=)` against scipy.ndimage.spline_filter,
    for the padded modes of the image padded by 12 samples as SciPy pads it;
  * `warp.ndimage_warp`, `warp.affine_transform` and the two functions of
    `decorators_warp` against SciPy itself.
Integer images compare with array_equal, float images by their bits.  Both switches
(SFM_SPLINE_ORDERS, SFM_SPLINE_MODES) are on in every test but the one of the default.
"""
import functools
import types

import numpy as np
import pytest
import scipy.ndimage
import torch
from scipy import ndimage

from sofima_amd import _abi, _dev, _spline, decorators_warp, map_utils, warp
from tests import ndwarp_modes_ref as ref
from tests import ndwarp_rel_ref as rel_ref
from tests import spline_modes_ref as modes
from tests.test_gpu_ndwarp_spline import assert_same

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.float32)
ORDERS = (2, 3, 4, 5)
MODES = modes.NEW_MODES
CVAL = 7.25
_ABI_DTYPE = {np.dtype(np.uint8): _abi.DTYPE_U8, np.dtype(np.uint16): _abi.DTYPE_U16,
              np.dtype(np.float32): _abi.DTYPE_F32}


@pytest.fixture(autouse=True)
def switches(request):
  with _abi.option(_spline.OPTION, 1):
    if request.node.name == 'test_the_modes_are_opt_in':
      yield
      return
    with _abi.option(_spline.MODES_OPTION, 1):
      yield


def sampler(mode, cval):
  return functools.partial(scipy.ndimage.map_coordinates, mode=mode, cval=cval)


def resident(a, dev):
  a = np.ascontiguousarray(a)
  if a.dtype == np.uint16:
    return torch.from_numpy(a.view(np.int16)).to(dev)
  return torch.from_numpy(a).to(dev)


def scipy_coeffs(img, order, mode, cval):
  with np.errstate(all='ignore'):
    return ndimage.spline_filter(modes.pad(img, mode, cval), order, output=np.float64, mode=mode)


def device_coeffs(img, order, mode, cval, dev):
  """The prefilter alone: the float64 coefficients of a whole 2-D / 3-D array."""
  shape = (1,) * (3 - img.ndim) + img.shape
  t = resident(img, dev)
  ws, off = _spline.prefilter([(t.data_ptr(), shape, (shape[1] * shape[2], shape[2], 1))],
                              _ABI_DTYPE[img.dtype], order, dev, mode, img.ndim,
                              _spline.pad_value(cval, img.dtype))
  pad = 2 * modes.PAD if mode in modes.PADDED else 0
  cshape = tuple(s + pad for s in img.shape)
  assert off == [0] and ws.dtype == torch.float64 and ws.numel() == max(int(np.prod(cshape)), 1)
  return ws.cpu().numpy().reshape(cshape)


# (5,7), (3,4,6), (1,5,2): a length-1 axis of a 3-D array is padded and filtered;
# (1,1,9): the unpadded modes skip both length-1 axes; (2,70): the x pass crosses two
# 32-column chunks, three when padded; (70,9): two workgroups of the row kernel; (2,2):
# the shortest line
COEFF_SHAPES = ((5, 7), (3, 4, 6), (1, 5, 2), (1, 1, 9), (2, 70), (70, 9), (2, 2))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('order', ORDERS)
def test_coefficients(gpu, order, mode):
  rng = np.random.default_rng(10 * order + MODES.index(mode))
  for shape in COEFF_SHAPES:
    for dtype in DTYPES:
      img = ref.image(rng, shape, dtype)
      assert_same(device_coeffs(img, order, mode, CVAL, gpu), scipy_coeffs(img, order, mode, CVAL),
                  (shape, np.dtype(dtype).name))


@pytest.mark.parametrize('mode', ['nearest', 'reflect', 'grid-constant', 'grid-wrap'])
def test_item_table_with_a_strided_region(gpu, mode):
  """Two regions of different shape in one table, one of them every second column of a
  box inside a larger array: each is filtered where it lies."""
  rng = np.random.default_rng(5)
  for order in (3, 4):
    for dtype in DTYPES:
      whole = ref.image(rng, (3, 4, 6), dtype)
      big = ref.image(rng, (4, 9, 20), dtype)
      region = big[1:3, 2:7, 3:17:2]
      assert region.shape == (2, 5, 7)
      whole_t, big_t = resident(whole, gpu), resident(big, gpu)
      item = big.dtype.itemsize
      table = [(whole_t.data_ptr(), whole.shape, (24, 6, 1)),
               (big_t.data_ptr() + item * (1 * 180 + 2 * 20 + 3), region.shape, (180, 20, 2))]
      ws, off = _spline.prefilter(table, _ABI_DTYPE[np.dtype(dtype)], order, gpu, mode, 3,
                                  _spline.pad_value(CVAL, dtype))
      pad = 2 * modes.PAD if mode in modes.PADDED else 0
      shapes = [tuple(s + pad for s in a.shape) for a in (whole, region)]
      assert off == [0, int(np.prod(shapes[0]))]
      got = ws.cpu().numpy()
      for a, o, s in zip((whole, region), off, shapes):
        assert_same(got[o:o + int(np.prod(s))].reshape(s), scipy_coeffs(a, order, mode, CVAL),
                    (order, np.dtype(dtype).name, s))


# -- ndimage_warp ------------------------------------------------------------------------
def device_at(img, cmap, out_shape, order, **kw):
  dim = img.ndim
  zero = np.zeros(dim, np.int64)
  size = np.array(out_shape[::-1], np.int64)
  b = types.SimpleNamespace(start=zero, size=size)
  return warp.ndimage_warp(img, cmap, (1,) * dim, tuple(size), (0,) * dim, order=order,
                           image_box=types.SimpleNamespace(start=zero, size=zero),
                           map_box=b, out_box=b, **kw)


def warp_at(img, coords, order, mode, cval):
  """(device, SciPy twice, SciPy twice under the default mode) at `coords` [ndim, n]."""
  cmap, out_shape = ref.stride1_map(coords)
  got = device_at(img, cmap, out_shape, order, map_coordinates=sampler(mode, cval))
  stride = (1,) * img.ndim
  want = ref.ndimage_warp_scipy(img, cmap, stride, order, mode, cval, out_shape)
  default = ref.ndimage_warp_scipy(img, cmap, stride, order, 'constant', 0.0, out_shape)
  return got, want, default


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', MODES)
def test_ndimage_warp_against_scipy(gpu, mode, order):
  rng = np.random.default_rng(2000 + 10 * MODES.index(mode) + order)
  for k, shape in enumerate(ref.SHAPES_2D + ref.SHAPES_3D):
    img = ref.image(rng, shape, DTYPES[(k + order) % 3])
    coords = ref.mode_coords(rng, shape)
    got, want, default = warp_at(img, coords, order, mode, CVAL)
    assert_same(got, want, shape)
    assert np.mean(want != default) > 0.2, shape


@pytest.mark.parametrize('mode', ['nearest', 'grid-wrap'])
def test_resident_image_and_relative_float32_map(gpu, mode):
  rng = np.random.default_rng(21)
  for shape, nodes, stride in (((12, 15), (5, 7), (3.0, 2.5)), ((5, 9, 11), (4, 6, 5), (2.0, 2.0, 3.5))):
    for dtype in DTYPES:
      img = ref.image(rng, shape, dtype)
      cmap = rng.uniform(-20.0, 20.0, (len(shape),) + nodes).astype(np.float32)
      got = warp.ndimage_warp(resident(img, gpu).view(torch.uint16) if dtype == np.uint16 else
                              resident(img, gpu), torch.from_numpy(cmap).to(gpu), stride,
                              shape[::-1], (0,) * len(shape), order=3, device_output=True,
                              map_coordinates=sampler(mode, CVAL))
      assert isinstance(got, _dev.DeviceArray) and got.dtype == np.dtype(dtype)
      want = rel_ref.warp_scipy(img, cmap, stride, 3, mode, CVAL)
      assert_same(np.asarray(got), want, (shape, np.dtype(dtype).name))
      default = rel_ref.warp_scipy(img, cmap, stride, 3)
      assert np.mean(want != default) > 0.2


@pytest.mark.parametrize('mode,cval', [('nearest', 0.0), ('reflect', 0.0), ('grid-constant', CVAL),
                                        ('grid-wrap', 0.0)])
def test_map_smaller_than_the_output(gpu, mode, cval):
  rng = np.random.default_rng(7)
  for shape, nodes, stride in (((12, 15), (3, 4), (3.0, 2.5)), ((5, 9, 11), (2, 3, 3), (2.0, 2.0, 3.5))):
    for dtype in DTYPES:
      img = ref.image(rng, shape, dtype)
      cmap = rng.uniform(-1.5, 1.5, (len(shape),) + nodes)
      got = warp.ndimage_warp(img, cmap, stride, shape[::-1], (0,) * len(shape), order=3,
                              map_coordinates=sampler(mode, cval))
      want = ref.ndimage_warp_scipy(img, cmap, stride, 3, mode, cval)
      assert_same(got, want, (shape, np.dtype(dtype).name))
      default = ref.ndimage_warp_scipy(img, cmap, stride, 3, 'constant', 0.0)
      assert np.mean(want != default) > 0.2


def test_nan_and_huge_coordinates_give_cval(gpu):
  rng = np.random.default_rng(9)
  bad = np.array([np.nan, 2.0**31, -2.0**31, 1e300, -1e300, np.inf, -np.inf, 2.0**40 + 0.5])
  for shape in ((5, 7), (3, 4, 6)):
    dim = len(shape)
    n = bad.size * dim
    coords = np.stack([rng.uniform(0, s - 1, 100 + n) for s in shape])
    for d in range(dim):
      coords[d, 100 + d * bad.size:100 + (d + 1) * bad.size] = bad
    cmap, out_shape = ref.stride1_map(coords)
    for dtype in DTYPES:
      img = ref.image(rng, shape, dtype)
      for mode in MODES:
        got = device_at(img, cmap, out_shape, 3,
                        map_coordinates=sampler(mode, 200.7)).ravel()[100:100 + n]
        assert_same(got, ref.convert(np.full(n, 200.7), dtype), (shape, mode))


@pytest.mark.parametrize('cval', [-3, 1.5, 300])
def test_grid_constant_pads_with_cval_in_the_image_s_type(gpu, cval):
  """np.pad stores cval in the uint8 image (-3 -> 253, 300 -> 44), the taps beyond the
  padded array read cval itself, and a sample goes through the conversion."""
  rng = np.random.default_rng(11)
  img = ref.image(rng, (5, 7), np.uint8)
  coords = ref.mode_coords(rng, (5, 7))
  for order in (2, 3):
    got, want, default = warp_at(img, coords, order, 'grid-constant', cval)
    assert_same(got, want, (cval, order))
    assert np.mean(want != default) > 0.2


# -- affine_transform ----------------------------------------------------------------------
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('mode', MODES)
def test_affine_transform_against_scipy(gpu, mode, order):
  rng = np.random.default_rng(3000 + 10 * MODES.index(mode) + order)
  for k, shape in enumerate(ref.SHAPES_2D + ref.SHAPES_3D):
    img = ref.image(rng, shape, DTYPES[(k + order) % 3])
    for name, m, off in ref.matrices(rng, len(shape))[2:6]:
      want = ndimage.affine_transform(img, m, off, order=order, mode=mode, cval=CVAL)
      got = warp.affine_transform(img, m, off, order=order, mode=mode, cval=CVAL)
      assert_same(got, want, (shape, name))
      if name == 'mostly_outside' and min(shape) >= 3:
        default = ndimage.affine_transform(img, m, off, order=order)
        assert np.mean(want != default) > 0.2, (shape, name)


# -- decorators_warp -----------------------------------------------------------------------
def test_warp_coord_map(gpu):
  rng = np.random.default_rng(41)
  img = ref.image(rng, (11, 9, 5), np.uint8)                    # xyz
  cmap = rng.uniform(-6.0, 6.0, (3, 3, 5, 6)).astype(np.float32)
  stride = (2.0, 2.0, 2.0)
  got = decorators_warp.warp_coord_map(img, cmap, mode='nearest', cval=CVAL, stride=stride,
                                       overlap=(0, 0, 0), order=3)
  want = rel_ref.warp_scipy(img.T, cmap, stride, 3, 'nearest', CVAL).T
  assert_same(got, want)
  assert np.mean(want != rel_ref.warp_scipy(img.T, cmap, stride, 3).T) > 0.2


def test_warp_affine(gpu):
  rng = np.random.default_rng(42)
  img = ref.image(rng, (11, 9, 5), np.float32)                  # xyz
  a = 0.4
  matrix = np.array([[np.cos(a), -np.sin(a), 0.0, 3.0], [np.sin(a), np.cos(a), 0.02, -2.0],
                     [0.0, 0.05, 1.0, 0.5]])
  got = decorators_warp.warp_affine(img, matrix, order=3, implementation='sofima',
                                    map_coordinates=sampler('reflect', 0.0))
  box = types.SimpleNamespace(start=np.zeros(3, np.int64), size=np.array(img.shape, np.int64))
  homogeneous = np.eye(4)
  homogeneous[:3] = matrix
  cmap = np.asarray(map_utils.make_affine_map(np.linalg.inv(homogeneous)[:3, :], box, [1, 1, 1]))
  want = rel_ref.warp_scipy(img.T, cmap, (1, 1, 1), 3, 'reflect', 0.0).T
  assert_same(got, want)
  assert np.mean(want != rel_ref.warp_scipy(img.T, cmap, (1, 1, 1), 3).T) > 0.2


# -- the default ---------------------------------------------------------------------------
def test_the_modes_are_opt_in(gpu):
  """SFM_SPLINE_MODES unset, the order switch on: every mode name raises, in Python and
  from the library."""
  assert _abi.get_option(_spline.MODES_OPTION) in (None, '0')
  img = np.zeros((8, 9), np.uint8)
  cmap = np.zeros((2, 2, 2), np.float32)
  lib = _abi.load()
  for order in ORDERS:
    for mode in MODES:
      with pytest.raises(NotImplementedError, match=f'{mode}.*{order}'):
        warp.ndimage_warp(img, cmap, (8, 8), (8, 8), (0, 0), order=order,
                          map_coordinates=sampler(mode, 0.0))
      with pytest.raises(NotImplementedError, match=f'{mode}.*{order}'):
        warp.affine_transform(img, np.eye(2), order=order, mode=mode)
      with pytest.raises(NotImplementedError, match=_spline.MODES_OPTION):
        warp.affine_transform(img, np.eye(2), order=order, mode=mode)
      d = _abi.SfmNdWarpDesc()
      d.ndim, d.order = 2, order
      d.image = d.src_map = d.out = 1      # never reached
      assert lib.sfm_ndimage_warp_mode(d, _abi.MODES[mode], 0.0) == -1
      assert f'mode {_abi.MODES[mode]} at order {order}'.encode() in lib.sfm_last_error()
      p = _abi.SfmSplinePrefilterDesc()
      p.order = order
      assert lib.sfm_spline_prefilter_mode(p, _abi.MODES[mode], 2, 0.0) == -1
      assert f'mode {_abi.MODES[mode]} at order {order}'.encode() in lib.sfm_last_error()
