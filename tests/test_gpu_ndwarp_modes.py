"""SciPy's boundary modes and fill value in `warp.ndimage_warp` on the device (-m gpu):
`map_coordinates=functools.partial(scipy.ndimage.map_coordinates, mode=, cval=)`.

The reference hands that callable to both steps (warp.py:308-314), so the reference
result is SciPy's map_coordinates twice with the same mode and cval
(`ndwarp_modes_ref.ndimage_warp_scipy`).  The coordinates of every case are those
of tests/test_ndwarp_modes_ref.py: a stride-1 float64 map as large as the output
holds them as node values (`stride1_map`), which the order-1 step hands on.  Integer
images compare with array_equal, float32 images by their bits.  Every case also
differs from the default mode on more than 20 % of its outputs, in SciPy's result.
"""
import functools
import types

import numpy as np
import pytest
import scipy.ndimage

from sofima_amd import _abi, _spline, warp
from tests import ndwarp_modes_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.float32)
CVAL = 7.25


def assert_same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


@pytest.fixture(autouse=True)
def spline_orders():
  with _abi.option(_spline.OPTION, 1):
    yield


def sampler(mode, cval):
  return functools.partial(scipy.ndimage.map_coordinates, mode=mode, cval=cval)


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


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('mode', ref.MODES)
def test_modes_against_scipy(gpu, mode, order, dtype):
  rng = np.random.default_rng(100 * ref.MODES.index(mode) + 10 * order + np.dtype(dtype).itemsize)
  for shape in ref.SHAPES_2D + ref.SHAPES_3D:
    img = ref.image(rng, shape, dtype)
    coords = ref.mode_coords(rng, shape)
    got, want, default = warp_at(img, coords, order, mode, CVAL)
    assert_same(got, want, shape)
    assert np.mean(want != default) > 0.2, shape


@pytest.mark.parametrize('order', [2, 3, 4, 5])
@pytest.mark.parametrize('mode', ref.SPLINE_MODES)
def test_high_order_modes_against_scipy(gpu, mode, order):
  rng = np.random.default_rng(1000 + 10 * ref.MODES.index(mode) + order)
  for k, shape in enumerate(ref.SHAPES_2D + ref.SHAPES_3D):
    img = ref.image(rng, shape, DTYPES[(k + order) % 3])
    coords = ref.mode_coords(rng, shape)
    got, want, default = warp_at(img, coords, order, mode, CVAL)
    assert_same(got, want, shape)
    assert np.mean(want != default) > 0.2, shape


@pytest.mark.parametrize('mode,cval', [('nearest', 0.0), ('mirror', 0.0), ('constant', CVAL)])
def test_map_smaller_than_the_output(gpu, mode, cval):
  """The node grid covers a corner of the output: the map step itself leaves it, and the
  dense coordinate there is cval in source voxels, or the folded node value."""
  rng = np.random.default_rng(7)
  for shape, nodes, stride in (((12, 15), (3, 4), (3.0, 2.5)), ((5, 9, 11), (2, 3, 3), (2.0, 2.0, 3.5))):
    for dtype in DTYPES:
      img = ref.image(rng, shape, dtype)
      cmap = rng.uniform(-1.5, 1.5, (len(shape),) + nodes)
      for order in (0, 1, 3) if mode in ref.SPLINE_MODES else (0, 1):
        got = warp.ndimage_warp(img, cmap, stride, shape[::-1], (0,) * len(shape), order=order,
                                map_coordinates=sampler(mode, cval))
        want = ref.ndimage_warp_scipy(img, cmap, stride, order, mode, cval)
        assert_same(got, want, (shape, np.dtype(dtype).name, order))
        default = ref.ndimage_warp_scipy(img, cmap, stride, order, 'constant', 0.0)
        assert np.mean(want != default) > 0.2
        assert_same(warp.ndimage_warp(img, cmap, stride, shape[::-1], (0,) * len(shape),
                                      order=order), default)


@pytest.mark.parametrize('order', [0, 1, 3])
def test_nan_and_huge_coordinates_give_cval(gpu, order):
  """SciPy casts these to an integer under every mode but 'constant' (undefined): the
  device returns cval, through the conversion of a sampled value."""
  rng = np.random.default_rng(9)
  bad = np.array([np.nan, 2.0**31, -2.0**31, 1e300, -1e300, np.inf, -np.inf, 2.0**40 + 0.5])
  for shape in ((5, 7), (3, 4, 6)):
    dim = len(shape)
    n = bad.size * dim
    # finite coordinates first (a node next to a NaN node turns NaN in the order-1 step)
    coords = np.stack([rng.uniform(0, s - 1, 100 + n) for s in shape])
    for d in range(dim):
      coords[d, 100 + d * bad.size:100 + (d + 1) * bad.size] = bad
    cmap, out_shape = ref.stride1_map(coords)
    for dtype in DTYPES:
      img = ref.image(rng, shape, dtype)
      for mode in ref.MODES if order < 2 else ref.SPLINE_MODES:
        got = device_at(img, cmap, out_shape, order,
                        map_coordinates=sampler(mode, 200.7)).ravel()[100:100 + n]
        want = ref.convert(np.full(n, 200.7), dtype)
        assert_same(got, want, (shape, mode, np.dtype(dtype).name))


def test_cval_goes_through_the_conversion(gpu):
  rng = np.random.default_rng(11)
  img = ref.image(rng, (5, 7), np.uint8)
  coords = ref.mode_coords(rng, (5, 7))
  for cval in (-3, 0, 1.5, 200.7, 300):
    for mode in ('constant', 'grid-constant'):
      got, want, _ = warp_at(img, coords, 1, mode, cval)
      assert_same(got, want, (cval, mode))
  for cval in (np.nan, np.inf, -np.inf):
    with pytest.raises(ValueError, match='cval'):
      warp_at(img, coords, 1, 'constant', cval)
    got, want, _ = warp_at(img.astype(np.float32), coords, 1, 'constant', cval)
    assert_same(got, want, cval)


def test_what_is_not_built_raises(gpu):
  img = np.zeros((8, 9), np.uint8)
  cmap = np.zeros((2, 2, 2), np.float32)
  args = (img, cmap, (8, 8), (8, 8), (0, 0))
  for order in _spline.ORDERS:
    for mode in ('reflect', 'grid-mirror', 'nearest', 'grid-wrap', 'grid-constant'):
      with pytest.raises(NotImplementedError, match=f'{mode}.*{order}'):
        warp.ndimage_warp(*args, order=order, map_coordinates=sampler(mode, 0.0))
  with pytest.raises(ValueError, match='bogus'):
    warp.ndimage_warp(*args, map_coordinates=sampler('bogus', 0.0))
  for bad in (lambda *a, **k: None,
              functools.partial(scipy.ndimage.map_coordinates, order=3),
              functools.partial(scipy.ndimage.map_coordinates, img),
              functools.partial(scipy.ndimage.affine_transform, mode='nearest'),
              scipy.ndimage.affine_transform):
    with pytest.raises(NotImplementedError):
      warp.ndimage_warp(*args, map_coordinates=bad)
  # the library rejects them as well
  lib = _abi.load()
  d = _abi.SfmNdWarpDesc()
  d.ndim, d.order = 2, 3
  d.image = d.src_map = d.out = 1      # never reached
  assert lib.sfm_ndimage_warp_mode(d, _abi.MODES['reflect'], 0.0) == -1
  assert b'mode' in lib.sfm_last_error()
  assert lib.sfm_ndimage_warp_mode(d, 7, 0.0) == -1
  d.dtype = _abi.DTYPE_U8
  assert lib.sfm_ndimage_warp_mode(d, 0, float('nan')) == -1
  assert b'cval' in lib.sfm_last_error()


def test_scipy_itself_is_the_default(gpu, golden):
  old = golden('ndimage_warp')
  args = (old['u8_3d_image'], old['u8_3d_map'], tuple(int(v) for v in old['u8_3d_stride']),
          tuple(old['u8_3d_work']), tuple(old['u8_3d_overlap']))
  for order in (0, 1, 3):
    want = warp.ndimage_warp(*args, order=order)
    assert want.any()
    for mc in (scipy.ndimage.map_coordinates, functools.partial(scipy.ndimage.map_coordinates),
               sampler('constant', 0.0), sampler('constant', 0)):
      assert_same(warp.ndimage_warp(*args, order=order, map_coordinates=mc), want, order)
