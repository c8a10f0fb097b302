"""tests/ndwarp_spline_ref.py, the float64 restatement of SciPy's prefiltered spline
sampling that the device kernels are written from, against SciPy itself: element
for element, no tolerance."""
import numpy as np
import pytest
from scipy import ndimage

from tests import ndwarp_spline_ref as ref

DTYPES = (np.uint8, np.uint16, np.float32)


def same(a, b):
  return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_prefilter_equals_spline_filter(order):
  rng = np.random.default_rng(order)
  shapes = ref.EDGE_SHAPES + ((1, 1), (1, 1, 1), (2, 1), (4, 6, 5), (200,))
  for shape in shapes:
    for dtype in DTYPES:
      img = ref.edge_image(rng, shape, dtype)
      want = ndimage.spline_filter(img, order, output=np.float64, mode='constant')
      got = ref.prefilter(img, order)
      assert same(got, want), (shape, dtype)
      # ... and one axis alone
      for axis in range(len(shape)):
        c = img.astype(np.float64)
        ref.filter_axis(c, axis, order)
        assert same(c, ndimage.spline_filter1d(img, order, axis=axis, output=np.float64,
                                               mode='constant')), (shape, dtype, axis)


@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_zn_is_libm_pow(order):
  import math
  t = ref.zn_table(order, (3, 70))       # a 2-D shape is padded in front
  poles = ref.POLES[order]
  assert t.shape == (3, 2) and np.all(t[0, :len(poles)] == 1.0)
  for p, z in enumerate(poles):
    assert t[1, p] == math.pow(z, 2) and t[2, p] == math.pow(z, 69)
  assert np.all(t[:, len(poles):] == 0.0)


@pytest.mark.parametrize('order', [2, 3, 4, 5])
@pytest.mark.parametrize('dtype', DTYPES)
def test_map_coordinates_equals_scipy(order, dtype):
  rng = np.random.default_rng(10 * order + np.dtype(dtype).itemsize)
  for shape in ref.EDGE_SHAPES:
    img = ref.edge_image(rng, shape, dtype)
    coords = ref.edge_coords(rng, shape, order)
    want = ndimage.map_coordinates(img, coords, order=order)
    got = ref.map_coordinates(img, coords, order)
    assert same(got, want), (shape, int((got != want).sum()))
    assert np.mean(want != 0) > 0.3


@pytest.mark.parametrize('order', [2, 3])
def test_float_images_with_inf_and_nan(order):
  """0 x NaN and 0 x inf in the init sweep: the whole line goes NaN in SciPy too."""
  rng = np.random.default_rng(7)
  img = ref.edge_image(rng, (6, 40), np.float32)
  img[2, 30] = np.inf
  img[4, 3] = np.nan
  coords = ref.edge_coords(rng, img.shape, order)
  with np.errstate(all='ignore'):
    want = ndimage.map_coordinates(img, coords, order=order)
  assert same(ref.map_coordinates(img, coords, order), want)


def test_far_voxel_reaches_the_line_start():
  """An all-zero line with one voxel at the far end of a 200-long axis: the init
  sweep has to run the whole line."""
  img = np.zeros((3, 200), np.float32)
  img[1, 199] = 1e30
  for order in (2, 3, 4, 5):
    want = ndimage.spline_filter(img, order, output=np.float64, mode='constant')
    assert same(ref.prefilter(img, order), want)
    assert want[1, 0] != 0.0


@pytest.mark.parametrize('dim', [2, 3])
def test_ndimage_warp_equals_the_oracle(dim):
  from oracle import warp_oracle
  rng = np.random.default_rng(dim)
  if dim == 2:
    img = rng.integers(0, 256, (40, 53)).astype(np.uint8)
    cmap = (rng.standard_normal((2, 5, 6)) * 4).astype(np.float32)
    stride = (10.5, 10.25)
  else:
    img = rng.integers(0, 65536, (9, 20, 17)).astype(np.uint16)
    cmap = (rng.standard_normal((3, 4, 5, 4)) * 2).astype(np.float32)
    stride = (3, 5.0, 5.5)
  for order in (2, 3, 4, 5):
    want = warp_oracle.ndimage_warp(img, cmap, stride, order=order)
    got = ref.ndimage_warp(img, cmap, stride, order)
    assert same(got, want), order
