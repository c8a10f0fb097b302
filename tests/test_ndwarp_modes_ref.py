"""tests/ndwarp_modes_ref.py against SciPy, bit for bit (CPU): the boundary modes and
fill values of scipy.ndimage.map_coordinates at orders 0, 1 and 3, the coordinate
arithmetic of scipy.ndimage.affine_transform, the conversion of `cval` to integer
images, and the B-spline coefficients that the high-order modes share.  The
device samplers are written from that restatement; tests/test_gpu_ndwarp_modes.py
and tests/test_gpu_affine_warp.py compare them with SciPy again."""
import numpy as np
import pytest
from scipy import ndimage

from tests import ndwarp_modes_ref as ref
from tests import ndwarp_spline_ref as spline_ref

SHAPES = ((1, 1), (1, 5), (5, 1), (2, 3), (2, 2, 2), (1, 4, 3), (3, 1, 4), (5, 7), (3, 4, 6),
          (130, 70), (3, 66, 33))


def assert_same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    bits = np.uint32 if want.dtype == np.float32 else np.uint64
    differ = got.view(bits) != want.view(bits)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


def test_shapes_are_the_shared_ones():
  assert set(SHAPES) == set(ref.SHAPES_2D + ref.SHAPES_3D)


def test_axis_coords():
  c = ref.axis_coords(5)
  for v in (-11.0, -10.5, 16.0, 15.5, 0.0, 4.0, -0.5 - 1e-9, -0.5 + 1e-9, 1e-9, -1e-9,
            4.0 - 1e-9, 4.0 + 1e-9, 4.5 - 1e-9, 4.5 + 1e-9, 5.0 - 1e-9, 5.0 + 1e-9,
            1e6 + 0.25, -1e6 - 0.25):
    assert v in c, v
  assert c.min() == -1e6 - 0.25 and np.sort(c)[1] == -11.0


@pytest.mark.parametrize('order', [0, 1, 3])
@pytest.mark.parametrize('mode', ref.MODES)
def test_map_coordinates(order, mode):
  if order > 1 and mode not in ref.SPLINE_MODES:
    with pytest.raises(NotImplementedError, match=mode):
      ref.map_coordinates(np.zeros((3, 3)), np.zeros((2, 1)), order, mode)
    return
  rng = np.random.default_rng(10 * order + ref.MODES.index(mode))
  for shape in SHAPES:
    coords = ref.mode_coords(rng, shape)
    for dtype, cval in ((np.uint8, 200.7), (np.uint16, 7.25), (np.float32, -3.5),
                        (np.float64, 7.25)):
      img = ref.image(rng, shape, dtype)
      want = ndimage.map_coordinates(img, coords, order=order, mode=mode, cval=cval)
      assert_same(ref.map_coordinates(img, coords, order, mode, cval), want,
                  (shape, np.dtype(dtype).name))
      if mode != 'constant' and dtype == np.float64 and max(shape) > 1:
        default = ndimage.map_coordinates(img, coords, order=order)
        assert np.mean(want != default) > 0.2, shape


@pytest.mark.parametrize('mode', ref.MODES)
def test_taps_of_weight_zero(mode):
  """0 x inf is NaN: which sample a tap of weight 0 reads shows in the result."""
  rng = np.random.default_rng(3)
  for n in (1, 2, 3, 5):
    c = ref.axis_coords(n)[None]
    for k in range(n):
      img = rng.uniform(20.0, 300.0, n)
      img[k] = np.inf
      with np.errstate(all='ignore'):
        want = ndimage.map_coordinates(img, c, order=1, mode=mode, cval=7.25)
      assert_same(ref.map_coordinates(img, c, 1, mode, 7.25), want, (n, k))


@pytest.mark.parametrize('order', [0, 1, 3])
def test_cval_conversions(order):
  """An integer image takes cval through the conversion of a sampled value; float32
  takes NaN and the infinities."""
  rng = np.random.default_rng(5)
  img = ref.image(rng, (5, 7), np.uint8)
  coords = ref.mode_coords(rng, (5, 7))
  for cval, stored in ((-3, 0), (0, 0), (1.5, 2), (200.7, 201), (300, 255)):
    for mode in ('constant', 'grid-constant') if order < 2 else ('constant',):
      want = ndimage.map_coordinates(img, coords, order=order, mode=mode, cval=cval)
      assert_same(ref.map_coordinates(img, coords, order, mode, cval), want, (cval, mode))
    far = ndimage.map_coordinates(img, [[-50.0], [3.0]], order=order, cval=cval)
    assert far[0] == stored
  img = img.astype(np.float32)
  for cval in (np.nan, np.inf, -np.inf):
    for mode in ('constant', 'grid-constant') if order < 2 else ('constant',):
      with np.errstate(all='ignore'):
        want = ndimage.map_coordinates(img, coords, order=order, mode=mode, cval=cval)
      assert_same(ref.map_coordinates(img, coords, order, mode, cval), want, (cval, mode))


@pytest.mark.parametrize('order', [2, 3, 5])
def test_high_order_modes_share_the_mirror_coefficients(order):
  rng = np.random.default_rng(order)
  for shape in ((2, 3), (5, 7), (3, 4, 6), (1, 4, 3)):
    img = ref.image(rng, shape, np.float32)
    mirror = spline_ref.prefilter(img, order)
    for mode in ('mirror', 'constant', 'grid-constant', 'wrap'):
      got = ndimage.spline_filter(img, order, output=np.float64, mode=mode)
      assert_same(got, mirror, (shape, mode))
    reflect = ndimage.spline_filter(img, order, output=np.float64, mode='reflect')
    assert_same(ndimage.spline_filter(img, order, output=np.float64, mode='nearest'), reflect)
    assert not np.array_equal(reflect, mirror)
    assert not np.array_equal(
        ndimage.spline_filter(img, order, output=np.float64, mode='grid-wrap'), mirror)


@pytest.mark.parametrize('shape', SHAPES)
def test_affine_coordinate_order(shape):
  """Products added in axis order onto 0, the offset last: order 1 on a float64 image
  shows every rounding of the coordinate."""
  rng = np.random.default_rng(sum(shape))
  dim = len(shape)
  img = rng.uniform(20.0, 300.0, shape)
  other = 0
  total = 0
  for name, m, off in ref.matrices(rng, dim):
    want = ndimage.affine_transform(img, m, off, order=1)
    assert_same(ref.affine_transform(img, m, off, 1), want, name)
    first = ref.map_coordinates(img, ref.affine_coords(shape, m, off, offset_first=True), 1)
    if name.startswith('random'):
      inside = want != 0
      other += int(np.sum(first[inside] != want[inside]))
      total += int(inside.sum())
  if min(shape) >= 3:
    assert other > 0.05 * total, (other, total)


@pytest.mark.parametrize('order', [0, 1, 3])
def test_affine_transform(order):
  rng = np.random.default_rng(40 + order)
  for shape in ((2, 3), (5, 7), (1, 4, 3), (3, 4, 6)):
    dim = len(shape)
    for dtype in (np.uint8, np.float32):
      img = ref.image(rng, shape, dtype)
      for name, m, off in ref.matrices(rng, dim):
        for mode in ref.MODES if order < 2 else ref.SPLINE_MODES:
          want = ndimage.affine_transform(img, m, off, order=order, mode=mode, cval=7.25)
          assert_same(ref.affine_transform(img, m, off, order, mode, 7.25), want,
                      (shape, name, mode))
        # the three matrix shapes
        m34 = np.concatenate([m, off[:, None]], axis=1)
        m44 = np.concatenate([m34, [[0.0] * dim + [1.0]]], axis=0)
        want = ndimage.affine_transform(img, m, off, order=order)
        for mat in (m34, m44):
          assert_same(ndimage.affine_transform(img, mat, order=order), want, name)
          assert_same(ref.affine_transform(img, mat, order=order), want, name)
