"""`warp.affine_transform` on the device (-m gpu) against scipy.ndimage.affine_transform,
2-D and 3-D: the fused kernel forms the source coordinates from the matrix (no map)
and runs the samplers of sfm_ndsample.h with SciPy's boundary mode and fill value.
Integer images compare with array_equal, float32 images by their bits.  The
coordinate arithmetic and the samplers are pinned on the CPU first
(tests/test_ndwarp_modes_ref.py), on the same matrices (`ndwarp_modes_ref.matrices`)."""
import numpy as np
import pytest
from scipy import ndimage

from sofima_amd import _abi, _spline, warp
from tests import ndwarp_modes_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.float32)
SHAPES = ref.SHAPES_2D + ref.SHAPES_3D
# the cases that assert their coverage: under 'constant' the matrices that keep the
# output over the image, on shapes with no axis shorter than 3 (a short axis leaves
# with the first shift or turn); under every other mode each output is an image value
COVERING = ('identity', 'shift_int', 'shift_half', 'rot_shear_scale')


def covering(shape, name, mode='constant'):
  return mode != 'constant' or (name in COVERING and min(shape) >= 3)


def assert_same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


@pytest.fixture(autouse=True)
def spline_orders(request):
  if request.node.name == 'test_orders_above_1_are_opt_in':
    yield
    return
  with _abi.option(_spline.OPTION, 1):
    yield


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('order', [0, 1, 3])
def test_matrices_against_scipy(gpu, order, dtype):
  """Every matrix on every shape, default mode."""
  rng = np.random.default_rng(10 * order + np.dtype(dtype).itemsize)
  for shape in SHAPES:
    img = ref.image(rng, shape, dtype)
    for name, m, off in ref.matrices(rng, len(shape)):
      want = ndimage.affine_transform(img, m, off, order=order)
      assert_same(warp.affine_transform(img, m, off, order=order), want, (shape, name))
      if covering(shape, name):
        assert np.mean(want != 0) > 0.2, (shape, name)


@pytest.mark.parametrize('order', [2, 4, 5])
def test_other_orders(gpu, order):
  rng = np.random.default_rng(order)
  for shape, dtype in (((5, 7), np.uint8), ((3, 4, 6), np.float32), ((130, 70), np.uint16)):
    img = ref.image(rng, shape, dtype)
    name, m, off = ref.matrices(rng, len(shape))[4]
    assert name == 'rot_shear_scale'
    for mode in ref.SPLINE_MODES:
      want = ndimage.affine_transform(img, m, off, order=order, mode=mode, cval=7.25)
      assert_same(warp.affine_transform(img, m, off, order=order, mode=mode, cval=7.25), want,
                  (shape, mode))
      assert np.mean(want != 0) > 0.2


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('mode', ref.MODES)
def test_modes_against_scipy(gpu, mode, order, dtype):
  rng = np.random.default_rng(100 * ref.MODES.index(mode) + 10 * order + np.dtype(dtype).itemsize)
  for shape in SHAPES:
    img = ref.image(rng, shape, dtype)
    for name, m, off in ref.matrices(rng, len(shape))[1:6]:
      want = ndimage.affine_transform(img, m, off, order=order, mode=mode, cval=7.25)
      got = warp.affine_transform(img, m, off, order=order, mode=mode, cval=7.25)
      assert_same(got, want, (shape, name))
      if covering(shape, name, mode):
        assert np.mean(want != 0) > 0.2, (shape, name)


@pytest.mark.parametrize('mode', ref.SPLINE_MODES)
def test_order_3_modes_against_scipy(gpu, mode):
  rng = np.random.default_rng(31)
  for k, shape in enumerate(SHAPES):
    img = ref.image(rng, shape, DTYPES[k % 3])
    for name, m, off in ref.matrices(rng, len(shape))[2:6]:
      want = ndimage.affine_transform(img, m, off, order=3, mode=mode, cval=7.25)
      assert_same(warp.affine_transform(img, m, off, order=3, mode=mode, cval=7.25), want,
                  (shape, name))


def test_the_three_matrix_shapes(gpu):
  rng = np.random.default_rng(3)
  for shape in ((5, 7), (3, 4, 6)):
    dim = len(shape)
    img = ref.image(rng, shape, np.float32)
    name, m, off = ref.matrices(rng, dim)[4]
    want = ndimage.affine_transform(img, m, off, order=1)      # (SciPy's default is 3)
    assert np.mean(want != 0) > 0.2
    m34 = np.concatenate([m, off[:, None]], axis=1)
    m44 = np.concatenate([m34, [[0.0] * dim + [1.0]]], axis=0)
    for mat in (m34, m44, m34.tolist()):
      assert_same(warp.affine_transform(img, mat), want)
      # like SciPy, the offset argument is ignored with these
      assert_same(warp.affine_transform(img, mat, offset=5.0), want)
    assert_same(warp.affine_transform(img, m, 1.5), ndimage.affine_transform(img, m, 1.5, order=1))
    m44[dim, 0] = 0.5
    with pytest.raises(ValueError):
      warp.affine_transform(img, m44)


def test_cval_goes_through_the_conversion(gpu):
  rng = np.random.default_rng(4)
  img = ref.image(rng, (5, 7), np.uint8)
  name, m, off = ref.matrices(rng, 2)[5]
  assert name == 'mostly_outside'
  for cval, stored in ((-3, 0), (0, 0), (1.5, 2), (200.7, 201), (300, 255)):
    want = ndimage.affine_transform(img, m, off, order=1, cval=cval)
    assert want[-1, -1] == stored
    assert_same(warp.affine_transform(img, m, off, cval=cval), want, cval)
  for cval in (np.nan, np.inf, -np.inf):
    with pytest.raises(ValueError, match='cval'):
      warp.affine_transform(img, m, off, cval=cval)
    f32 = img.astype(np.float32)
    assert_same(warp.affine_transform(f32, m, off, cval=cval),
                ndimage.affine_transform(f32, m, off, order=1, cval=cval), cval)


def test_nan_and_huge_coordinates_give_cval(gpu):
  img = ref.image(np.random.default_rng(5), (5, 7), np.uint8)
  for mode in ref.MODES:
    for off in (np.nan, 2.0**31, -1e300, np.inf):
      got = warp.affine_transform(img, np.eye(2), [off, 0.0], mode=mode, cval=200.7)
      assert (got == 201).all(), (mode, off)
    got = warp.affine_transform(img, [[2.0**31, 0.0], [0.0, 1.0]], mode=mode, cval=200.7)
    assert (got[1:] == 201).all(), mode      # row 0 samples row 0


def test_orders_above_1_are_opt_in(gpu):
  img = np.arange(72, dtype=np.uint8).reshape(8, 9)
  assert _abi.get_option(_spline.OPTION) in (None, '0')
  for order in _spline.ORDERS:
    with pytest.raises(NotImplementedError, match=_spline.OPTION):
      warp.affine_transform(img, np.eye(2), order=order)
  assert_same(warp.affine_transform(img, np.eye(2)), img)


def test_what_is_not_built_raises(gpu):
  img = np.zeros((8, 9), np.uint8)
  with pytest.raises(NotImplementedError, match='diagonal'):
    warp.affine_transform(img, [1.0, 2.0])
  with pytest.raises(NotImplementedError, match='output_shape'):
    warp.affine_transform(img, np.eye(2), output_shape=(4, 4))
  with pytest.raises(NotImplementedError, match='output'):
    warp.affine_transform(img, np.eye(2), output=np.float32)
  for order in _spline.ORDERS:
    for mode in ('reflect', 'nearest', 'grid-wrap', 'grid-constant'):
      with pytest.raises(NotImplementedError, match=f'{mode}.*{order}'):
        warp.affine_transform(img, np.eye(2), order=order, mode=mode)
  for order in (6, -1):
    with pytest.raises(NotImplementedError):
      warp.affine_transform(img, np.eye(2), order=order)
  with pytest.raises(NotImplementedError):
    warp.affine_transform(img.astype(np.int32), np.eye(2))
  with pytest.raises(NotImplementedError):
    warp.affine_transform(img.astype(np.uint64), np.eye(2))
  with pytest.raises(ValueError):
    warp.affine_transform(np.zeros(5, np.uint8), np.eye(1))
  with pytest.raises(RuntimeError):
    warp.affine_transform(img, np.eye(4))
  with pytest.raises(RuntimeError):
    warp.affine_transform(img, np.eye(2), offset=[1.0, 2.0, 3.0])
  with pytest.raises(ValueError, match='bogus'):
    warp.affine_transform(img, np.eye(2), mode='bogus')
