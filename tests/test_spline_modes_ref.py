"""tests/spline_modes_ref.py against SciPy itself, bit for bit: the reflect and wrap
initialisations of the B-spline prefilter, and the pad-filter-shift rule of
map_coordinates for 'nearest' and 'grid-constant' at orders 2 to 5."""
import numpy as np
import pytest
from scipy import ndimage

from tests import spline_modes_ref as ref

LENGTHS = (2, 3, 4, 5, 7, 13, 40, 200)
ORDERS = (2, 3, 4, 5)


def same_bits(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    bits = np.uint32 if want.dtype == np.float32 else np.uint64
    differ = got.view(bits) != want.view(bits)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


def line(rng, n, dtype):
  if np.dtype(dtype).kind == 'f':
    return rng.uniform(-50.0, 300.0, n).astype(dtype)
  return rng.integers(0, 256, n).astype(dtype)


@pytest.mark.parametrize('mode', ['reflect', 'grid-mirror', 'nearest', 'grid-wrap'])
@pytest.mark.parametrize('order', ORDERS)
def test_spline_filter1d(order, mode):
  rng = np.random.default_rng(order)
  for dtype in (np.uint8, np.float32):
    for n in LENGTHS:
      x = line(rng, n, dtype)
      want = ndimage.spline_filter1d(x, order, output=np.float64, mode=mode)
      same_bits(ref.prefilter(x, order, mode), want, (n, dtype))


@pytest.mark.parametrize('order', ORDERS)
def test_spline_filter_nd(order):
  rng = np.random.default_rng(10 + order)
  for shape in ((5, 7), (3, 4, 6), (1, 5, 2)):
    x = rng.uniform(-5.0, 30.0, shape).astype(np.float32)
    for mode in ('reflect', 'grid-wrap'):
      want = ndimage.spline_filter(x, order, output=np.float64, mode=mode)
      same_bits(ref.prefilter(x, order, mode), want, (shape, mode))


def outside_coords(rng, shape, n=300):
  """[ndim, n] coordinates from 3 lengths + 30 outside the array on either side (well
  past the pad of 12) to inside it, with integers and half-integers among them."""
  cols = [np.stack([rng.uniform(-3.0 * s - 30.0, 4.0 * s + 30.0, n) for s in shape]),
          np.stack([rng.uniform(-14.0, s + 13.0, n) for s in shape]),
          np.stack([rng.uniform(0.0, s - 1.0, n) for s in shape]),
          np.stack([rng.integers(-30, s + 30, n) * 0.5 for s in shape])]
  return np.concatenate(cols, axis=1)


@pytest.mark.parametrize('mode,cval', [('nearest', 0.0), ('grid-constant', 37.5),
                                        ('grid-constant', -3.0)])
@pytest.mark.parametrize('order', ORDERS)
def test_padded_rule_is_map_coordinates(order, mode, cval):
  rng = np.random.default_rng(20 + order)
  for shape in ((2, 3), (5, 7), (13, 4), (3, 4, 6), (1, 5, 2)):
    for dtype in (np.uint8, np.float32):
      x = line(rng, shape, dtype)
      coords = outside_coords(rng, shape)
      with np.errstate(all='ignore'):
        want = ndimage.map_coordinates(x, coords, output=np.float64, order=order, mode=mode,
                                       cval=cval)
        coeffs, shift = ref.padded_coefficients(x, order, mode, cval)
        got = ref.modes_ref.sample(coeffs, coords + shift, order, mode, cval)
        same_bits(got, want, (shape, dtype))
        # ... and in the image's type, and identical to prefilter=False on the shifted
        # coordinates
        same_bits(ref.map_coordinates(x, coords, order, mode, cval),
                  ndimage.map_coordinates(x, coords, order=order, mode=mode, cval=cval),
                  (shape, dtype))
        same_bits(ndimage.map_coordinates(coeffs, coords + shift, output=np.float64, order=order,
                                          mode=mode, cval=cval, prefilter=False), want)


@pytest.mark.parametrize('mode', ['reflect', 'grid-mirror', 'grid-wrap'])
@pytest.mark.parametrize('order', ORDERS)
def test_unpadded_modes_are_map_coordinates(order, mode):
  rng = np.random.default_rng(30 + order)
  for shape in ((2, 3), (5, 7), (3, 4, 6), (1, 5, 2)):
    x = line(rng, shape, np.float32)
    coords = outside_coords(rng, shape)
    same_bits(ref.map_coordinates(x, coords, order, mode),
              ndimage.map_coordinates(x, coords, order=order, mode=mode), (shape,))


def test_pad_is_np_pad():
  x = np.arange(6, dtype=np.uint8).reshape(2, 3) + 20
  with np.errstate(all='ignore'):
    for cval in (-3.0, 1.5, 300.0, 7.0):
      np.testing.assert_array_equal(ref.pad(x, 'grid-constant', cval),
                                    np.pad(x, 12, mode='constant', constant_values=cval))
  xf = x.astype(np.float32)
  same_bits(ref.pad(xf, 'grid-constant', 0.1), np.pad(xf, 12, mode='constant',
                                                     constant_values=0.1))
  np.testing.assert_array_equal(ref.pad(x, 'nearest'), np.pad(x, 12, mode='edge'))
  assert ref.pad(x, 'reflect') is x


@pytest.mark.parametrize('order', [2, 3, 5])
def test_equality_classes(order):
  """mirror = constant = grid-constant = wrap; reflect = nearest = grid-mirror;
  grid-wrap differs from both."""
  rng = np.random.default_rng(40 + order)
  x = rng.uniform(0.0, 255.0, (9, 11))

  def f(mode):
    return ndimage.spline_filter(x, order, output=np.float64, mode=mode)

  for mode in ('constant', 'grid-constant', 'wrap'):
    same_bits(f(mode), f('mirror'), mode)
    assert ref.INIT[mode] == 'mirror'
  for mode in ('nearest', 'grid-mirror'):
    same_bits(f(mode), f('reflect'), mode)
    assert ref.INIT[mode] == 'reflect'
  assert ref.INIT['grid-wrap'] == 'wrap'
  assert (f('reflect') != f('mirror')).any()
  assert (f('grid-wrap') != f('mirror')).any()
  assert (f('grid-wrap') != f('reflect')).any()
  same_bits(ref.prefilter(x, order, 'mirror'), f('mirror'))
