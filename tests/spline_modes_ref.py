"""NumPy restatement of SciPy's B-spline prefilter for the boundary modes that do
not use the mirror initialisation, and of the padding that `map_coordinates` and
`affine_transform` put in front of it, in plain float64 arithmetic and in SciPy's
operation order.  tests/test_spline_modes_ref.py pins it to SciPy bit for bit; the
new variants of the device kernels (sfm_spline.hip) are written from this file.

`scipy.ndimage.spline_filter` initialises its recursion in one of three ways:
  * mirror   'mirror', 'constant', 'grid-constant', 'wrap'
             (tests/ndwarp_spline_ref.filter_axis)
  * reflect  'reflect', 'grid-mirror', 'nearest'
  * wrap     'grid-wrap'
`map_coordinates` pads the image by 12 samples on every axis before it filters for
'nearest' (edge values) and 'grid-constant' (cval, cast to the image's type as
np.pad casts it), and samples the padded coefficients at coordinate + 12 with the
same mode: `padded_coefficients` and `map_coordinates` below.
"""
import math

import numpy as np

from tests import ndwarp_modes_ref as modes_ref
from tests import ndwarp_spline_ref as spline_ref

POLES = spline_ref.POLES
PAD = 12
NEW_MODES = ('nearest', 'reflect', 'grid-mirror', 'grid-constant', 'grid-wrap')
INIT = {'mirror': 'mirror', 'constant': 'mirror', 'grid-constant': 'mirror', 'wrap': 'mirror',
        'reflect': 'reflect', 'grid-mirror': 'reflect', 'nearest': 'reflect',
        'grid-wrap': 'wrap'}
PADDED = ('nearest', 'grid-constant')


def filter_axis(c, axis, order, init):
  """One spline_filter1d pass over `axis` of the float64 array `c`, in place, every
  line at once, with the initialisation `init` of the recursion."""
  if init == 'mirror':
    spline_ref.filter_axis(c, axis, order)
    return
  c = np.moveaxis(c, axis, 0)
  n = c.shape[0]
  if n == 1:
    return
  c *= spline_ref.gain(order)
  for z in POLES[order]:
    if init == 'reflect':
      zn = math.pow(z, n)
      c0 = c[0].copy()
      c[0] = c[0] + zn * c[n - 1]
      zi = z
      for i in range(1, n):            # i = n - 1 pairs c[n-1] with the running c[0]
        c[0] += zi * (c[i] + zn * c[n - 1 - i])
        zi *= z
      c[0] *= z / (1.0 - zn * zn)
      c[0] += c0
      for i in range(1, n):
        c[i] += z * c[i - 1]
      c[n - 1] *= z / (z - 1.0)
    else:
      assert init == 'wrap'
      zi = z
      for i in range(1, n):
        c[0] += zi * c[n - i]
        zi *= z
      c[0] /= 1.0 - zi
      for i in range(1, n):
        c[i] += z * c[i - 1]
      zi = z
      for i in range(0, n - 1):
        c[n - 1] += zi * c[i]
        zi *= z
      c[n - 1] *= z / (zi - 1.0)
    for i in range(n - 2, -1, -1):
      c[i] = z * (c[i + 1] - c[i])


def prefilter(image, order, mode):
  """scipy.ndimage.spline_filter(image, order, output=float64, mode=mode)."""
  c = np.array(image, dtype=np.float64, copy=True, order='C')
  with np.errstate(all='ignore'):
    for axis in range(c.ndim):
      filter_axis(c, axis, order, INIT[mode])
  return c


def pad_value(cval, dtype):
  """`cval` as np.pad stores it in an array of `dtype`."""
  a = np.empty(1, np.dtype(dtype))
  with np.errstate(all='ignore'):
    a[...] = np.float64(cval)
  return a[0]


def pad(image, mode, cval=0.0):
  """The array SciPy filters in place of `image`."""
  image = np.asarray(image)
  if mode == 'nearest':
    return np.pad(image, PAD, mode='edge')
  if mode == 'grid-constant':
    out = np.empty(tuple(s + 2 * PAD for s in image.shape), image.dtype)
    out[...] = pad_value(cval, image.dtype)
    out[tuple(slice(PAD, PAD + s) for s in image.shape)] = image
    return out
  return image


def padded_coefficients(image, order, mode, cval=0.0):
  """(float64 coefficients that the sampler reads, the shift of its coordinates)."""
  if mode in PADDED:
    return prefilter(pad(image, mode, cval), order, mode), float(PAD)
  return prefilter(image, order, mode), 0.0


def map_coordinates(image, coords, order, mode, cval=0.0):
  """scipy.ndimage.map_coordinates(image, coords, order=order, mode=mode, cval=cval)
  for orders 2 to 5 and every mode."""
  image = np.asarray(image)
  coeffs, shift = padded_coefficients(image, order, mode, cval)
  coords = np.asarray(coords, np.float64)
  if shift:
    coords = coords + shift
  return modes_ref.convert(modes_ref.sample(coeffs, coords, order, mode, cval), image.dtype)
