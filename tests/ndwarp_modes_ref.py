"""NumPy restatement of scipy.ndimage.map_coordinates and affine_transform with a
boundary mode and a fill value, in plain float64 arithmetic and in SciPy's
operation order.  tests/test_ndwarp_modes_ref.py pins it to SciPy bit for bit; the
device samplers (sfm_ndsample.h) and affine_warp_kernel (sfm_ndwarp_kernel.h) are written
from this file.

Per axis of length `len` a sample is formed in three steps:
  * `fold_coordinate`: a coordinate outside [0, len - 1] is folded by the mode
    ("constant" marks it outside: the whole sample is `cval`; "grid-constant"
    and "nearest" leave it where it is, weights included, and treat the taps);
  * base tap floor(c) (odd orders) or floor(c + 0.5) (even orders, order 0
    included), order + 1 taps from base - order // 2, weights from the folded
    coordinate;
  * `fold_tap`: a tap index outside [0, len - 1] is folded by the mode as well
    ("constant" and "wrap" mirror it; "nearest" clamps it; "grid-constant" reads
    `cval` there instead).
Orders 2 to 5 sample the mirror B-spline coefficients of the image
(tests/ndwarp_spline_ref.prefilter), which SciPy computes for "constant",
"mirror" and "wrap" alike; the other modes use another prefilter and are not
restated.  A NaN coordinate or one of magnitude >= 2^31 gives `cval` under every
mode: SciPy casts those to an integer, which is undefined, except under
"constant", where they are simply outside.
"""
import numpy as np

from tests import ndwarp_spline_ref as spline_ref

MODES = ('constant', 'grid-constant', 'nearest', 'mirror', 'reflect', 'grid-mirror', 'wrap',
         'grid-wrap')
SPLINE_MODES = ('constant', 'mirror', 'wrap')      # orders 2 to 5
_ALIAS = {'grid-mirror': 'reflect'}
HUGE = 2.0**31

SHAPES_2D = ((1, 1), (1, 5), (5, 1), (2, 3), (5, 7), (130, 70))
SHAPES_3D = ((2, 2, 2), (1, 4, 3), (3, 1, 4), (3, 4, 6), (3, 66, 33))


def _trunc(x):
  return np.trunc(x)


def fold_coordinate(c, n, mode):
  """(folded float64 coordinate, outside) of the coordinates `c` on an axis of
  length `n`; `outside` marks samples that are `cval` as a whole."""
  mode = _ALIAS.get(mode, mode)
  c = np.array(c, np.float64, copy=True)
  bad = ~(np.abs(c) < HUGE)                       # NaN, inf, huge
  c[bad] = 0.0
  lo = c < 0
  hi = c > n - 1
  out = c.copy()
  outside = bad.copy()
  with np.errstate(all='ignore'):
    if mode == 'constant':
      outside |= lo | hi
    elif mode in ('grid-constant', 'nearest'):
      pass                  # "nearest" clamps the taps, not the coordinate
    elif n <= 1:
      out[lo | hi] = 0.0
    elif mode == 'mirror':
      sz2 = 2 * n - 2
      v = c[lo]
      v = sz2 * _trunc(-v / sz2) + v
      out[lo] = np.where(v <= 1 - n, v + sz2, -v)
      v = c[hi]
      v = v - sz2 * _trunc(v / sz2)
      out[hi] = np.where(v >= n, sz2 - v, v)
    elif mode == 'reflect':
      sz2 = 2 * n
      v = c[lo]
      v = np.where(v < -sz2, sz2 * _trunc(-v / sz2) + v, v)
      out[lo] = np.where(v < -n, v + sz2, np.where(v > -1e-15, 1e-15, -v) - 1)
      v = c[hi]
      v = v - sz2 * _trunc(v / sz2)
      out[hi] = np.where(v >= n, sz2 - v - 1, v)
    elif mode == 'wrap':
      sz = n - 1
      v = c[lo]
      out[lo] = v + sz * (_trunc(-v / sz) + 1)
      v = c[hi]
      out[hi] = v - sz * _trunc(v / sz)
    elif mode == 'grid-wrap':
      v = c[lo]
      out[lo] = v + n * (_trunc((-1 - v) / n) + 1)
      v = c[hi]
      v = v - n * _trunc((v + 1) / n)
      out[hi] = np.where(v < 0, v + n, v)
    else:
      raise ValueError(mode)
  return out, outside


def fold_tap(i, n, mode):
  """(index inside [0, n - 1], reads cval) of the integer tap indices `i`."""
  mode = _ALIAS.get(mode, mode)
  i = np.asarray(i, np.int64)
  fill = np.zeros(i.shape, bool)
  if mode == 'grid-constant':
    fill = (i < 0) | (i >= n)
    return np.clip(i, 0, n - 1), fill
  if n <= 1:
    return np.zeros_like(i), fill
  if mode == 'nearest':
    return np.clip(i, 0, n - 1), fill
  if mode in ('constant', 'mirror', 'wrap'):
    # "wrap" folds the coordinate with period n - 1 and then mirrors its taps
    p = 2 * n - 2
    j = np.abs(i) % p
    return np.where(j >= n, p - j, j), fill
  if mode == 'reflect':
    p = 2 * n
    j = np.mod(i, p)
    return np.where(j >= n, p - 1 - j, j), fill
  if mode == 'grid-wrap':
    return np.mod(i, n), fill
  raise ValueError(mode)


def sample(values, coords, order, mode='constant', cval=0.0):
  """float64 samples of `values` (the image for orders 0 and 1, its mirror
  B-spline coefficients for orders 2 to 5) at `coords` ([ndim, ...])."""
  values = np.asarray(values, np.float64)
  coords = np.asarray(coords, np.float64)
  dim = values.ndim
  out_shape = coords.shape[1:]
  cc = coords.reshape(dim, -1)
  k = order + 1
  outside = np.zeros(cc.shape[1], bool)
  ws, idx, fills = [], [], []
  with np.errstate(all='ignore'):
    for d in range(dim):
      n = values.shape[d]
      c, out_d = fold_coordinate(cc[d], n, mode)
      outside |= out_d
      c = np.where(out_d, 0.0, c)
      base = np.floor(c) if order & 1 else np.floor(c + 0.5)
      if order == 0:
        ws.append([np.ones_like(c)])
      elif order == 1:
        t = c - base
        w0 = 1.0 - t
        ws.append([w0, 1.0 - w0])
      else:
        ws.append(spline_ref.weights(order, c - base))
      start = base.astype(np.int64) - order // 2
      taps, fl = [], []
      for j in range(k):
        i, f = fold_tap(start + j, n, mode)
        taps.append(i)
        fl.append(f)
      idx.append(taps)
      fills.append(fl)
    acc = np.zeros(cc.shape[1], np.float64)
    for tap in np.ndindex(*(k,) * dim):
      v = values[tuple(idx[d][tap[d]] for d in range(dim))]
      fill = np.zeros(cc.shape[1], bool)
      for d in range(dim):
        fill |= fills[d][tap[d]]
      v = np.where(fill, cval, v)
      if order > 0:
        for d in range(dim):
          v = v * ws[d][tap[d]]
      acc = acc + v
  return np.where(outside, cval, acc).reshape(out_shape)


def convert(v, dtype):
  return spline_ref.convert(v, dtype)


def check(order, mode):
  """What is restated (and built): raises NotImplementedError otherwise."""
  if mode not in MODES:
    raise ValueError(f'boundary mode {mode!r}')
  if order > 1 and _ALIAS.get(mode, mode) not in SPLINE_MODES:
    raise NotImplementedError(f'mode {mode!r} at order {order}')


def map_coordinates(image, coords, order=1, mode='constant', cval=0.0):
  """scipy.ndimage.map_coordinates(image, coords, order=order, mode=mode, cval=cval)."""
  image = np.asarray(image)
  check(order, mode)
  values = spline_ref.prefilter(image, order) if order > 1 else image
  return convert(sample(values, coords, order, mode, cval), image.dtype)


def split_matrix(matrix, offset, dim):
  """(matrix [dim, dim], offset [dim]) of the forms scipy's affine_transform takes."""
  matrix = np.asarray(matrix, np.float64)
  if matrix.shape == (dim + 1, dim + 1) or matrix.shape == (dim, dim + 1):
    return np.ascontiguousarray(matrix[:dim, :dim]), np.ascontiguousarray(matrix[:dim, dim])
  assert matrix.shape == (dim, dim), matrix.shape
  offset = np.asarray(offset, np.float64)
  return np.ascontiguousarray(matrix), np.broadcast_to(offset, (dim,)).copy()


def affine_coords(shape, matrix, offset, offset_first=False):
  """[ndim, *shape] source coordinates: products added in axis order onto 0, the
  offset last."""
  dim = len(shape)
  m, off = split_matrix(matrix, offset, dim)
  grid = np.mgrid[tuple(slice(0, s) for s in shape)].astype(np.float64)
  out = np.zeros((dim,) + tuple(shape), np.float64)
  for h in range(dim):
    acc = np.zeros(shape, np.float64) + (off[h] if offset_first else 0.0)
    for k in range(dim):
      acc = acc + grid[k] * m[h, k]
    out[h] = acc if offset_first else acc + off[h]
  return out


def affine_transform(image, matrix, offset=0.0, order=1, mode='constant', cval=0.0):
  """scipy.ndimage.affine_transform(image, matrix, offset, order=order, mode=mode,
  cval=cval) for 2-D matrices."""
  image = np.asarray(image)
  return map_coordinates(image, affine_coords(image.shape, matrix, offset), order, mode, cval)


# -- test inputs shared by the CPU and GPU tests ---------------------------------------
def axis_coords(n):
  """The coordinates of one axis of length `n`: every integer and half-integer from
  -2 n - 1 to 3 n + 1, +-1e-9 around -0.5, 0, n - 1, n - 0.5 and n, and two far ones."""
  grid = np.arange(-2 * n - 1, 3 * n + 1 + 0.25, 0.5)
  near = np.array([-0.5, 0.0, n - 1.0, n - 0.5, float(n)])
  return np.concatenate([grid, near - 1e-9, near + 1e-9, [1e6 + 0.25, -1e6 - 0.25]])


def mode_coords(rng, shape, n_random=40):
  """[ndim, n] coordinates: `axis_coords` on each axis in turn, the other axes at
  random positions inside and around the array; then all axes at once from their
  `axis_coords`, and random points over the array and a rim as large as it."""
  dim = len(shape)
  cols = []
  for d, n in enumerate(shape):
    special = axis_coords(n)
    for rep in range(2):
      c = np.stack([rng.uniform(0, s - 1, special.size) if rep else
                    rng.uniform(-s - 1.0, 2.0 * s, special.size) for s in shape])
      c[d] = special
      cols.append(c)
  m = max(axis_coords(n).size for n in shape)
  cols.append(np.stack([rng.choice(axis_coords(n), m) for n in shape]))
  cols.append(np.stack([rng.uniform(-s - 1.0, 2.0 * s, n_random) for s in shape]))
  cols.append(np.stack([rng.uniform(0, s - 1, n_random) for s in shape]))
  return np.concatenate(cols, axis=1).reshape(dim, -1)


def matrices(rng, dim):
  """(name, matrix [dim, dim], offset [dim]): the cases of the affine tests."""
  eye = np.eye(dim)
  out = [('identity', eye, np.zeros(dim)),
         ('shift_int', eye, np.array([2.0, -1.0, 1.0])[:dim]),
         ('shift_half', eye, np.array([0.5, -0.5, 0.5])[:dim]),
         ('zero', np.zeros((dim, dim)), np.array([1.25, 0.5, 1.0])[:dim])]
  a = 0.3
  rot = np.eye(dim)
  rot[-2:, -2:] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
  shear = np.eye(dim)
  shear[-1, -2] = 0.15
  if dim == 3:
    shear[0, 2] = 0.05
  scale = np.diag([1.1, 0.9, 1.05][:dim])
  out.append(('rot_shear_scale', rot @ shear @ scale, np.array([0.3, -0.7, 0.2])[:dim]))
  out.append(('mostly_outside', 3.0 * eye + 0.01, np.array([-1.5, 0.25, -2.0])[:dim]))
  for k in range(3):
    out.append((f'random{k}', eye + rng.uniform(-0.3, 0.3, (dim, dim)), rng.uniform(-2, 2, dim)))
  return out


def image(rng, shape, dtype):
  """Values well away from 0 and from the fill values the tests use."""
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    return rng.uniform(20.0, 300.0, shape).astype(dtype)
  return rng.integers(20, np.iinfo(dtype).max + 1, shape).astype(dtype)


# -- warp.ndimage_warp with SciPy's sampler ----------------------------------------------
def ndimage_warp_scipy(image, coord_map, stride, order, mode, cval, out_shape=None):
  """warp.ndimage_warp (warp.py:189-335) with map_coordinates=partial(scipy's, mode=,
  cval=), one work box, no boxes but an output shape: SciPy itself on both steps."""
  from scipy import ndimage
  image = np.asarray(image)
  coord_map = np.asarray(coord_map)
  dim = coord_map.shape[0]
  src = np.array(coord_map, copy=True)
  grid = np.mgrid[tuple(slice(0, s) for s in coord_map.shape[1:])]
  for i in range(dim):
    src[i, ...] += grid[dim - 1 - i] * stride[dim - 1 - i]
  out_shape = image.shape if out_shape is None else tuple(out_shape)
  pos = np.mgrid[tuple(slice(0, s) for s in out_shape)]
  pos = [(c - 0) / s for c, s in zip(pos, stride)]
  with np.errstate(all='ignore'):
    dense = [ndimage.map_coordinates(ev, pos, order=1, mode=mode, cval=cval) for ev in src[::-1]]
    return ndimage.map_coordinates(image, dense, order=order, mode=mode, cval=cval)


def stride1_map(coords, width=48):
  """(relative float64 map, out_shape) whose absolute stride-1 nodes hold `coords`
  [ndim, n] in row-major order, zero-padded to whole rows."""
  dim, n = coords.shape
  rows = -(-n // width)
  out_shape = (1,) * (dim - 2) + (rows, width)
  full = np.zeros((dim, rows * width))
  full[:, :n] = coords
  absolute = full.reshape((dim,) + out_shape)[::-1]      # channels x, y[, z]
  idx = np.mgrid[tuple(slice(0, s) for s in out_shape)][::-1]
  return np.ascontiguousarray(absolute - idx), out_shape
