"""NumPy statement of the map geometry helpers and of warp.warp_points.

Written from the contract, not from the reference's text: offsets are float64
arrays `index * stride (+ start * stride)`, added to (subtracted from) the
widened map and narrowed once to the map's dtype; boxes are reduced from the
extents of that absolute map with the reference's integer expressions; the
affine map is a left-to-right float64 sum; a warped point is the four-term
bilinear combination of its surrounding nodes in float64, narrowed to float32.
`tests/test_mapgeom_refs.py` pins all of it against the reference's own output
(tests/golden/mapgeom.npz).
"""
import numpy as np


class Box:
  """xyz box with integer arrays, built like the reference's: Box(start=, size=)."""

  def __init__(self, start, size):
    self.start = np.array(start)
    self.size = np.array(size)

  def __repr__(self):
    return f'Box(start={self.start}, size={self.size})'


def _vec(value, dim):
  if np.ndim(value) == 0:
    return (value,) * dim
  assert len(value) == dim
  return tuple(value)


def _offsets(shape, stride, box):
  """Per channel (x, y[, z]) the float64 offset array, broadcastable to [z, y, x]."""
  dim = len(stride)
  out = []
  for c in range(dim):
    axis = 3 - 1 - c                      # channel 0 runs along x, the last axis
    idx = np.arange(shape[axis], dtype=np.float64)
    off = idx * np.float64(stride[dim - 1 - c])
    if box is not None:
      off = off + np.float64(box.start[c]) * np.float64(stride[dim - 1 - c])
    view = [1, 1, 1]
    view[axis] = -1
    out.append(off.reshape(view))
  return out


def _check_box(cm, dim, box):
  if box is not None and not np.all(
      np.array(cm.shape[-dim:][::-1]) == np.asarray(box.size)[:dim]):
    raise ValueError(f'box shape ({box.size}) mismatch with coord map ({cm.shape})')


def _shift(coord_map, stride, box, sign):
  cm = np.asarray(coord_map)
  dim = cm.shape[0]
  _check_box(cm, dim, box)
  offs = _offsets(cm.shape[1:], _vec(stride, dim), box)
  out = np.empty_like(cm)
  for c in range(dim):
    out[c] = (cm[c].astype(np.float64) + sign * offs[c]).astype(cm.dtype)
  return out


def to_absolute(coord_map, stride, box=None):
  return _shift(coord_map, stride, box, 1.0)


def to_relative(coord_map, stride, box=None):
  return _shift(coord_map, stride, box, -1.0)


def outer_extents(coord_map, stride, box):
  """[(nanmin, nanmax)] per channel of the absolute map, in the map's dtype
  (NaN, NaN for an all-NaN channel)."""
  ab = to_absolute(coord_map, stride, box)
  out = []
  for c in ab:
    ok = ~np.isnan(c)
    out.append((c[ok].min(), c[ok].max()) if ok.any() else
               (ab.dtype.type(np.nan),) * 2)
  return out


def outer_box(coord_map, box, stride, target_len=None):
  dim = np.shape(coord_map)[0]
  tl_xyz = _vec(target_len if target_len is not None else stride, dim)[::-1]
  start = np.array(box.start).copy()
  size = np.array(box.size).copy()
  for i, ((lo, hi), tl) in enumerate(zip(outer_extents(coord_map, stride, box), tl_xyz)):
    lo = int(lo) // tl
    start[i] = lo
    size[i] = -(int(-hi) // tl) - lo + 1
  return Box(start, size)


def inner_extents(coord_map, stride, box):
  """Per axis x, y[, z]: (max of the line minima, min of the line maxima) of that
  axis' channel along that axis."""
  ab = to_absolute(coord_map, stride, box)
  return [(ab[c].min(axis=-1 - c).max(), ab[c].max(axis=-1 - c).min())
          for c in range(ab.shape[0])]


def inner_box(coord_map, box, stride):
  cm = np.asarray(coord_map)
  dim = cm.shape[0]
  if np.isnan(cm).any():
    raise NotImplementedError('inner_box needs fill_missing for maps with NaN')
  stride = _vec(stride, dim)
  ext = inner_extents(cm, stride, box)
  lo = [int(-(-ext[c][0] // stride[dim - 1 - c])) for c in range(dim)]
  hi = [ext[c][1] // stride[dim - 1 - c] for c in range(dim)]
  if dim == 2:
    return Box((lo[0], lo[1], box.start[2]),
               (hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, box.size[2]))
  return Box(tuple(lo), tuple(h - l + 1 for h, l in zip(hi, lo)))


def affine_positions(box, stride):
  """[3, z, y, x] float64 node positions, channels x, y, z."""
  stride = _vec(stride, 3)
  shape = tuple(int(v) for v in np.asarray(box.size)[::-1])
  pos = np.empty((3,) + shape)
  for c in range(3):
    axis = 2 - c
    view = [1, 1, 1]
    view[axis] = -1
    p = np.arange(shape[axis], dtype=np.float64) * np.float64(stride[axis]) + np.float64(
        box.start[c])
    pos[c] = p.reshape(view)
  return pos


def make_affine_map(matrix, box, stride):
  m = np.asarray(matrix, np.float64)
  p = affine_positions(box, stride)
  out = np.empty_like(p)
  for c in range(3):
    out[c] = (((m[c, 0] * p[0] + m[c, 1] * p[1]) + m[c, 2] * p[2]) + m[c, 3]) - p[c]
  return out


def affine_bound(matrix, box, stride):
  """8 eps64 (sum_j |a_ij| |x_j| + |t_i| + |x_i|): forward bound of a three-term
  float64 dot product plus two additions, with margin."""
  m = np.abs(np.asarray(matrix, np.float64))
  p = np.abs(affine_positions(box, stride))
  return np.stack([8 * np.finfo(np.float64).eps *
                   (m[c, 0] * p[0] + m[c, 1] * p[1] + m[c, 2] * p[2] + m[c, 3] + p[c])
                   for c in range(3)])


def section_index(z, start_z, nz):
  """int(z - start) indexed like NumPy; IndexError outside [-nz, nz)."""
  z_rel = int(z - start_z)
  if not -nz <= z_rel < nz:
    raise IndexError(f'index {z_rel} is out of bounds for axis 1 with size {nz}')
  return z_rel % nz


def warp_points_f32(points, coord_map, map_box, stride):
  """(x, y) float32 [n, 2] before the integer rounding: the four-term bilinear
  combination in float64 of the twice-rounded absolute nodes."""
  pts = np.asarray(points)
  cm = np.asarray(coord_map)
  assert cm.shape[0] == 2
  nz, ny, nx = cm.shape[1:]
  if ny < 2 or nx < 2:
    raise ValueError('the grid needs at least 2 nodes along y and x')
  ab = to_absolute(cm, stride)
  org = np.asarray(map_box.start)[:2] * np.float64(stride)
  for c in range(2):
    ab[c] = (ab[c].astype(np.float64) + org[c]).astype(cm.dtype)
  gx = (np.arange(nx) + int(map_box.start[0])).astype(np.float64) * np.float64(stride)
  gy = (np.arange(ny) + int(map_box.start[1])).astype(np.float64) * np.float64(stride)
  zi = np.array([section_index(z, map_box.start[2], nz) for z in pts[:, 2]], dtype=np.int64)
  qx = pts[:, 0].astype(np.float64)
  qy = pts[:, 1].astype(np.float64)

  def cell(g, q):
    i = np.clip(np.searchsorted(g, q, side='right') - 1, 0, len(g) - 2)
    return i, (q - g[i]) / (g[i + 1] - g[i])

  ix, tx = cell(gx, qx)
  iy, ty = cell(gy, qy)
  out = np.empty((len(pts), 2), np.float32)
  for c in range(2):
    v = ab[c].astype(np.float64)
    val = (v[zi, iy, ix] * ((1 - ty) * (1 - tx)) + v[zi, iy, ix + 1] * ((1 - ty) * tx) +
           v[zi, iy + 1, ix] * (ty * (1 - tx)) + v[zi, iy + 1, ix + 1] * (ty * tx))
    out[:, c] = val.astype(np.float32)
  return out


def warp_points(points, coord_map, map_box, stride):
  pts = np.array(points)
  ret = pts.copy()
  if len(pts) == 0:
    if np.shape(coord_map)[2] < 2 or np.shape(coord_map)[3] < 2:
      raise ValueError('the grid needs at least 2 nodes along y and x')
    return ret
  xy = warp_points_f32(pts, coord_map, map_box, stride)
  if np.issubdtype(ret.dtype, np.integer):
    xy = np.round(xy)
  ret[:, :2] = xy.astype(ret.dtype)
  return ret


def ulp_distance_f32(a, b):
  """Distance in float32 ulps; 0 where both are NaN."""
  a = np.asarray(a, np.float32)
  b = np.asarray(b, np.float32)

  def key(v):
    i = v.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)

  d = np.abs(key(a) - key(b))
  both_nan = np.isnan(a) & np.isnan(b)
  one_nan = np.isnan(a) ^ np.isnan(b)
  return np.where(both_nan, 0, np.where(one_nan, np.iinfo(np.int64).max, d))


def check_points_float(got, want):
  """The cap on float results: equal after narrowing on >= 99.99 % of the
  coordinates, at most 1 float32 ulp on the rest.  Returns the unequal count."""
  got = np.asarray(got)
  want = np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape
  assert np.array_equal(got[:, 2], want[:, 2], equal_nan=True)
  d = ulp_distance_f32(got[:, :2].astype(np.float32), want[:, :2].astype(np.float32))
  assert d.max(initial=0) <= 1, f'{d.max()} ulp'
  n_off = int((d > 0).sum())
  assert n_off <= 1e-4 * d.size, f'{n_off} of {d.size} coordinates differ'
  return n_off


def check_points_int(got, want, ref_f32):
  """Integer results: exact, except where the float32 value lies within 1 ulp of a
  .5 tie (at most 0.01 % of the coordinates).  Returns the excluded count."""
  got = np.asarray(got)
  want = np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape
  assert np.array_equal(got[:, 2], want[:, 2])
  f = np.asarray(ref_f32, np.float32)
  tie = np.floor(f) + np.float32(0.5)
  near = ulp_distance_f32(f, tie) <= 1
  assert near.sum() <= 1e-4 * near.size
  assert np.array_equal(got[:, :2][~near], want[:, :2][~near])
  assert np.all(np.abs(got[:, :2][near].astype(np.int64) - want[:, :2][near]) <= 1)
  return int(near.sum())


# -- tests/golden/mapgeom.npz ---------------------------------------------------
def py_scalar(v):
  """A stored stride as the caller's Python number: int when integral (the box
  expressions floor-divide by it), else float."""
  v = float(v)
  return int(v) if v == int(v) else v


def py_stride(values):
  vals = [py_scalar(v) for v in np.asarray(values).ravel()]
  return vals[0] if len(set(vals)) == 1 else tuple(vals)


def load_golden():
  """{'geo': [...], 'aff': [...], 'pts': [...]}: one dict of arrays per case."""
  import os
  g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                           'mapgeom.npz'))
  out = {'geo': {}, 'aff': {}, 'pts': {}}
  for key in g.files:
    kind, idx, field = key[:3], int(key[3:5]), key[6:]
    out[kind].setdefault(idx, {})[field] = g[key]
  res = {}
  for kind, cases in out.items():
    res[kind] = [cases[i] for i in sorted(cases)]
    for rec in res[kind]:
      rec['name'] = str(rec['name'])
  return res


def geo_box(rec):
  return Box(rec['start'], rec['size']) if int(rec['hasbox']) else None
