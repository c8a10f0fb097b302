"""NumPy restatement of scipy.ndimage.map_coordinates for spline orders 2 to 5,
mode "constant", cval 0, in plain float64 arithmetic and in SciPy's operation
order: the B-spline prefilter (`prefilter`, what `scipy.ndimage.spline_filter(
image, order, output=float64, mode='constant')` computes) and the sampler
(`sample`, NI_GeometricTransform).  tests/test_ndwarp_spline_ref.py pins both to
SciPy element for element; the device kernels (sfm_spline.hip, spline_sample of
sfm_ndsample.h) are written from this file, and the GPU tests compare with it
where SciPy is not the reference.

`ndimage_warp` is warp.ndimage_warp (warp.py:189-335) with one work box: the
dense coordinates by SciPy's order-1 map_coordinates (as the oracle forms them),
the image by `map_coordinates` of this file.
"""
import math

import numpy as np

# SciPy's literals (ni_splines.c: get_filter_poles); sqrt(3) - 2 and its kin
# differ in the last bits
POLES = {
    2: (-0.171572875253809902396622551580603843,),
    3: (-0.267949192431122706472553658494127633,),
    4: (-0.361341225900220177092212841325675255, -0.013725429297339121360331226939128204),
    5: (-0.430575347099973791851434783493520110, -0.043096288203264653822712376822550182),
}


def gain(order):
  g = 1.0
  for z in POLES[order]:
    g *= (1.0 - z) * (1.0 - 1.0 / z)
  return g


def zn_table(order, shape):
  """[3, 2] pow(pole, len - 1) per axis (z, y, x; a 2-D shape is padded in
  front) and pole, with the host's libm: what the device is handed."""
  shape = (1,) * (3 - len(shape)) + tuple(int(v) for v in shape)
  out = np.zeros((3, 2), np.float64)
  for k, n in enumerate(shape):
    for p, z in enumerate(POLES[order]):
      out[k, p] = math.pow(z, n - 1)
  return out


def filter_axis(c, axis, order):
  """One spline_filter1d pass over `axis` of the float64 array `c`, in place,
  mirror boundaries, every line at once (the recursion runs along the axis)."""
  c = np.moveaxis(c, axis, 0)
  n = c.shape[0]
  if n == 1:
    return
  c *= gain(order)
  for z in POLES[order]:
    zn = math.pow(z, n - 1)
    zi = z
    c[0] = c[0] + zn * c[n - 1]
    for i in range(1, n - 1):
      c[0] += zi * (c[i] + zn * c[n - 1 - i])
      zi *= z
    c[0] /= 1.0 - zn * zn
    for i in range(1, n):
      c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
      c[i] = z * (c[i + 1] - c[i])


def prefilter(image, order):
  """float64 B-spline coefficients of `image`: axis 0 first, each pass on the
  previous pass's output."""
  c = np.array(image, dtype=np.float64, copy=True, order='C')
  with np.errstate(all='ignore'):
    for axis in range(c.ndim):
      filter_axis(c, axis, order)
  return c


def weights(order, x):
  """The order + 1 tap weights at offset `x` from the base sample, in tap order."""
  if order == 2:
    w1 = 0.75 - x * x
    y = 0.5 - x
    w0 = 0.5 * y * y
    return [w0, w1, 1.0 - w0 - w1]
  if order == 3:
    y, z = x, 1.0 - x
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0
    w0 = z * z * z / 6.0
    return [w0, w1, w2, 1.0 - w0 - w1 - w2]
  if order == 4:
    t = x * x
    w2 = t * (t * 0.25 - 0.625) + 115.0 / 192.0
    y = 1.0 + x
    w1 = y * (y * (y * (5.0 - y) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0
    z = 1.0 - x
    w3 = z * (z * (z * (5.0 - z) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0
    y = 0.5 - x
    y = y * y
    w0 = y * y / 24.0
    return [w0, w1, w2, w3, 1.0 - w0 - w1 - w2 - w3]
  assert order == 5
  y, z = x, 1.0 - x
  t = y * y
  w2 = t * (t * (0.25 - y / 12.0) - 0.5) + 0.55
  t = z * z
  w3 = t * (t * (0.25 - z / 12.0) - 0.5) + 0.55
  y1 = y + 1.0
  w1 = y1 * (y1 * (y1 * (y1 * (y1 / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425
  z1 = z + 1.0
  w4 = z1 * (z1 * (z1 * (z1 * (z1 / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425
  t = 1.0 - x
  t2 = t * t
  w0 = t * t2 * t2 / 120.0
  return [w0, w1, w2, w3, w4, 1.0 - w0 - w1 - w2 - w3 - w4]


def sample(coeffs, coords, order):
  """float64 value of the spline with coefficients `coeffs` at `coords` ([ndim,
  ...]): 0 outside [0, len - 1] on any axis (NaN included), taps mirrored without
  repeating the edge sample, summed in row-major order."""
  coeffs = np.asarray(coeffs, np.float64)
  coords = np.asarray(coords, np.float64)
  dim = coeffs.ndim
  out_shape = coords.shape[1:]
  cc = coords.reshape(dim, -1)
  k = order + 1
  inside = np.ones(cc.shape[1], bool)
  ws, idx = [], []
  with np.errstate(all='ignore'):
    for d in range(dim):
      n = coeffs.shape[d]
      ok = (cc[d] >= 0.0) & (cc[d] <= float(n - 1))
      inside &= ok
      c = np.where(ok, cc[d], 0.0)
      base = np.floor(c) if order & 1 else np.floor(c + 0.5)
      ws.append(weights(order, c - base))
      start = base.astype(np.int64) - order // 2
      taps = []
      for j in range(k):
        i = np.abs(start + j)
        if n == 1:
          i = np.zeros_like(i)
        else:
          i = i % (2 * n - 2)
          i = np.where(i >= n, 2 * n - 2 - i, i)
        taps.append(i)
      idx.append(taps)
    acc = np.zeros(cc.shape[1], np.float64)
    for tap in np.ndindex(*(k,) * dim):
      v = coeffs[tuple(idx[d][tap[d]] for d in range(dim))]
      for d in range(dim):
        v = v * ws[d][tap[d]]
      acc = acc + v
  return np.where(inside, acc, 0.0).reshape(out_shape)


def convert(v, dtype):
  """double -> output dtype like NI's CASE_INTERP_OUT_*."""
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    with np.errstate(all='ignore'):
      return v.astype(dtype)
  vmax = float(np.iinfo(dtype).max)
  with np.errstate(all='ignore'):
    v = np.where(v > 0.0, v + 0.5, 0.0)
    v = np.where(v > vmax, vmax, v)
  return v.astype(dtype)


def map_coordinates(image, coords, order):
  """scipy.ndimage.map_coordinates(image, coords, order=order) for order 2 .. 5."""
  image = np.asarray(image)
  return convert(sample(prefilter(image, order), coords, order), image.dtype)


def ndimage_warp(image, coord_map, stride, order, image_start=None, map_start=None,
                 out_start=None, out_size=None, scipy_sampler=False):
  """warp.ndimage_warp with one work box (the reference prefilters the whole image
  for every work box, so the decomposition does not change the result); boxes are
  xyz start / size vectors, out_scale is 1.  The map keeps its dtype, as in the
  reference (oracle.warp_oracle.ndimage_warp computes float32 maps only).  With
  `scipy_sampler` the image is sampled by SciPy itself: map_coordinates twice."""
  from scipy import ndimage
  image = np.asarray(image)
  coord_map = np.asarray(coord_map)
  dim = coord_map.shape[0]
  shape = coord_map.shape[1:]
  src = np.array(coord_map, copy=True)
  grid = np.mgrid[tuple(slice(0, s) for s in shape)]
  off_zyx = [h * st for h, st in zip(grid, stride)]
  for i in range(dim):
    src[i, ...] += off_zyx[-(i + 1)]
  if map_start is not None:
    src += (np.asarray(map_start)[:dim] * np.asarray(stride)[::-1] -
            np.asarray(image_start)[:dim] / np.ones(dim)).reshape((dim,) + (1,) * dim)
  src = src.copy() * np.ones(dim)[(slice(None),) + (np.newaxis,) * dim]
  if out_size is not None:
    out_shape = tuple(int(v) for v in np.asarray(out_size)[::-1][-dim:])
    out_start = np.asarray(out_start)
  else:
    out_shape = image.shape
    out_start = np.zeros(3, np.int64)
  if map_start is not None:
    offset = (np.asarray(map_start) * np.asarray(stride)[::-1] - out_start)[::-1]
  else:
    offset = (0, 0, 0)
  pos = np.mgrid[tuple(slice(0, s) for s in out_shape)]
  pos = [(c - o) / s for c, s, o in zip(pos, stride, offset)]
  dense = [ndimage.map_coordinates(ev, pos, order=1) for ev in src[::-1]]
  if scipy_sampler:
    return ndimage.map_coordinates(image, dense, order=order).astype(image.dtype)
  return map_coordinates(image, np.array(dense), order)


# -- test inputs shared by the CPU and GPU tests ---------------------------------------
EDGE_SHAPES = ((2, 2), (3, 3), (1, 9), (9, 1), (5, 65), (3, 130), (70, 5), (3, 5, 70),
               (66, 3, 4), (2, 1, 7))


def edge_image(rng, shape, dtype):
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    return rng.uniform(-50.0, 300.0, shape).astype(dtype)
  return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def edge_coords(rng, shape, order, n_random=160):
  """[ndim, n] coordinates: per axis exact 0, len - 1, len - 1 + 1e-9, -1e-9, every
  integer and half-integer of the axis (the even-order floor(cc + 0.5) branch), NaN,
  points more than `order` outside, combined with random positions on the other
  axes, and random points over the array and a rim of order + 2 around it."""
  dim = len(shape)
  cols = []
  for d, n in enumerate(shape):
    special = np.concatenate([
        [0.0, n - 1.0, n - 1.0 + 1e-9, -1e-9, np.nan, -(order + 1.5), n + order + 0.5],
        np.arange(n, dtype=np.float64)[:12], np.arange(n, dtype=np.float64)[-12:],
        np.arange(0.5, n - 1, 1.0)[:12], np.arange(0.5, n - 1, 1.0)[-12:]])
    for rep in range(2):
      c = np.stack([rng.uniform(0, s - 1, special.size) if rep else
                    rng.integers(0, s, special.size).astype(np.float64) for s in shape])
      c[d] = special
      cols.append(c)
  lo = -(order + 2.0)
  cols.append(np.stack([rng.uniform(lo, s - 1 - lo, n_random) for s in shape]))
  cols.append(np.stack([rng.uniform(0, s - 1, n_random) for s in shape]))
  # all axes on an edge or an integer at once
  cols.append(np.stack([rng.integers(0, s, n_random).astype(np.float64) for s in shape]))
  return np.concatenate(cols, axis=1).reshape(dim, -1)


# -- tests/golden/ndimage_warp_spline.npz ----------------------------------------------
def image_of(base, dtype):
  """The image of a dtype from a stored uint8 one (as make_golden_ndwarp_spline.py
  forms it)."""
  dtype = np.dtype(dtype)
  if dtype == np.uint8:
    return base
  if dtype == np.uint16:
    return base.astype(np.uint16) * np.uint16(257)
  assert dtype == np.float32
  return base.astype(np.float32) / np.float32(3) - np.float32(20)


def warp_cases(g):
  """The ndimage_warp cases of the fixture: dicts with name, image, map, stride,
  work, overlap, order, boxes ({image, map, out: (start, size)} or None), warped."""
  out = []
  for name in g['names']:
    name = str(name)
    image = image_of(g[str(g[f'{name}_base'])], str(g[f'{name}_dtype']))
    stride = g[f'{name}_stride']
    stride = tuple(int(v) if g[f'{name}_stride_is_int'] else float(v) for v in stride)
    boxes = None
    if f'{name}_image_box' in g.files:
      boxes = {k: tuple(g[f'{name}_{k}_box']) for k in ('image', 'map', 'out')}
    out.append(dict(name=name, image=image, map=g['map2' if image.ndim == 2 else 'map3'],
                    stride=stride, work=tuple(int(v) for v in g[f'{name}_work']),
                    overlap=tuple(int(v) for v in g[f'{name}_overlap']),
                    order=int(g[f'{name}_order']), boxes=boxes, warped=g[f'{name}_warped']))
  return out


def render_cases(g, scenes):
  """The render section: [(scene of render3d.npz, order, [(request name, box, plan,
  out)])]; `scenes` is render3d_ref.scenes(render3d.npz), whose tiles, maps,
  weights, boxes and plans the spline scenes share."""
  out = []
  n = 0
  while f'r{n:02d}_base' in g.files:
    sc = scenes[int(g[f'r{n:02d}_base'])]
    reqs = [(name, b, plan, g[f'r{n:02d}_q{r:02d}_out'])
            for r, (name, b, plan, _) in enumerate(sc['requests'])
            if f'r{n:02d}_q{r:02d}_out' in g.files]
    out.append((sc, int(g[f'r{n:02d}_order']), reqs))
    n += 1
  return out


def render(out_box, tiles, plan, inverted, weights, stride, order, out_dtype=None):
  """tests/render3d_ref.render with the image sampled by `map_coordinates` of this
  file: per work item the data_box CROP is prefiltered, as the reference does.
  Orders 0 and 1 have no coefficients to restate: they are render3d_ref.render itself."""
  from scipy import ndimage
  from tests import render3d_ref
  if order < 2:
    return render3d_ref.render(out_box, tiles, plan, inverted, weights, stride, order, out_dtype)
  if out_dtype is None:
    out_dtype = np.asarray(next(iter(tiles.values()))).dtype
  pairs = []
  for item in plan:
    i, data_box, tg_box, local_warp_box, _ = item
    dense = render3d_ref.dense_coords(inverted[i][1], stride, tg_box, data_box, local_warp_box)
    crop = np.asarray(tiles[i])[render3d_ref._slices(data_box.start, data_box.size)]
    w = np.asarray(weights[i])[render3d_ref._slices(data_box.start[:2], data_box.size[:2])]
    w = np.repeat(w[None, ...], int(data_box.size[2]), axis=0)
    pairs.append((map_coordinates(crop, np.array(dense), order),
                  ndimage.map_coordinates(w, dense, order=1).astype(w.dtype)))
  return render3d_ref.blend(out_box, plan, pairs, out_dtype)
