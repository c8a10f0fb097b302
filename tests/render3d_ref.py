"""NumPy / SciPy restatement of the render loop of the reference's
`processor/warp.py: StitchAndRender3dTiles.process` (:292-343), and the readers
of tests/golden/render3d.npz.

`render` is what the reference computes for one output box from the work items
of `_load_tile_images`: per tile `warp.ndimage_warp` of the image region and of
the blending weights (scipy.ndimage.map_coordinates, warp.py:249-314), the
float32 weighted sums in ascending tile index, the normalisation and the cast.
tests/test_render3d_host.py pins it bit for bit to the reference's own output;
the GPU tests use it where the reference does not exist.
"""
import types

import numpy as np
from scipy import ndimage

REQUESTS = ('canvas', 'cut67', 'inside', 'corner', 'nothing', 'voxel')


def box(start, size):
  return types.SimpleNamespace(start=np.array(start, np.int64), size=np.array(size, np.int64))


def _slices(start_xyz, size_xyz):
  return tuple(slice(int(a), int(a + n)) for a, n in zip(start_xyz[::-1], size_xyz[::-1]))


def dense_coords(inverted_map, stride, tg_box, data_box, local_warp_box):
  """The z, y, x source coordinates of every voxel of local_warp_box in the frame
  of data_box (warp.py:249-311)."""
  stride = tuple(stride)
  src = np.array(inverted_map, dtype=np.float64, copy=True)
  idx = np.mgrid[tuple(slice(0, s) for s in src.shape[1:])]
  off_zyx = [h * st for h, st in zip(idx, stride)]
  for c in range(3):
    src[c, ...] += off_zyx[-(c + 1)]
  src += (tg_box.start[:3] * stride[::-1] - data_box.start[:3] / (1.0, 1.0, 1.0)
          ).reshape(3, 1, 1, 1)
  src = src.copy() * np.array((1.0, 1.0, 1.0))[:, None, None, None]
  offset = (tg_box.start * stride[::-1] - local_warp_box.start)[::-1]
  coords = np.mgrid[tuple(slice(0, int(s)) for s in local_warp_box.size[::-1])]
  coords = [(c - o) / s for c, s, o in zip(coords, stride, offset)]
  return [ndimage.map_coordinates(ev, coords, order=1) for ev in src[::-1]]


def warped_pair(tile, weights, inverted_map, stride, item, order):
  """(warped image, warped weights) of one work item: the two ndimage_warp calls
  of :308-331."""
  _, data_box, tg_box, local_warp_box, _ = item
  dense = dense_coords(inverted_map, stride, tg_box, data_box, local_warp_box)
  image = np.asarray(tile)[_slices(data_box.start, data_box.size)]
  sub_dts = np.asarray(weights)[_slices(data_box.start[:2], data_box.size[:2])][None, ...]
  sub_dts = np.repeat(sub_dts, int(data_box.size[2]), axis=0)
  warped = ndimage.map_coordinates(image, dense, order=order).astype(image.dtype)
  warped_dts = ndimage.map_coordinates(sub_dts, dense, order=1).astype(sub_dts.dtype)
  return warped, warped_dts


def blend(out_box, plan, pairs, out_dtype):
  """:292-293, :333-343 from the per-tile (image, weights) pairs, in plan order."""
  shape = tuple(int(v) for v in out_box.size[::-1])
  img = np.zeros(shape, np.float32)
  norm = np.zeros(shape, np.float32)
  for item, (image, warped_dts) in zip(plan, pairs):
    sub_box = item[4]
    sl = _slices(sub_box.start - out_box.start, sub_box.size)
    img[sl] += image * warped_dts
    norm[sl] += warped_dts
  ret = img
  ret[norm > 0] /= norm[norm > 0]
  return ret.astype(out_dtype)


def render(out_box, tiles, plan, inverted, weights, stride, order=1, out_dtype=None):
  if out_dtype is None:
    out_dtype = np.asarray(next(iter(tiles.values()))).dtype
  pairs = [warped_pair(tiles[item[0]], weights[item[0]], inverted[item[0]][1], stride, item,
                       order) for item in plan]
  return blend(out_box, plan, pairs, out_dtype)


def outer_box_np(coord_map, b, stride, target_len=None):
  """map_utils.outer_box (map_utils.py:307-342) in NumPy, for 3-channel maps."""
  stride = tuple(stride)
  ab = np.array(coord_map, copy=True)
  idx = np.mgrid[tuple(slice(0, s) for s in ab.shape[1:])]
  for c in range(3):
    ab[c] += (idx[2 - c] + b.start[c]) * stride[2 - c]
  tl_xyz = (tuple(stride) if target_len is None else (target_len,) * 3
            if np.isscalar(target_len) else tuple(target_len))[::-1]
  start, size = b.start.copy(), b.size.copy()
  for i, tl in enumerate(tl_xyz):
    x_min, x_max = np.nanmin(ab[i]), np.nanmax(ab[i])
    x_min = int(x_min) // tl
    start[i] = x_min
    size[i] = -(int(-x_max) // tl) - x_min + 1
  return box(start, size)


# -- tests/golden/render3d.npz -----------------------------------------------------
def tiles_of(base, dtype):
  """The tiles of a dtype from the stored uint8 ones (as make_golden_render3d.py
  forms them)."""
  dtype = np.dtype(dtype)
  if dtype == np.uint8:
    return base
  if dtype == np.uint16:
    t = base.astype(np.uint16) * np.uint16(3) + np.uint16(1000)
    t[1, 0, 0, :4] = (0, 65535, 1, 65534)
    return t
  assert dtype == np.float32
  return base.astype(np.float32) * np.float32(0.25) - np.float32(7.5)


def _plan(rows):
  return [(int(r[0, 0]),) + tuple(box(r[k], r[k + 1]) for k in (1, 3, 5, 7)) for r in rows]


def scenes(g):
  """The scenes of the fixture: dicts with dtype, order, margin, offset, stride,
  tiles {i: array}, meshes, tile_idx_to_xy, boxes {i: (out_box, tg_box)},
  inverted {i: (tg_box, map)}, weights {i: array} and requests
  [(name, box, plan, out)]."""
  base = g['tiles_uint8']
  n = base.shape[0]
  xy = {i: tuple(int(v) for v in g['key_xy'][i]) for i in range(n)}
  inverted = {i: (box(*g[f'inv_box_{i}']), g[f'inv_{i}']) for i in range(n)}
  out = []
  s = 0
  while f's{s:02d}_dtype' in g.files:
    p = f's{s:02d}_'
    dtype = np.dtype(str(g[p + 'dtype']))
    t = tiles_of(base, dtype)
    b = g[p + 'boxes']
    reqs = []
    for r, name in enumerate(REQUESTS):
      q = f'{p}r{r:02d}_'
      reqs.append((name, box(*g[q + 'box']), _plan(g[q + 'plan']), g[q + 'out']))
    out.append(dict(
        name=f's{s:02d}', dtype=dtype, order=int(g[p + 'order']), margin=int(g[p + 'margin']),
        offset=tuple(int(v) for v in g[p + 'offset']),
        stride=tuple(int(v) for v in g[p + 'stride']),
        tiles={i: t[i] for i in range(n)}, meshes=g['meshes'], tile_idx_to_xy=xy,
        boxes={i: (box(b[i, 0], b[i, 1]), box(b[i, 2], b[i, 3])) for i in range(n)},
        inverted=inverted, weights={i: g[f'{p}w_{i}'] for i in range(n)}, requests=reqs))
    s += 1
  return out


def same_plan(got, want):
  """Work items equal in tile index and in every box."""
  if len(got) != len(want):
    return False
  for a, b in zip(got, want):
    if a[0] != b[0]:
      return False
    for x, y in zip(a[1:], b[1:]):
      if not (np.array_equal(np.asarray(x.start), y.start) and
              np.array_equal(np.asarray(x.size), y.size)):
        return False
  return True
