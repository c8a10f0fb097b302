"""Warp-and-blend rendering of 3-D tile montages on the device.

Drop-in for the compute part of `processor/warp.py: StitchAndRender3dTiles`
(processor/warp.py:112-345): the step that turns the solved tile meshes of a
volumetric montage into voxels.  The reference renders an output box tile by
tile -- `warp.ndimage_warp` of the image, `warp.ndimage_warp` of the blending
weights, a float32 weighted sum in NumPy -- and normalises at the end.  Here an
output box is ONE kernel (`sfm_render_tiles3d`): every output voxel walks the
tiles that reach it in ascending tile index, computes the dense source
coordinates once per tile, samples image and weights, accumulates in registers
and stores the normalised, cast value once.  The operations are the
reference's, in its order and precision, so the rendered volume is the
reference's bit for bit (tests/golden/render3d.npz).

  tile_boxes     <->  _collect_tile_boxes  (:112-145)
  blend_weights  <->  _get_dts             (:147-161)
  plan_render    <->  _load_tile_images    (:183-241), the box arithmetic
  render         <->  process              (:292-343)
  fill_inverted  <->  the fill_missing call of _load_tile_images (:199-203)

Array level, no volume stores.  Boxes are objects with `.start` / `.size` in
xyz or (start, size) pairs; the boxes returned are `Box` tuples, which are both.
The per-tile inverse maps (the reference's 3-D `invert_map`, :195-198) are
inputs: they are mesh sized, computed once per tile, and depend on 3-D Qhull.
`plan_render`, `render` and `TileRenderer` take them without NaN, i.e. after the
nearest-only `fill_missing` of :199-203, which `fill_inverted` runs on the
device.

Kept from the reference: a voxel no tile reaches is 0; a NaN or out-of-range
dense coordinate samples 0 for image and weight; with `margin > 0` a tile on the
outer side of the grid loses its last column / row (the `-1` slice end of
:153-155); the truncating cast after `(v * w) / w` can give `v - 1`.  Different:
the reference adds tiles in `as_completed` order, which is unspecified; this
code adds them in ascending tile index.  Spline orders 2 to 5 of the image
(opt-in: the switch SFM_SPLINE_ORDERS=1, `_abi.set_option`; without it they raise
NotImplementedError as before): the
reference warps each tile's `data_box` CROP, so per `render` call the crops of
all plan items are prefiltered into one float64 workspace (one batch of
launches over the plan table, mirrored at the crops' edges) and the fused kernel
samples those coefficients; orders 0 and 1 read the tiles in place.  The weights
are always sampled with order 1.  Not built: uint64 label tiles, `out_scale`
other than 1 (NotImplementedError).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Sequence

import numpy as np
import torch

from . import _abi
from . import _dev
from . import _spline
from . import map_utils
from ._dev import DeviceArray


class Box(NamedTuple):
  """xyz box; a (start, size) pair that also has `.start` / `.size` / `.end`."""
  start: np.ndarray
  size: np.ndarray

  @property
  def end(self) -> np.ndarray:
    return self.start + self.size


def _as_box(box) -> Box:
  start, size = map_utils._box(box)
  return Box(np.array(start, dtype=np.int64), np.array(size, dtype=np.int64))


def _intersection(a: Box, b: Box) -> Box | None:
  start = np.maximum(a.start, b.start)
  end = np.minimum(a.end, b.end)
  if np.any(end <= start):
    return None
  return Box(start, end - start)


def _array(x):
  """NumPy arrays and torch tensors as they are (both slice alike)."""
  return x.tensor if isinstance(x, DeviceArray) else x


def tile_boxes(tile_meshes, tile_idx_to_xy, tile_shape_zyx: Sequence[int],
               stride: Sequence[float], offset: Sequence[int] = (0, 0, 0)
               ) -> dict[int, tuple[Box, Box]]:
  """{i: (out_box, tg_box)} of every tile (processor/warp.py:112-145).

  tile_meshes: [3, n_tiles, z, y, x] solved meshes in relative format (NumPy,
  torch or DeviceArray); tile_idx_to_xy: {i: (tx, ty)} grid positions;
  tile_shape_zyx: shape of a tile; stride: zyx mesh stride; offset: xyz global
  offset of the rendered image.  tg_box is `map_utils.outer_box` of the tile's
  mesh in node units, out_box the region the tile can render in global
  coordinates.
  """
  meshes = _array(tile_meshes)
  map_box = Box(np.zeros(3, np.int64), np.array(tuple(meshes.shape[2:])[::-1], np.int64))
  ret = {}
  for i in range(meshes.shape[1]):
    tx, ty = tile_idx_to_xy[i]
    tg_box = _as_box(map_utils.outer_box(meshes[:, i, ...], map_box, stride))
    out_box = Box(
        np.array((tg_box.start[0] * stride[2] + tx * tile_shape_zyx[-1] + offset[0],
                  tg_box.start[1] * stride[1] + ty * tile_shape_zyx[-2] + offset[1],
                  tg_box.start[2] * stride[0] + offset[2]), np.int64),
        np.array((tg_box.size[0] * stride[2], tg_box.size[1] * stride[1],
                  tg_box.size[2] * stride[0]), np.int64))
    ret[i] = out_box, tg_box
  return ret


def blend_weights(tile_shape_zyx: Sequence[int], tx: int, ty: int,
                  grid_shape_yx: Sequence[int], margin: int, device: bool = False):
  """[y, x] float32 blending weights of the tile at (tx, ty) (processor/warp.py:147-161).

  The reference masks the tile except `margin` pixels at the sides that face
  another tile and takes the Euclidean distance transform with a black border
  (`edt.edt(mask, black_border=True)`).  The mask is one rectangle, so the
  nearest background pixel of a pixel inside lies straight across one of the
  four sides: the transform is max(0, min(x - x0 + 1, x1 - x, y - y0 + 1,
  y1 - y)) with exclusive ends x1, y1.  With `margin > 0` a side on the outer
  edge of the grid ends at -1 like the reference's slice, i.e. the last column /
  row is outside the mask.  `device=True` returns a DeviceArray.
  """
  ny, nx = (int(v) for v in tile_shape_zyx[1:])
  if margin > 0:
    x0 = margin if tx > 0 else 0
    x1 = -margin if tx < grid_shape_yx[-1] - 1 else -1
    y0 = margin if ty > 0 else 0
    y1 = -margin if ty < grid_shape_yx[-2] - 1 else -1
    x0, x1 = min(x0, nx), max(nx + x1, 0)     # what the slice x0:x1 selects
    y0, y1 = min(y0, ny), max(ny + y1, 0)
  else:
    x0, x1, y0, y1 = 0, nx, 0, ny
  x = np.arange(nx, dtype=np.int64)[None, :]
  y = np.arange(ny, dtype=np.int64)[:, None]
  dist = np.minimum(np.minimum(x - x0 + 1, x1 - x), np.minimum(y - y0 + 1, y1 - y))
  w = np.maximum(dist, 0).astype(np.float32)
  if device:
    return DeviceArray(_dev.upload(np.ascontiguousarray(w), _dev.device()))
  return w


def plan_render(box, boxes, inverted, tile_idx_to_xy, tile_shape_zyx: Sequence[int],
                stride: Sequence[float], offset: Sequence[int] = (0, 0, 0)
                ) -> list[tuple[int, Box, Box, Box, Box]]:
  """Per-tile work items of one output box, in ascending tile index:
  (i, data_box, tg_box, local_warp_box, sub_box) (processor/warp.py:183-241).

  box: the output box in global coordinates; boxes: the result of `tile_boxes`;
  inverted: {i: (tg_box, inverted_map)} with tg_box ALREADY widened by one node
  on every side (:195) and the map [3, z, y, x] float64 without NaN (NumPy,
  torch or DeviceArray).  A tile is skipped like in the reference: no
  intersection with `box`, no map node near it, no image data under it.
  sub_box is the part of `box` the tile renders, local_warp_box the same region
  in the tile's frame, data_box the part of the tile image the region can
  sample (`map_utils.outer_box` of the map nodes around it, on the device).
  `BoundingBox.scale` is taken as floor of start * s and ceil of end * s.
  """
  box = _as_box(box)
  image_box = Box(np.zeros(3, np.int64), np.array(tuple(tile_shape_zyx)[::-1], np.int64))
  plan = []
  for i in sorted(boxes):
    out_box = _as_box(boxes[i][0])
    sub_box = _intersection(out_box, box)
    if sub_box is None or i not in inverted:
      continue
    tx, ty = tile_idx_to_xy[i]
    tg_box = _as_box(inverted[i][0])
    inverted_map = _array(inverted[i][1])
    local_out_start = out_box.start - np.array(
        (tx * tile_shape_zyx[-1] + offset[0], ty * tile_shape_zyx[-2] + offset[1], offset[2]),
        np.int64)
    local_warp_box = Box(sub_box.start - out_box.start + local_out_start, sub_box.size)

    s = 1.0 / np.array(stride)[::-1]
    lo = np.floor(local_warp_box.start * s).astype(np.int64) - 2
    hi = np.ceil(local_warp_box.end * s).astype(np.int64) + 2
    local_map_box = _intersection(Box(lo, hi - lo), tg_box)
    if local_map_box is None:
      continue
    q0 = local_map_box.start - tg_box.start
    q1 = q0 + local_map_box.size
    assert np.all(q0 >= 0)
    sub_map = inverted_map[:, int(q0[2]):int(q1[2]), int(q0[1]):int(q1[1]), int(q0[0]):int(q1[0])]

    data_box = _as_box(map_utils.outer_box(sub_map, local_map_box, stride, 1))
    data_box = _intersection(data_box, image_box)
    if data_box is None:
      continue
    plan.append((i, data_box, tg_box, local_warp_box, sub_box))
  return plan


def fill_inverted(inverted) -> dict[int, tuple[Box, DeviceArray]]:
  """{i: (tg_box, inverted_map)} with the maps' NaN nodes filled by the nearest
  valid node, the reference's `fill_missing(extrapolate=True,
  interpolate_first=False)` of processor/warp.py:199-203, on the device.

  inverted: {i: (tg_box, [3, z, y, x] map)} as the 3-D `invert_map` leaves them
  (NaN outside the hull of the tile's nodes; NumPy, torch or DeviceArray).
  Returns float64 DeviceArrays, ready for `plan_render` / `TileRenderer`.
  """
  filled = {}
  for i, (tg_box, inv) in inverted.items():
    inv = _array(inv)
    inv = inv.to(torch.float64) if isinstance(inv, torch.Tensor) else np.asarray(
        inv, dtype=np.float64)
    filled[i] = _as_box(tg_box), map_utils.fill_missing(
        inv, extrapolate=True, interpolate_first=False)
  return filled


_DTYPES = {np.dtype(np.uint8): _abi.DTYPE_U8, np.dtype(np.uint16): _abi.DTYPE_U16,
           np.dtype(np.float32): _abi.DTYPE_F32}
_TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16,
          np.dtype(np.float32): torch.float32}


def _device_tile(tile, dev) -> torch.Tensor:
  """[z, y, x] uint8 / uint16 / float32 contiguous device tensor; a tile that is
  on the device already is used where it lies."""
  if isinstance(tile, DeviceArray):
    tile = tile.tensor
  if isinstance(tile, torch.Tensor):
    t = tile.to(dev).contiguous()
  else:
    arr = np.ascontiguousarray(tile)
    if arr.dtype == np.uint64:
      raise NotImplementedError('render: uint64 label tiles')
    if arr.dtype not in _DTYPES:
      raise NotImplementedError(f'render: {arr.dtype} tiles (uint8, uint16, float32)')
    view = arr.view(np.int16) if arr.dtype == np.uint16 else arr
    t = _dev.upload(view, dev)
    if arr.dtype == np.uint16:
      t = t.view(torch.uint16)
  if t.dtype not in _TORCH.values():
    raise NotImplementedError(f'render: {t.dtype} tiles (uint8, uint16, float32)')
  if t.ndim != 3:
    raise ValueError(f'render: tiles are [z, y, x], got shape {tuple(t.shape)}')
  return t


def _device_abs_map(inverted_map, stride, dev) -> torch.Tensor:
  """The request-independent part of the absolute source map of
  warp.ndimage_warp (warp.py:249): inverted map + node index * stride, float64."""
  m = _array(inverted_map)
  if isinstance(m, torch.Tensor):
    m = m.to(device=dev, dtype=torch.float64)
  else:
    m = np.asarray(m, dtype=np.float64)
  if m.ndim != 4 or m.shape[0] != 3:
    raise ValueError(f'render: inverted maps are [3, z, y, x], got shape {tuple(m.shape)}')
  return map_utils.to_absolute(m, stride).tensor


def _device_weights(w, dev) -> torch.Tensor:
  w = _array(w)
  if isinstance(w, torch.Tensor):
    return w.to(device=dev, dtype=torch.float32).contiguous()
  return _dev.upload(np.ascontiguousarray(w, dtype=np.float32), dev)


def _launch(box: Box, plan, tiles, abs_maps, weights, stride, order, out_dtype,
            device_output):
  """One sfm_render_tiles3d call over device-resident arrays (dicts by tile)."""
  _spline.check_order(order, 'render')
  dev = _dev.device()
  dtypes = {np.dtype(str(tiles[item[0]].dtype).replace('torch.', '')) for item in plan}
  if len(dtypes) > 1:
    raise ValueError(f'render: tiles of different dtypes: {sorted(map(str, dtypes))}')
  if dtypes:
    tile_dtype = dtypes.pop()
  elif out_dtype is not None:
    tile_dtype = np.dtype(out_dtype)
  else:
    raise ValueError('render: an empty plan needs out_dtype')
  out_dtype = tile_dtype if out_dtype is None else np.dtype(out_dtype)
  if out_dtype != tile_dtype and out_dtype != np.float32:
    raise NotImplementedError(
        f'render: out_dtype {out_dtype} for {tile_dtype} tiles (the tile dtype or float32)')
  if tile_dtype not in _DTYPES:
    raise NotImplementedError(f'render: {tile_dtype} tiles (uint8, uint16, float32)')

  stride_zyx = np.asarray(stride)
  table = (_abi.SfmRenderTile * max(len(plan), 1))()
  regions = []
  for r, (i, data_box, tg_box, local_warp_box, sub_box) in zip(table, plan):
    data_box, tg_box = _as_box(data_box), _as_box(tg_box)
    local_warp_box, sub_box = _as_box(local_warp_box), _as_box(sub_box)
    tile, amap, w = tiles[i], abs_maps[i], weights[i]
    if tuple(w.shape) != tuple(tile.shape[1:]):
      raise ValueError(f'render: tile {i}: weights {tuple(w.shape)} for a tile '
                       f'{tuple(tile.shape)}')
    if np.any(sub_box.size != local_warp_box.size):
      raise ValueError(f'render: tile {i}: sub_box and local_warp_box differ in size')
    if np.any(tg_box.size[::-1] != tuple(amap.shape[1:])):
      raise ValueError(f'render: tile {i}: tg_box {tg_box.size} for a map {tuple(amap.shape)}')
    # the scalars of warp.py:255-258 and :288, formed as NumPy forms them there
    shift = tg_box.start * stride_zyx[::-1] - data_box.start / np.ones(3)
    node0 = (tg_box.start * stride_zyx[::-1] - local_warp_box.start)[::-1]
    r.image, r.abs_map, r.weights = tile.data_ptr(), amap.data_ptr(), w.data_ptr()
    r.tile_shape = (C.c_int32 * 3)(*tile.shape)
    r.map_shape = (C.c_int32 * 3)(*amap.shape[1:])
    r.data_start = (C.c_int32 * 3)(*(int(v) for v in data_box.start[::-1]))
    r.data_size = (C.c_int32 * 3)(*(int(v) for v in data_box.size[::-1]))
    r.sub_start = (C.c_int32 * 3)(*(int(v) for v in (sub_box.start - box.start)[::-1]))
    r.sub_size = (C.c_int32 * 3)(*(int(v) for v in sub_box.size[::-1]))
    r.shift = (C.c_double * 3)(*(float(v) for v in shift))
    r.offset = (C.c_double * 3)(*(float(v) for v in node0))
    if order in _spline.ORDERS:
      # the crop the reference warps, where it lies in the tile
      start, size = tuple(r.data_start), tuple(r.data_size)
      if any(a < 0 or a + n > t or n < 1 for a, n, t in zip(start, size, tile.shape)):
        raise ValueError(f'render: tile {i}: data_box {data_box} leaves the tile')
      pitch = (tile.shape[1] * tile.shape[2], tile.shape[2], 1)
      first = sum(a * p for a, p in zip(start, pitch))
      regions.append((tile.data_ptr() + first * tile.element_size(), size, pitch))

  out_shape = tuple(int(v) for v in box.size[::-1])
  out_t = torch.empty(out_shape, dtype=_TORCH[out_dtype], device=dev)
  d = _abi.SfmRenderTilesDesc()
  d.dtype = _DTYPES[tile_dtype]
  d.out_dtype = _DTYPES[out_dtype]
  d.order = int(order)
  d.n_tiles = len(plan)
  d.out_shape = (C.c_int32 * 3)(*out_shape)
  d.stride = (C.c_double * 3)(*(float(v) for v in stride_zyx))
  table_t = None
  if plan:
    table_t = _dev.upload(np.frombuffer(table, dtype=np.uint8).copy(), dev)
    d.tiles_host = table
    d.tiles = table_t.data_ptr()
  d.out = out_t.data_ptr()
  d.stream = _dev.stream_ptr()
  if order in _spline.ORDERS:
    # coefficients of all crops, dense and back to back in plan order: what the
    # kernel expects
    coeffs, _ = _spline.prefilter(regions, _DTYPES[tile_dtype], order, dev)
    _abi.check(_abi.load().sfm_render_tiles3d_spline(C.byref(d), coeffs.data_ptr()))
  else:
    _abi.check(_abi.load().sfm_render_tiles3d(C.byref(d)))
  if device_output:
    return DeviceArray(out_t)
  if out_dtype == np.uint16:
    return out_t.view(torch.int16).cpu().numpy().view(np.uint16)
  return out_t.cpu().numpy()


def render(box, tiles, plan, inverted, weights, stride: Sequence[float], *, order: int = 1,
           out_dtype=None, device_output: bool = False):
  """Renders the output box from the tiles of `plan` (processor/warp.py:292-343).

  box: the output box; tiles: {i: [z, y, x] whole tile} (NumPy, torch or
  DeviceArray; uint8, uint16 or float32; the `data_box` region is read in
  place, tiles on the device are not copied); plan: the result of
  `plan_render` for `box`; inverted: {i: (tg_box, inverted_map)} as given to
  `plan_render`; weights: {i: blend_weights of the tile}; stride: zyx mesh
  stride; order: 0 or 1, or with the switch SFM_SPLINE_ORDERS=1 2 to 5, for the
  image (the weights are always sampled with order 1; orders 2 to 5 prefilter the `data_box` crops into a workspace of 8
  bytes per crop voxel).  Returns [z, y, x] of `out_dtype` (the tile dtype by default;
  float32 is the only other choice), as NumPy or, with `device_output`, as a
  DeviceArray.
  """
  box = _as_box(box)
  if not plan and out_dtype is None:
    any_tile = next(iter(tiles.values()), None)
    out_dtype = None if any_tile is None else _array(any_tile).dtype
    if isinstance(out_dtype, torch.dtype):
      out_dtype = np.dtype(str(out_dtype).replace('torch.', ''))
  dev = _dev.device()
  used = [item[0] for item in plan]
  dev_tiles = {i: _device_tile(tiles[i], dev) for i in used}
  abs_maps = {i: _device_abs_map(inverted[i][1], stride, dev) for i in used}
  dev_weights = {i: _device_weights(weights[i], dev) for i in used}
  return _launch(box, plan, dev_tiles, abs_maps, dev_weights, stride, order, out_dtype,
                 device_output)


class TileRenderer:
  """The tiles, inverted maps, weights and tile boxes of one montage, resident on
  the device: `render(box)` plans and renders one output box, and a sweep over
  many boxes uploads nothing but the per-request tile table.

  tiles: {i: [z, y, x]}; tile_meshes: [3, n_tiles, z, y, x]; tile_idx_to_xy:
  {i: (tx, ty)}; inverted: {i: (tg_box, inverted_map)} (see `plan_render`);
  stride: zyx; grid_shape_yx: shape of the tile grid (default: the extent of
  `tile_idx_to_xy`); the rest as the constructor arguments of the reference
  processor.
  """

  def __init__(self, tiles, tile_meshes, tile_idx_to_xy, inverted, stride, *,
               offset: Sequence[int] = (0, 0, 0), margin: int = 0, order: int = 1,
               grid_shape_yx: Sequence[int] | None = None, out_dtype=None):
    dev = _dev.device()
    self.stride = tuple(stride)
    self.offset = tuple(offset)
    self.order = order
    self.tile_idx_to_xy = dict(tile_idx_to_xy)
    self.tiles = {i: _device_tile(t, dev) for i, t in tiles.items()}
    shapes = {tuple(t.shape) for t in self.tiles.values()}
    if len(shapes) != 1:
      raise ValueError(f'TileRenderer: tiles of different shapes: {sorted(shapes)}')
    self.tile_shape_zyx = shapes.pop()
    first = next(iter(self.tiles.values()))
    self.out_dtype = np.dtype(str(first.dtype).replace('torch.', '')) if out_dtype is None \
        else np.dtype(out_dtype)
    if grid_shape_yx is None:
      grid_shape_yx = (max(xy[1] for xy in self.tile_idx_to_xy.values()) + 1,
                       max(xy[0] for xy in self.tile_idx_to_xy.values()) + 1)
    self.inverted = {}
    self.abs_maps = {}
    for i, (tg_box, inv) in inverted.items():
      inv = _array(inv)
      inv_t = inv.to(device=dev, dtype=torch.float64).contiguous() if isinstance(
          inv, torch.Tensor) else _dev.upload(np.ascontiguousarray(inv, dtype=np.float64), dev)
      self.inverted[i] = _as_box(tg_box), inv_t
      self.abs_maps[i] = _device_abs_map(inv_t, self.stride, dev)
    self.weights = {
        i: blend_weights(self.tile_shape_zyx, *self.tile_idx_to_xy[i], grid_shape_yx, margin,
                         device=True).tensor for i in self.tiles}
    meshes = _array(tile_meshes)
    if not isinstance(meshes, torch.Tensor):
      meshes = _dev.upload(np.ascontiguousarray(meshes), dev)
    self.boxes = tile_boxes(meshes, self.tile_idx_to_xy, self.tile_shape_zyx, self.stride,
                            self.offset)

  def plan(self, box):
    return plan_render(box, self.boxes, self.inverted, self.tile_idx_to_xy,
                       self.tile_shape_zyx, self.stride, self.offset)

  def render(self, box, device_output: bool = False, plan=None):
    """[z, y, x] rendering of `box`; `plan` reuses the result of `self.plan(box)`."""
    box = _as_box(box)
    if plan is None:
      plan = self.plan(box)
    return _launch(box, plan, self.tiles, self.abs_maps, self.weights, self.stride,
                   self.order, self.out_dtype, device_output)
