"""Elastic tile montages on MI355X.

Drop-in for the reference's `stitch_elastic.py`.  The in-plane chain is
`compute_flow_map` -> per tile pair `clean_flow` + `reconcile_flows` ->
`aggregate_arrays` -> `relax_mesh(prev_fn=compute_target_mesh)`; with
`device_output=True` the flows stay in HBM from the correlation peaks to the
mesh solve:

  * `compute_flow_map` / `compute_flow_map3d` (stitch_elastic.py:85-282): one
    `flow_field` call per pair of overlap strips;
  * `filter_flow_maps` (an extension): `flow_utils.clean_flow` +
    `flow_utils.reconcile_flows` of every tile-pair flow of a montage in ONE
    launch, each pair on its own extent; returns a `TileFlows`;
  * `aggregate_arrays` (stitch_elastic.py:285-453): the packing of flows, tile
    meshes and neighbour metadata, on the host as in the reference or, with
    `device_output=True`, assembled on the device;
  * `compute_target_mesh` (stitch_elastic.py:624-676, with `_update_mesh`
    :573-620 and `_apply_flow` :456-570) -- the `prev_fn` that `mesh.relax_mesh`
    evaluates inside every force evaluation when a montage is relaxed.

The notebooks build the prev_fn as
    jit(lambda x: transpose(vmap(partial(compute_target_mesh, x=x, fx=fx, fy=fy,
                                         stride=stride))(nbors), [1, 0, 2, 3]))
`TargetMeshFn(nbors, fx, fy, stride)` is that function as one HIP kernel;
`mesh.relax_mesh(x, None, cfg, prev_fn=TargetMeshFn(...))` runs it natively.
"""
from __future__ import annotations

import collections.abc
import ctypes as C
import enum

import numpy as np
import torch

from . import _abi
from . import _dev
from ._dev import DeviceArray


class NeighborInfo(enum.IntEnum):
  """Indices in a neighbour-info row (stitch_elastic.py:43-72)."""
  nbor_idx = 0
  flow_idx = 1
  coarse_offset_ortho = 2
  flow_size_ortho = 3
  flow_size_overlap = 4
  fine_off_x = 5
  fine_off_y = 6
  dim = 7
  coarse_offset_z = 8
  flow_size_z = 9
  fine_off_z = 10


class TargetMeshFn:
  """prev_fn(x) for all tiles of a montage.

  In-plane: x [2, N, y, x] -> [2, N, y, x] (flows fx / fy [2, n, y, x], stride
  yx, 8 neighbour fields).  Volumetric: x [3, N, z, y, x] -> the same (flows
  [3, n, z, y, x], stride zyx, 11 neighbour fields).
  """

  def __init__(self, nbors, fx, fy, stride=(20, 20)):
    dev = _dev.device()
    nb = np.ascontiguousarray(np.asarray(nbors), dtype=np.int32)
    if nb.ndim != 3 or nb.shape[1] != 4 or nb.shape[2] < 8:
      raise ValueError('nbors must be [n_tiles, 4, 8 or 11]')
    self.fx = _dev.as_device_f32(fx, dev, copy=False)
    self.fy = _dev.as_device_f32(fy, dev, copy=False)
    ncomp = int(self.fx.shape[0])
    if ncomp not in (2, 3) or self.fx.ndim != ncomp + 2 or self.fy.ndim != ncomp + 2:
      raise ValueError('flows must be [2, n, y, x] or [3, n, z, y, x]')
    if ncomp == 3 and nb.shape[2] < 11:
      raise ValueError('volumetric montages need the 11-field NeighborInfo rows')
    if len(stride) != ncomp:
      raise ValueError('stride must be [z]yx with one entry per spatial dimension')
    self.ncomp = ncomp
    self.nbors = torch.from_numpy(nb).to(dev)
    self.stride = tuple(float(s) for s in stride)
    d = _abi.SfmTargetMeshDesc()
    d.ncomp = ncomp
    d.n_tiles = nb.shape[0]
    lead = [1] * (3 - ncomp)
    d.fx_shape = (C.c_int32 * 3)(*lead, *self.fx.shape[2:])
    d.fy_shape = (C.c_int32 * 3)(*lead, *self.fy.shape[2:])
    d.n_fx = self.fx.shape[1]
    d.n_fy = self.fy.shape[1]
    d.nbor_fields = nb.shape[2]
    d.stride = (C.c_float * 3)(*([1.0] * (3 - ncomp)), *self.stride)
    d.nbors = self.nbors.data_ptr()
    d.fx = self.fx.data_ptr()
    d.fy = self.fy.data_ptr()
    self.desc = d

  def bind(self, x_t: torch.Tensor) -> _abi.SfmTargetMeshDesc:
    if (x_t.ndim != self.ncomp + 2 or x_t.shape[0] != self.ncomp or
        x_t.shape[1] != self.desc.n_tiles):
      raise ValueError('x must be [2, n_tiles, y, x] or [3, n_tiles, z, y, x]')
    self.desc.mesh_shape = (C.c_int32 * 3)(*([1] * (3 - self.ncomp)), *x_t.shape[2:])
    return self.desc

  def __call__(self, x) -> DeviceArray:
    dev = _dev.device()
    x_t = _dev.as_device_f32(x, dev, copy=False)
    d = self.bind(x_t)
    out = torch.empty_like(x_t)
    _abi.check(_abi.load().sfm_target_mesh(C.byref(d), x_t.data_ptr(),
                                           out.data_ptr(), _dev.stream_ptr()))
    return DeviceArray(out)


def compute_target_mesh(nbor_data, x, fx, fy, stride=(20, 20)) -> np.ndarray:
  """Target positions for ONE tile mesh (stitch_elastic.py:624-676).

  nbor_data: [4, 8 or 11] neighbour info of the tile; x, fx, fy as in the
  reference (in-plane [2, n, y, x] or volumetric [3, n, z, y, x]).
  Only this tile is evaluated (`SfmTargetMeshDesc.n_eval = 1`).
  """
  dev = _dev.device()
  x_t = _dev.as_device_f32(x, dev, copy=False)
  fn = TargetMeshFn(np.asarray(nbor_data)[None], fx, fy, stride)
  d = fn.desc
  # ONE row of neighbour info evaluated against the meshes of all n tiles
  d.n_tiles = int(x_t.shape[1])
  d.n_eval = 1
  d.mesh_shape = (C.c_int32 * 3)(*([1] * (3 - fn.ncomp)), *x_t.shape[2:])
  out = torch.empty((fn.ncomp, 1) + tuple(x_t.shape[2:]), dtype=torch.float32,
                    device=dev)
  _abi.check(_abi.load().sfm_target_mesh(C.byref(d), x_t.data_ptr(), out.data_ptr(),
                                         _dev.stream_ptr()))
  return out[:, 0].cpu().numpy()


def _overlap_strips(pre, post, off_xy, axis: int, stride):
  """Overlap strips of an adjacent tile pair, aligned to the flow stride
  (stitch_elastic.py:232-262), and the offset recorded for them (:277-280).

  off_xy: coarse (x, y) offset of `post`; stride is yx.
  """
  along = 1 - axis                    # image axis of the tile-tile connection
  # strip width: the start inside `pre` is moved down to a stride multiple
  extent = pre.shape[along]
  start = (extent + int(off_xy[axis])) // stride[along] * stride[along]
  overlap = extent - start
  # orthogonal shift, rounded to the stride of that image axis
  s_ortho = stride[::-1][1 - axis]
  ortho = int(s_ortho * np.round(off_xy[1 - axis] / s_ortho))
  pre_sl = [slice(None), slice(None)]
  post_sl = [slice(None), slice(None)]
  pre_sl[along] = slice(start, None)
  post_sl[along] = slice(0, overlap)
  if ortho > 0:                       # post sits further along the ortho axis
    pre_sl[axis] = slice(ortho, None)
    post_sl[axis] = slice(None, -ortho)
  elif ortho < 0:
    pre_sl[axis] = slice(None, ortho)
    post_sl[axis] = slice(-ortho, None)
  off = (-overlap, ortho) if axis == 0 else (ortho, -overlap)
  return pre[tuple(pre_sl)], post[tuple(post_sl)], off


# Tile pairs whose flow_field() call may be enqueued before the oldest result is
# fetched (compute_flow_map, compute_flow_map3d): enough for the host to stay
# ahead of the GPU, small enough to bound the device memory held by queued pairs.
MAX_PAIRS_IN_FLIGHT = 8


def compute_flow_map(tile_map, offset_map: np.ndarray, axis: int,
                     patch_size=(120, 120), stride=(20, 20),
                     batch_size: int = 256, device_output: bool = False):
  """Fine flow between horizontally (axis 0) or vertically (axis 1) adjacent
  2-d tiles (stitch_elastic.py:198-282).

  tile_map: (x, y) -> tile image; offset_map: [2, y, x] coarse XY offsets of
  the (x+1, y) / (x, y+1) tile.  Returns ({(x, y): flow [4, gy, gx]},
  {(x, y): (off_x, off_y) at which the flow was computed}); the flow arrays are
  NaN-padded by patch // 2 // stride nodes so that they are aligned with the
  tile's mesh.  Every pair is one `flow_field` call on the overlap strips,
  i.e. the int8 matrix-core correlation for uint8 tiles.  `device_output=True`
  (an extension) returns the flows as DeviceArrays, NaN-padded on the device,
  without fetching them (`filter_flow_maps` takes them as they are).
  """
  from . import flow_field
  calc = flow_field.JAXMaskedXCorrWithStatsCalculator()
  patch_size = tuple(int(p) for p in patch_size)
  stride = tuple(int(s) for s in stride)
  pads = [(0, 0)] + [(p // 2 // s, p // 2 // s - 1)
                     for p, s in zip(patch_size, stride)]
  grid_y, grid_x = offset_map.shape[-2:]
  flows, offsets = {}, {}
  # every pair is enqueued before the first result is fetched: the fields stay
  # in HBM until the loop is done, so the host prepares pair n + 1 while the GPU
  # works on pair n (a strip pair of the 8 x 8 montage: 0.97 -> 0.7x ms)
  pending, events = [], []
  for y in range(grid_y - axis):
    for x in range(grid_x - (1 - axis)):
      off_xy = offset_map[:, y, x]
      if np.isnan(off_xy[0]):
        continue
      pre, post, off = _overlap_strips(
          tile_map[x, y], tile_map[x + (1 - axis), y + axis], off_xy, axis,
          stride)
      f = calc.flow_field(pre, post, patch_size=patch_size, step=stride,
                          batch_size=batch_size, device_output=True)
      offsets[x, y] = off
      if device_output:
        # (left, right) per axis from the last one; the NaN np.pad writes
        flows[x, y] = DeviceArray(torch.nn.functional.pad(
            f.tensor, (pads[2][0], pads[2][1], pads[1][0], pads[1][1]),
            value=float('nan')))
        # nothing is fetched: the same bound on the run-ahead, through events
        done = torch.cuda.Event()
        done.record()
        events.append(done)
        if len(events) >= MAX_PAIRS_IN_FLIGHT:
          events.pop(0).synchronize()
        continue
      pending.append(((x, y), f))
      # bounded run-ahead: strips and workspaces of the queued pairs stay
      # allocated until the compute stream has passed them
      if len(pending) >= MAX_PAIRS_IN_FLIGHT:
        key, f = pending.pop(0)
        flows[key] = np.pad(np.asarray(f), pads, constant_values=np.nan)
  for key, f in pending:
    flows[key] = np.pad(np.asarray(f), pads, constant_values=np.nan)
  return flows, offsets


def _aligned_overlap3d(tile_shape, offset, axis: int, stride):
  """Overlap region of a 3-d tile pair, aligned to the flow stride
  (stitch_elastic.py:125-180).

  tile_shape, offset: xyz; stride: zyx.  The neighbour sits at the grid step
  along `axis` plus `offset`.  Its position is nudged so that, inside the
  current tile, the overlap starts on a multiple of s = stride[2 - axis] along
  every axis (the reference aligns ALL axes to the stride of the connection
  axis).  Returns (start in the current tile, start in the neighbour, size)
  -- xyz integers -- and the xyz offset recorded for the pair.
  """
  shape = np.asarray(tile_shape, dtype=np.float64)
  # (the reference keeps the neighbour position in a connectomics BoundingBox,
  # whose corners are integers: a fractional coarse offset is truncated there --
  # third-party semantics, absent from /root/reference, pinned for integer
  # offsets only -- and the recorded offsets are ints)
  pos = np.array([shape[0] * (1 - axis) + offset[0], shape[1] * axis + offset[1],
                  offset[2]], dtype=np.float64)
  pos = np.trunc(pos)

  def overlap(nb):
    lo = np.maximum(0.0, nb)
    hi = np.minimum(shape, nb + shape)
    return lo, lo - nb, hi - lo        # start in current, start in neighbour, size

  s = stride[2 - axis]
  cur0, nb0, size0 = overlap(pos)
  nudge = np.zeros(3)
  # along the connection: the strip starts on a multiple of s inside the current
  # tile (moved towards its origin, i.e. the strip only grows)
  first = shape[axis] - size0[axis]
  nudge[axis] = -((shape[axis] - first // s * s) - size0[axis])
  for ax in range(3):
    if ax == axis:
      continue
    if cur0[ax] > 0:
      nudge[ax] = s * np.round(cur0[ax] / s) - cur0[ax]
    elif nb0[ax] > 0:
      nudge[ax] = -(s * np.round(nb0[ax] / s) - nb0[ax])
  pos = pos + nudge
  cur, nb, size = overlap(pos)
  assert np.all(cur % s == 0) and np.all(nb % s == 0)
  rec = pos.copy()
  rec[axis] = -size[axis]
  return (cur.astype(int), nb.astype(int), size.astype(int),
          tuple(int(v) for v in rec))


def compute_flow_map3d(tile_map, tile_shape, offset_map: np.ndarray, axis: int,
                       patch_size=(120, 120, 120), stride=(40, 40, 40),
                       batch_size: int = 16):
  """Fine flow between horizontally (axis 0) or vertically (axis 1) adjacent
  3-d tiles (stitch_elastic.py:85-194).

  tile_map: (x, y) -> [1, z, y, x] volume (any indexable); tile_shape: xyz;
  offset_map: [3, 1, y, x] coarse xyz offsets of the (x+1, y) / (x, y+1) tile;
  patch_size / stride: zyx.  Returns ({(x, y): flow [5, gz, gy, gx]}, {(x, y):
  xyz offset at which the neighbour was positioned for the flow}); flows are
  NaN-padded by patch // 2 // stride nodes like the reference's.  Every pair is
  one volumetric `flow_field` call (FFT form) on the aligned overlap.
  """
  from . import flow_field
  calc = flow_field.JAXMaskedXCorrWithStatsCalculator()
  patch_size = tuple(int(p) for p in patch_size)
  stride = tuple(int(v) for v in stride)
  pads = [(0, 0)] + [(p // 2 // v, p // 2 // v - 1) for p, v in zip(patch_size, stride)]
  grid_y, grid_x = offset_map.shape[-2:]
  flows, offsets = {}, {}
  pending = []
  for y in range(grid_y - axis):
    for x in range(grid_x - (1 - axis)):
      cur, nb, size, rec = _aligned_overlap3d(tile_shape, offset_map[:, 0, y, x], axis,
                                              stride)

      def crop(tile, start):          # xyz start / size -> [z, y, x] block
        sl = tuple(slice(int(a), int(a + n)) for a, n in zip(start[::-1], size[::-1]))
        return np.asarray(tile[(slice(None),) + sl]).squeeze(axis=0)

      pre = crop(tile_map[x, y], cur)
      post = crop(tile_map[x + (1 - axis), y + axis], nb)
      assert pre.shape == post.shape
      pending.append(((x, y), calc.flow_field(
          pre, post, patch_size=patch_size, step=stride, batch_size=batch_size,
          device_output=True)))
      offsets[x, y] = rec
      if len(pending) >= MAX_PAIRS_IN_FLIGHT:   # two overlap volumes + FFT workspace each
        key, f = pending.pop(0)
        flows[key] = np.pad(np.asarray(f), pads, constant_values=np.nan)
  for key, f in pending:   # fetched after the last pair is enqueued (compute_flow_map)
    flows[key] = np.pad(np.asarray(f), pads, constant_values=np.nan)
  return flows, offsets


class TileFlows(collections.abc.Mapping):
  """The filtered fine flows of a montage (`filter_flow_maps`): a read-only
  mapping over the tile-pair keys, in input order, on top of one device array.

  data: DeviceArray [2, n, Y, X] float32, Y, X the largest extents, NaN outside
  a pair's own extent; shapes: host int32 [n, 2], the (h, w) of every pair;
  batched: host bool [n], the pairs the batched kernel took (the others went
  through `clean_flow` + `reconcile_flows`).  `tf[key]` is the pair's
  DeviceArray [2, h, w] (a view of `data`).
  """

  def __init__(self, keys, data: DeviceArray, shapes: np.ndarray, batched: np.ndarray):
    self._index = {k: i for i, k in enumerate(keys)}
    self.data = data
    self.shapes = shapes
    self.batched = batched
    for a in (self.shapes, self.batched):
      a.setflags(write=False)

  def __getitem__(self, key) -> DeviceArray:
    i = self._index[key]
    h, w = self.shapes[i]
    return DeviceArray(self.data.tensor[:, i, :h, :w])

  def __contains__(self, key):
    return key in self._index

  def __iter__(self):
    return iter(self._index)

  def __len__(self):
    return len(self._index)

  def index(self, key) -> int:
    """Position of the pair along the second axis of `data`."""
    return self._index[key]

  def to_host(self) -> dict:
    """{key: NumPy [2, h, w]}, fetched in one copy."""
    host = np.asarray(self.data)
    return {k: host[:, i, :self.shapes[i, 0], :self.shapes[i, 1]].copy()
            for k, i in self._index.items()}

  def __repr__(self):
    return f'TileFlows({len(self)} pairs, data={self.data})'


def _pack_rows(values, rows, n_rows: int, channels: int, spatial, dev) -> torch.Tensor:
  """float32 device tensor [channels, n_rows, *spatial], NaN except that
  [:, rows[j]] starts with the first `channels` channels of values[j] (NumPy
  arrays, torch tensors or DeviceArrays of their own, smaller extents).  Host
  values go up in one copy; device values are stacked per shape.  The inputs are
  not written."""
  spatial = tuple(int(s) for s in spatial)
  host, on_device = [], {}
  for v, r in zip(values, rows):
    if isinstance(v, DeviceArray):
      v = v.tensor
    if isinstance(v, torch.Tensor) and v.is_cuda:
      on_device.setdefault(tuple(v.shape), []).append((r, v))
    else:
      host.append((r, np.asarray(v)))
  staged = None
  if host:
    stage = np.full((channels, len(host)) + spatial, np.nan, np.float32)
    for j, (_, a) in enumerate(host):
      c = min(channels, a.shape[0])
      stage[(slice(0, c), j) + tuple(slice(0, s) for s in a.shape[1:])] = a[:c]
    staged = _dev.upload(stage, dev)
    if not on_device and [r for r, _ in host] == list(range(n_rows)):
      return staged
  out = torch.full((channels, n_rows) + spatial, float('nan'), dtype=torch.float32, device=dev)
  if host:
    out.index_copy_(1, torch.tensor([r for r, _ in host], device=dev), staged)
  for shape, items in on_device.items():
    c = min(channels, shape[0])
    block = torch.stack([v[:c].to(device=dev, dtype=torch.float32) for _, v in items], dim=1)
    where = (slice(0, c), torch.tensor([r for r, _ in items], device=dev))
    out[where + tuple(slice(0, s) for s in shape[1:])] = block
  return out


def filter_flow_maps(flows, clean=None, reconcile=None) -> TileFlows:
  """`flow_utils.clean_flow` + `flow_utils.reconcile_flows` of every tile-pair
  flow of a montage, in one launch (an extension; the notebooks loop over the
  pairs).

  flows: mapping (x, y) -> [c, h, w] with c in (2, 4) -- what `compute_flow_map`
  returns -- NumPy arrays, torch tensors or DeviceArrays, mixed, of any extents;
  never written.  clean: dict of `clean_flow`'s four thresholds, reconcile: dict
  of `reconcile_flows`' max_gradient, max_deviation, min_patch_size; None skips
  the stage.  Per key and bit for bit the result is
      a = clean_flow(v[:, None], **clean)        # v[:2, None] when clean is None
      b = reconcile_flows([a], **reconcile)      # a when reconcile is None
      out[key] = b[:, 0]
  with every pair filtered on its own extent.  Pairs with more vectors than a
  workgroup holds (`sfm_filter_tile_flows_max_nodes`) go through those two calls;
  `TileFlows.batched` says which.
  """
  from . import flow_utils
  keys = list(flows.keys())
  vals = [flows[k] for k in keys]
  shapes = []
  for k, v in zip(keys, vals):
    shape = tuple(int(s) for s in v.shape)
    if len(shape) != 3 or shape[0] not in (2, 4) or min(shape[1:]) < 1:
      raise ValueError(f'flow {k} must be [c, h, w] with c in (2, 4) and h, w >= 1, '
                       f'got {shape}')
    shapes.append(shape)
  clean_t = flow_utils._clean_thresholds(**clean) if clean is not None else None
  reconcile_t = (flow_utils._reconcile_thresholds(**reconcile)
                 if reconcile is not None else None)
  dev = _dev.device()
  n = len(keys)
  extents = np.array([s[1:] for s in shapes], np.int32).reshape(n, 2)
  if n == 0:
    empty = torch.empty((2, 0, 0, 0), dtype=torch.float32, device=dev)
    return TileFlows(keys, DeviceArray(empty), extents, np.zeros(0, bool))
  lib = _abi.load()
  batched = extents[:, 0].astype(np.int64) * extents[:, 1] <= lib.sfm_filter_tile_flows_max_nodes()
  taken = np.flatnonzero(batched)
  data = None
  if len(taken):
    ext = np.ascontiguousarray(extents[taken])
    padded = tuple(int(v) for v in ext.max(axis=0))
    # a 2-channel pair among 4-channel ones carries NaN as sharpness and ratio:
    # comparisons with NaN are false, so the peak tests pass it as clean_flow does
    channels = 4 if clean is not None and any(shapes[i][0] == 4 for i in taken) else 2
    packed = _pack_rows([vals[i] for i in taken], range(len(taken)), len(taken), channels,
                        padded, dev)
    ext_dev = torch.from_numpy(ext).to(dev)
    out = torch.empty((2, len(taken)) + padded, dtype=torch.float32, device=dev)
    d = _abi.SfmTileFlowsDesc()
    d.channels = channels
    d.n = len(taken)
    d.padded_shape = (C.c_int32 * 2)(*padded)
    d.extents = ext.ctypes.data
    d.extents_device = ext_dev.data_ptr()
    if clean_t is not None:
      (d.min_peak_ratio, d.min_peak_sharpness, d.max_magnitude,
       d.clean_max_deviation) = clean_t
      d.do_clean = 1
    if reconcile_t is not None:
      d.max_gradient, d.max_deviation, d.min_patch_size, d.min_delta_z = reconcile_t
      d.do_reconcile = 1
    d.flows = packed.data_ptr()
    d.stream = _dev.stream_ptr()
    _abi.check(lib.sfm_filter_tile_flows(C.byref(d), out.data_ptr()))
    if len(taken) == n:
      data = out
  if data is None:
    full = tuple(int(v) for v in extents.max(axis=0))
    data = torch.full((2, n) + full, float('nan'), dtype=torch.float32, device=dev)
    if len(taken):
      data[:, torch.from_numpy(taken).to(dev), :padded[0], :padded[1]] = out
    for i in np.flatnonzero(~batched):
      v = _dev.as_device_f32(vals[i], dev, copy=False)
      a = (flow_utils.clean_flow(v[:, None], **clean) if clean is not None
           else DeviceArray(v[:2, None]))
      b = flow_utils.reconcile_flows([a], **reconcile) if reconcile is not None else a
      data[:, i, :shapes[i][1], :shapes[i][2]] = b.tensor[:, 0]
  return TileFlows(keys, DeviceArray(data), extents, batched)


def aggregate_arrays(x_data, y_data, tile_coords, coarse_mesh, stride, tile_shape,
                     device_output: bool = False):
  """Aggregates data for all tiles into single arrays (stitch_elastic.py:285-453).

  x_data / y_data: (coarse offsets [2 or 3, y, x] of the (x + 1, y) / (x, y + 1)
  tile, {(x, y): fine flow}, {(x, y): offset at which the flow was computed});
  tile_coords: sequence of (x, y); coarse_mesh: the rigid solution, indexed
  [:, y, x]; stride, tile_shape: [z]yx.  The fine flows may be NumPy arrays,
  DeviceArrays or a `TileFlows`; only their first 2 (3) channels are used.
  Returns (fx_all, fy_all, x_all, nbors, key_to_idx) as the reference does: the
  flows float64 [dim, n, [z,] y, x], NaN-padded to the largest flow ([dim, n, 1,
  1] of NaN without any flow), the tile meshes float32, the NeighborInfo rows
  int64 [n, 4, 8 or 11] with -1 where there is no neighbour.  With host flows
  nothing touches the device.  `device_output=True` (an extension) assembles
  fx_all, fy_all and x_all on the device as float32 DeviceArrays -- the values
  are float32 already -- which `TargetMeshFn` and `relax_mesh` take as they are;
  nbors and key_to_idx stay host objects.
  """
  cx, fine_x, offsets_x = x_data
  cy, fine_y, offsets_y = y_data
  cx, cy = np.asarray(cx), np.asarray(cy)
  assert cx.ndim == 3
  assert cy.ndim == 3
  key_to_idx = {(tx, ty): i for i, (tx, ty) in enumerate(tile_coords)}
  n = len(key_to_idx)
  dim = len(stride)
  unit = (dim,) + (1,) * dim

  def shape_of(f):
    return tuple(int(s) for s in f.shape)

  def pack(fine):
    # the largest flow of the dict, whether or not its tile is listed
    full = np.max([shape_of(v) for v in fine.values()] + [unit], axis=0)[1:].tolist()
    rows = [(k, i) for k, i in key_to_idx.items() if k in fine]
    if not device_output:
      host = fine.to_host() if isinstance(fine, TileFlows) else fine
      out = np.full([dim, n] + full, np.nan)
      for k, i in rows:
        f = np.asarray(host[k])
        out[(slice(None), i) + tuple(slice(0, s) for s in f.shape[1:])] = f[:dim]
      return out
    dev = _dev.device()
    if isinstance(fine, TileFlows) and dim == 2:
      # `data` is padded to the largest flow already
      out = torch.full([dim, n] + full, float('nan'), dtype=torch.float32, device=dev)
      if rows:
        src = torch.tensor([fine.index(k) for k, _ in rows], device=dev)
        out.index_copy_(1, torch.tensor([i for _, i in rows], device=dev),
                        fine.data.tensor.index_select(1, src))
      return DeviceArray(out)
    return DeviceArray(_pack_rows([fine[k] for k, _ in rows], [i for _, i in rows], n, dim,
                                  full, dev))

  fx_all, fy_all = pack(fine_x), pack(fine_y)

  def nbor_info(nbor_key, flow_key, coarse, fine, offsets, axis):
    sizes = shape_of(fine[flow_key])[-dim:]         # [z,] y, x
    ortho, overlap = sizes[-2:] if axis == 0 else sizes[-2:][::-1]
    off = offsets[flow_key]
    row = (key_to_idx[nbor_key], key_to_idx[flow_key], coarse[1] if axis == 0 else coarse[0],
           ortho, overlap, off[0], off[1], axis)
    if dim == 3:
      row += (coarse[2], sizes[0], off[2])
    return row

  # [tile, edge, NeighborInfo]: the -x, +x, -y, +y neighbours
  nbors = np.full((n, 4, 8 if dim == 2 else 11), -1, dtype=int)
  for tx, ty in tile_coords:
    edges = (
        ((tx - 1, ty), (tx - 1, ty), cx, fine_x, offsets_x, 0),
        ((tx + 1, ty), (tx, ty), cx, fine_x, offsets_x, 0),
        ((tx, ty - 1), (tx, ty - 1), cy, fine_y, offsets_y, 1),
        ((tx, ty + 1), (tx, ty), cy, fine_y, offsets_y, 1),
    )
    for e, (nbor_key, flow_key, coarse, fine, offsets, axis) in enumerate(edges):
      if flow_key in fine:
        nbors[key_to_idx[tx, ty], e, :] = nbor_info(
            nbor_key, flow_key, coarse[:, flow_key[1], flow_key[0]], fine, offsets, axis)

  # the coarse solution is the initial condition of every tile mesh
  mesh_shape = (np.array(tile_shape) // stride).tolist()
  coarse_mesh = np.asarray(coarse_mesh)
  if device_output:
    start = np.zeros((dim, n), np.float32)
    for tx, ty in tile_coords:
      start[:, key_to_idx[tx, ty]] = coarse_mesh[:, ty, tx].reshape(dim)
    x_all = torch.from_numpy(start).to(_dev.device()).reshape((dim, n) + (1,) * dim)
    x_all = DeviceArray(x_all.expand([dim, n] + mesh_shape).contiguous())
  else:
    x_all = np.zeros([dim, n] + mesh_shape, dtype=np.float32)
    for tx, ty in tile_coords:
      x_all[:, key_to_idx[tx, ty], ...] = coarse_mesh[:, ty, tx].reshape(unit)
  return fx_all, fy_all, x_all, nbors, key_to_idx
