"""The section loops around the flow estimator: `EstimateFlow`,
`EstimateMissingFlow` and `ReconcileAndFilterFlows`, at array level.

Drop-ins for the compute part of `processor/flow.py`:

  estimate_flow               <-> EstimateFlow.process         (processor/flow.py:163-245)
  missing_flow_geometry       <-> the box arithmetic of
                                  EstimateMissingFlow.process  (:634-737)
  estimate_missing_flow       <-> its section / look-back loop (:666-828)
  reconcile_and_filter_flows  <-> ReconcileAndFilterFlows.process (:386-493):
                                  clean, upsample the coarser flows onto the
                                  base lattice (`map_utils.resample_map`),
                                  reconcile

`EstimateMissingFlow` takes a 2-channel flow of a fixed look-back and tries to
fill the vectors that are NaN by correlating the section against earlier ones,
one look-back after the other, each time only at the nodes that are still
missing.  The result is the 3-channel flow `processor_mesh.relax_sections`
consumes, whose third channel names the look-back per node.  Boxes and volume
stores are replaced by arrays: the caller loads the image stack that
`missing_flow_geometry` names and hands it over.

The loop is many small rounds (sections x look-backs, a few hundred patches
each), so the image stack, the masks, the output planes and the per-section
`mask` / `attempts` state stay in HBM, and a round is planned and accepted by
two kernels of their own (`sfm_flow_select`, `sfm_missing_flow_update`) around
the correlation `flow_field()` runs.  Per round the host reads one integer.

Not covered: volume stores, mask configs, Beam counters and timers, image /
mask caches, 3-D flows, targeting fields, and batching several sections'
rounds into one correlation launch -- every (section, look-back) stays one
call, as in the reference, because the patches of a batch are coupled.
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
from typing import Any

import numpy as np

from . import flow_utils


@dataclasses.dataclass(frozen=True)
class MissingFlowGeometry:
  """What `EstimateMissingFlow.process` derives from its box; boxes are xyz
  (start, size) tuples, slices are (y, x)."""
  out_start: tuple[int, int, int]      # the output box, flow coordinates
  out_size: tuple[int, int, int]
  flow_slice: tuple[slice, slice]      # cuts the input flow [.., y, x] down to it
  load_start: tuple[int, int, int]     # the image box to load, clipped to the volume
  load_size: tuple[int, int, int]
  curr_slice: tuple[slice, slice]      # the current image inside a loaded section
  z0: int                              # index in the loaded stack of the section of flow[:, 0]


def _check_patch(patch_size: int, stride: int, search_radius: int) -> int:
  """processor/flow.py:571-582; returns the search patch size."""
  if patch_size % stride != 0:
    raise ValueError(f'patch_size {patch_size} not a multiple of stride {stride}')
  search_patch_size = patch_size + search_radius * 2
  if search_patch_size % stride != 0:
    raise ValueError(f'search_patch_size {search_patch_size} not a multiple of'
                     f' stride {stride}')
  return search_patch_size


def _clip(start, size, volume_size):
  """`clip_box_to_volume`: the intersection with [0, volume_size), or None."""
  lo = np.maximum(start, 0)
  hi = np.minimum(start + size, volume_size)
  if np.any(hi <= lo):
    return None
  return lo, hi - lo


def missing_flow_geometry(box_start, box_size, volume_size, *, patch_size: int, stride: int,
                          search_radius: int, delta_z: int, max_delta_z: int
                          ) -> MissingFlowGeometry | None:
  """The boxes of `EstimateMissingFlow.process` (processor/flow.py:634-737) for
  a flow box (xyz start and size, flow coordinates) over an image volume of
  `volume_size` (xyz).  None where the reference returns its input unchanged
  (no flow entry has enough image context, :652-653).  Host only, integers.

  The output box is the flow box without the nodes whose search window leaves
  the volume (:655-664); the image box to load spans the search windows of the
  remaining nodes in xy and the sections `delta_z` .. `max_delta_z` back in z,
  clipped to the volume (:696-722), so at the volume's first sections `z0` is
  smaller than `max_delta_z` and the look-backs end early.
  """
  search_patch_size = _check_patch(patch_size, stride, search_radius)
  start = np.array([int(v) for v in box_start], dtype=np.int64)
  size = np.array([int(v) for v in box_size], dtype=np.int64)
  vol = np.array([int(v) for v in volume_size], dtype=np.int64)
  half = search_patch_size // 2
  full_start = np.array([start[0] * stride - half, start[1] * stride - half, start[2]])
  full_size = np.array([(size[0] - 1) * stride + search_patch_size,
                        (size[1] - 1) * stride + search_patch_size, 1])
  prev = _clip(full_start, full_size, vol)
  if prev is None:
    raise ValueError('the flow box lies outside the image volume')
  prev_start, prev_size = prev
  if np.any(prev_size[:2] <= search_patch_size):
    return None

  # entries without sufficient image context are dropped on either side
  lo = (prev_start - full_start) // stride
  hi = -(((prev_start + prev_size) - (full_start + full_size)) // stride)    # ceil_div
  out_start = start + lo
  out_size = (start + size - hi) - out_start
  flow_slice = (slice(int(lo[1]), int(lo[1] + out_size[1])),
                slice(int(lo[0]), int(lo[0] + out_size[0])))

  curr = _clip(np.array([out_start[0] * stride - patch_size // 2,
                         out_start[1] * stride - patch_size // 2, out_start[2]]),
               np.array([(out_size[0] - 1) * stride + patch_size,
                         (out_size[1] - 1) * stride + patch_size, size[2]]), vol)
  if curr is None:
    raise ValueError('the current image box lies outside the image volume')
  curr_start, curr_size = curr
  out_end_z = out_start[2] + out_size[2]
  if delta_z > 0:
    load_z0, load_z1 = out_start[2] - max_delta_z, out_end_z
  else:
    load_z0, load_z1 = out_start[2], out_end_z - max_delta_z     # max_delta_z is negative
  load = _clip(np.array([prev_start[0], prev_start[1], load_z0]),
               np.array([prev_size[0], prev_size[1], load_z1 - load_z0]), vol)
  if load is None:
    raise ValueError('the image box to load lies outside the image volume')
  load_start, load_size = load
  rel = curr_start - load_start
  curr_slice = (slice(int(rel[1]), int(rel[1] + curr_size[1])),
                slice(int(rel[0]), int(rel[0] + curr_size[0])))
  as_tuple = lambda a: tuple(int(v) for v in a)
  return MissingFlowGeometry(as_tuple(out_start), as_tuple(out_size), flow_slice,
                             as_tuple(load_start), as_tuple(load_size), curr_slice,
                             int(out_start[2] - load_start[2]))


def flow_pairs(nz: int, z_stride: int, fixed_current: bool = False) -> list[tuple[int, int]]:
  """The (previous, current) section indices `EstimateFlow.process` correlates,
  in its order (processor/flow.py:213-229)."""
  if fixed_current:
    if z_stride > 0:
      return [(z, nz - 1) for z in range(0, nz - 1)]
    return [(z, 0) for z in range(1, nz)]
  rng = range(0, nz - z_stride) if z_stride > 0 else range(-z_stride, nz)
  return [(z, z + z_stride) for z in rng]


def estimate_flow(images, patch_size: int, stride: int, z_stride: int, *,
                  fixed_current: bool = False, masks=None,
                  mask_only_for_patch_selection: bool = False, selection_mask=None,
                  batch_size: int = 1024, calculator=None, device_output: bool = False):
  """The section-pair loop of `EstimateFlow.process` (processor/flow.py:184-231).

  images: [nz, Y, X] (uint8 or float32; NumPy, torch or DeviceArray), uploaded
  once for the whole stack; masks: optional [nz, Y, X] bool, True = excluded;
  selection_mask: optional host array [nz, gy, gx], indexed by the current
  section like the reference's.  Pairs are `flow_pairs(nz, z_stride,
  fixed_current)`.  Returns [4, n_pairs, gy, gx] float32 (the reference's
  transposed order, :245), assembled on the device; a DeviceArray with
  `device_output`.  Every plane is one `flow_field()` call.
  """
  import torch
  from . import _dev, flow_field as ff
  dev = _dev.device()
  img, _ = _dev.as_device_image(images, dev)
  if img.ndim != 3:
    raise ValueError('images must be [nz, y, x]')
  masks_d = _dev.as_device_mask(masks, dev)
  if masks_d is not None and tuple(masks_d.shape) != tuple(img.shape):
    raise ValueError('masks must have the shape of images')
  sel = None if selection_mask is None else np.asarray(selection_mask)
  pairs = flow_pairs(img.shape[0], z_stride, fixed_current)
  if not pairs:
    raise ValueError(f'no section pairs: {img.shape[0]} sections, z_stride {z_stride}')
  calc = calculator or ff.JAXMaskedXCorrWithStatsCalculator()
  planes = []
  for z_prev, z_curr in pairs:
    planes.append(calc.flow_field(
        img[z_prev], img[z_curr], patch_size, stride,
        None if masks_d is None else masks_d[z_prev],
        None if masks_d is None else masks_d[z_curr],
        mask_only_for_patch_selection=mask_only_for_patch_selection,
        selection_mask=None if sel is None else sel[z_curr],
        batch_size=batch_size, device_output=True).tensor)
  out = torch.stack(planes, dim=1)
  return _dev.DeviceArray(out) if device_output else out.cpu().numpy()


def select_patches(selection, batch_size: int, positions, counts, *, pre_counts=None,
                   pre_area: int = 1, post_counts=None, post_area: int = 1,
                   max_masked: float = 0.75) -> None:
  """`sfm_flow_select`: patch selection and ordered compaction in one launch.

  selection: uint8 device tensor [ny, nx] (rows may be strided); pre_counts /
  post_counts: optional int32 device tensors of `sfm_mask_patch_counts`, at
  least [ny, nx]; positions: int32 device tensor [capacity, 2]; counts: int32
  device tensor [2] that receives (n, n padded to whole batches).
  """
  from . import _abi, _dev
  if selection.ndim != 2 or selection.stride(1) != 1:
    raise ValueError('selection must be a 2-D plane with dense rows')
  d = _abi.SfmFlowSelectDesc()
  d.grid = (C.c_int32 * 2)(*selection.shape)
  d.batch_size = int(batch_size)
  d.capacity = positions.shape[0]
  d.selection = selection.data_ptr()
  d.selection_pitch = selection.stride(0) if selection.shape[0] > 1 else selection.shape[1]
  for side, plane, area in (('pre', pre_counts, pre_area), ('post', post_counts, post_area)):
    if plane is None:
      continue
    if plane.ndim != 2 or plane.stride(1) != 1:
      raise ValueError('count planes must be 2-D with dense rows')
    setattr(d, side + '_grid', (C.c_int32 * 2)(*plane.shape))
    setattr(d, side + '_counts', plane.data_ptr())
    setattr(d, side + '_pitch', plane.stride(0) if plane.shape[0] > 1 else plane.shape[1])
    setattr(d, side + '_area', int(area))
    setattr(d, side + '_max_masked', float(max_masked))
  d.positions = positions.data_ptr()
  d.counts = counts.data_ptr()
  d.stream = _dev.stream_ptr()
  _abi.check(_abi.load().sfm_flow_select(C.byref(d)))


def patch_starts(positions, total: int, patch_size, post_patch_size, step, pre_shape,
                 post_shape):
  """`sfm_flow_starts` for the first `total` rows of `positions`: the
  [2, total, 2] pre / post start coordinates `_run_batches_dev` takes."""
  import torch
  from . import _abi, _dev, flow_field as ff
  if positions.shape[0] < total or not positions.is_contiguous():
    raise ValueError('positions must be contiguous and hold `total` rows')
  starts = torch.empty((2, total, 2), dtype=torch.int32, device=positions.device)
  d = _abi.SfmFlowStartsDesc()
  d.ndim = 2
  d.n = total
  d.step = ff._i3(ff._pad3(step, 1))
  d.patch = ff._i3(ff._pad3(patch_size, 1))
  d.post_patch = ff._i3(ff._pad3(post_patch_size, 1))
  d.pre_shape = ff._i3(ff._pad3(pre_shape, 1))
  d.post_shape = ff._i3(ff._pad3(post_shape, 1))
  d.positions = positions.data_ptr()
  d.pre_starts = starts[0].data_ptr()
  d.post_starts = starts[1].data_ptr()
  d.stream = _dev.stream_ptr()
  _abi.check(_abi.load().sfm_flow_starts(C.byref(d)))
  return starts


def _clean_thresholds(min_peak_ratio, min_peak_sharpness, max_magnitude):
  """The doubles the device compares with, as `flow_utils.clean_flow` passes
  them: NumPy's comparison of a float32 array with the scalar, and a positive
  limit that float32 rounds to 0 still enables the magnitude test."""
  f = flow_utils._f32_threshold
  return (f(min_peak_ratio), f(min_peak_sharpness),
          max(f(max_magnitude), 5e-324) if max_magnitude > 0 else 0.0)


def missing_flow_update(field, out_planes, mask, attempts, filled_ptr: int, *,
                        min_peak_ratio: float, min_peak_sharpness: float,
                        max_magnitude: float, delta_z: int, max_attempts: int) -> None:
  """`sfm_missing_flow_update`: the accept / update step of one round
  (processor/flow.py:806-828) and the attempts cap of the next (:785).

  field: float32 device tensor [4, sy, sx], contiguous; out_planes: three
  float32 device planes [ny, nx], contiguous; mask: uint8 [ny, nx]; attempts:
  int32 [ny, nx]; filled_ptr: device address of this round's int64 counter.
  """
  from . import _abi, _dev
  if field.ndim != 3 or field.shape[0] != 4 or not field.is_contiguous():
    raise ValueError('field must be a contiguous [4, sy, sx] tensor')
  for t in tuple(out_planes) + (mask, attempts):
    if t.ndim != 2 or tuple(t.shape) != tuple(mask.shape) or not t.is_contiguous():
      raise ValueError('planes, mask and attempts must be contiguous and of one [ny, nx] shape')
  d = _abi.SfmMissingFlowDesc()
  d.shape = (C.c_int32 * 2)(*mask.shape)
  d.field_shape = (C.c_int32 * 2)(*field.shape[1:])
  d.field = field.data_ptr()
  d.out = (C.c_void_p * 3)(*(p.data_ptr() for p in out_planes))
  d.mask = mask.data_ptr()
  d.attempts = attempts.data_ptr()
  d.min_peak_ratio, d.min_peak_sharpness, d.max_magnitude = _clean_thresholds(
      min_peak_ratio, min_peak_sharpness, max_magnitude)
  d.delta_z = int(delta_z)
  d.max_attempts = int(max_attempts)
  d.filled = filled_ptr
  d.stream = _dev.stream_ptr()
  _abi.check(_abi.load().sfm_missing_flow_update(C.byref(d)))


@dataclasses.dataclass(frozen=True)
class CoarseFlow:
  """One of the lower-resolution flows of `reconcile_and_filter_flows`."""
  flow: Any                          # [c, z, y, x] over `box`
  box: Any                           # its read box: `.start` / `.size` or a (start, size) pair, xyz
  scale: float                       # base pixel size / this flow's pixel size, <= 1
  mag_scale: float | None = None     # divisor of the vectors; None: `scale`


_Box = collections.namedtuple('_Box', 'start size')


def _xyz_box(box) -> _Box:
  start, size = ((box.start, box.size) if hasattr(box, 'start') else box)
  return _Box(tuple(int(v) for v in np.asarray(start).ravel()),
              tuple(int(v) for v in np.asarray(size).ravel()))


def nearest_nodes(n: int, start: int, scale: float, q_start: int, q_n: int):
  """Along one axis, the coarse node that `RegularGridInterpolator(method=
  'nearest', bounds_error=False)` reads for the fine queries `q_start ..
  q_start + q_n - 1` when the coarse nodes lie at `(start + k) / scale`
  (processor/flow.py:447-461): the cell is found by bisection, the nearer end
  is taken and a query halfway goes to the lower index.  Returns (index [q_n]
  int64, outside [q_n] bool); `outside` marks the queries beyond the first or
  last coarse node, which the interpolator answers with NaN.  Host only.
  """
  grid = (np.arange(n) + start) / scale
  x = (np.arange(q_n) + q_start).astype(np.float64)
  if n == 1:
    return np.zeros(q_n, np.int64), x != grid[0]
  i = np.clip(np.searchsorted(grid, x, side='right') - 1, 0, n - 2)
  dist = (x - grid[i]) / (grid[i + 1] - grid[i])
  return np.where(dist <= .5, i, i + 1).astype(np.int64), (x < grid[0]) | (x > grid[-1])


def _clean_all_channels(flow, dev, min_peak_ratio, min_peak_sharpness, max_magnitude,
                        max_deviation):
  """`clean_flow` as the reference returns it: a 3-channel flow keeps its third
  channel, NaN where a vector was rejected (flow_utils.py:65-67, 77)."""
  import torch
  from . import _dev
  clean = flow_utils.clean_flow(flow, min_peak_ratio, min_peak_sharpness, max_magnitude,
                                max_deviation).tensor
  if tuple(flow.shape)[0] != 3:
    return clean
  raw = _dev.as_device_f32(flow, dev, copy=False)
  # rejected: NaN now and not before (a vector with a NaN component fails no test)
  bad = torch.isnan(clean[0]) & ~torch.isnan(raw[0])
  third = torch.where(bad, torch.full_like(raw[2], float('nan')), raw[2])
  return torch.cat([clean, third[None]])


def reconcile_and_filter_flows(flow, box, coarse=(), *, min_peak_ratio: float,
                               min_peak_sharpness: float, max_magnitude: float,
                               max_deviation: float, max_gradient: float,
                               min_patch_size: int, multi_section: bool = False,
                               base_delta_z: int = 0, mask=None):
  """The compute of `ReconcileAndFilterFlows.process` (processor/flow.py:386-493)
  on resident data: cleans a base flow and any number of coarser flows,
  upsamples the coarser ones onto the base lattice and reconciles them.

  flow: the base flow [c, z, y, x] (c = 2 .. 4) over `box` (`.start` / `.size`
  or a (start, size) pair, xyz; only x and y are used).  coarse: `CoarseFlow`s
  in order of decreasing preference, each with its read box in its own
  coordinates, its `scale` <= 1 and an optional `mag_scale`.  mask: optional
  bool, [z, y, x] or broadcastable to it, True = excluded.  Arrays are NumPy,
  torch or DeviceArray; none is modified.

  1. every flow goes through `clean_flow` with the four clean thresholds;
  2. the base flow, and a coarse flow of scale 1, gets the `multi_section`
     rule (:433-439): a flow without a third channel gets one that holds
     `base_delta_z` where channel 0 is finite and NaN elsewhere;
  3. a coarser flow is upsampled: all its z slices go through one
     `map_utils.resample_map(flow[:2], read box, box, 1 / scale, 1)` call and
     are divided by `mag_scale`; a fine node is NaN where its nearest coarse
     node (`nearest_nodes`) is NaN in channel 0 or the node lies outside the
     coarse grid; with `multi_section` channel 2 is the nearest coarse node's;
     a third channel of the base flow without `multi_section` is 0, as in the
     reference; `mask` is applied to the upsampled flows only;
  4. `flow_utils.reconcile_flows` with `max_gradient`, `max_deviation` and
     `min_patch_size`.

  The flows stay on the device throughout; the host waits for it once per
  coarser flow, where `resample_map` reads the per-slice status of its
  triangulation (a refused slice raises SofimaAmdError there).

  Returns a [2 or 3, z, y, x] float32 DeviceArray.  The upsampled values carry
  `resample_map`'s contract: equal to the reference's where all Delaunay
  triangulations of the valid coarse nodes agree, one admissible value
  elsewhere.
  """
  import torch
  from . import _dev, map_utils
  dev = _dev.device()
  box = _xyz_box(box)
  thresholds = (min_peak_ratio, min_peak_sharpness, max_magnitude, max_deviation)

  def expand(f):      # the multi_section rule
    if not multi_section or f.shape[0] == 3:
      return f
    third = torch.full_like(f[0], float('nan'))
    third[torch.isfinite(f[0])] = float(base_delta_z)
    return torch.cat([f[:2], third[None]])

  base = expand(_clean_all_channels(flow, dev, *thresholds))
  nz, ny, nx = (int(v) for v in base.shape[1:])
  if (nx, ny) != box.size[:2]:
    raise ValueError(f'box size {box.size} mismatch with the base flow {tuple(base.shape)}')
  mask_d = _dev.as_device_mask(mask, dev)
  if mask_d is not None:
    mask_d = torch.broadcast_to(mask_d.bool(), (nz, ny, nx))
  channels = 3 if multi_section else 2      # the reference's num_channels()
  flows = [base]
  for k, c in enumerate(coarse):
    if not c.scale <= 1.0:
      raise ValueError(f'coarse flow {k}: scale {c.scale} > 1')
    f = _clean_all_channels(c.flow, dev, *thresholds)
    if c.scale == 1:
      f = expand(f)
      if tuple(f.shape) != tuple(base.shape):
        raise ValueError(f'coarse flow {k} of scale 1 must have the base shape')
      flows.append(f)
      continue
    read_box = _xyz_box(c.box)
    if f.shape[1] != nz or (int(f.shape[3]), int(f.shape[2])) != read_box.size[:2]:
      raise ValueError(f'coarse flow {k}: shape {tuple(f.shape)} against read box '
                       f'{read_box.size} and {nz} sections')
    if f.shape[0] < channels:
      raise ValueError(f'coarse flow {k} has no channel 2 for a multi-section result')
    mag_scale = c.scale if c.mag_scale is None else c.mag_scale
    hires = torch.zeros_like(base)
    up = map_utils.resample_map(_dev.DeviceArray(f[:2].contiguous()), read_box, box,
                                1 / c.scale, 1).tensor
    iy, out_y = nearest_nodes(read_box.size[1], read_box.start[1], c.scale, box.start[1], ny)
    ix, out_x = nearest_nodes(read_box.size[0], read_box.start[0], c.scale, box.start[0], nx)
    near = f[:, :, torch.from_numpy(iy).to(dev)][:, :, :, torch.from_numpy(ix).to(dev)]
    outside = torch.from_numpy(out_y[:, None] | out_x[None, :]).to(dev)
    nan = torch.full((), float('nan'), dtype=torch.float32, device=dev)
    invalid = torch.isnan(near[0]) | outside
    # (a 0-dim device divisor: a true float32 division, as NumPy's)
    hires[:2] = torch.where(
        invalid, nan, up / torch.tensor(mag_scale, dtype=torch.float32, device=dev))
    for ch in range(2, channels):
      hires[ch] = torch.where(outside, nan, near[ch])
    if mask_d is not None:
      hires = torch.where(mask_d, nan, hires)
    flows.append(hires)
  return flow_utils.reconcile_flows(flows, max_gradient, max_deviation, min_patch_size)


def search_deltas(delta_z: int, max_delta_z: int) -> list[int]:
  """The look-backs tried after `delta_z`, nearest first (processor/flow.py:696-705)."""
  if delta_z > 0:
    return list(range(delta_z + 1, max_delta_z + 1))
  return list(range(delta_z - 1, max_delta_z - 1, -1))


def estimate_missing_flow(flow, images, *, patch_size: int, stride: int, delta_z: int,
                          max_delta_z: int, max_attempts: int, search_radius: int,
                          min_peak_ratio: float, min_peak_sharpness: float,
                          max_magnitude: float, curr_slice=None, z0: int | None = None,
                          masks=None, mask_only_for_patch_selection: bool = False,
                          selection_mask=None, batch_size: int = 1024, calculator=None,
                          device_output: bool = False) -> tuple[Any, np.ndarray]:
  """Fills the NaN vectors of a single-look-back flow from earlier sections:
  the loop of `EstimateMissingFlow.process` (processor/flow.py:666-828).

  flow: [2, nz, ny, nx], already cut to the output box
  (`missing_flow_geometry().flow_slice`).  images: [nzi, Y, X], uint8 or
  float32, the loaded stack; `z0` is the index in it of the section of
  flow[:, 0] (default `max_delta_z` for `delta_z > 0`, else 0) and `curr_slice`
  the (y, x) slices of the current image inside a section (default: starting
  at (search_radius, search_radius), ((n - 1) * stride + patch_size) long per
  axis).  masks: optional [nzi, Y, X] bool, True = excluded.  selection_mask:
  optional [nz, ny, nx], nodes that may be estimated.  All of them NumPy,
  torch or DeviceArray; none is modified.

  Returns (flow3, filled).  flow3 is [3, nz, ny, nx] float32 (a DeviceArray
  with `device_output`): the input vectors, the vectors filled in, and in
  channel 2 the look-back of every node -- `delta_z` where nothing was filled,
  on nodes that stay NaN too.  The reference keeps this array in float64; every
  value it holds is a float32 vector component or a small integer, so the
  float32 result is the same numbers.  filled is int64 [nz, n_search_deltas]:
  the nodes filled per section and look-back (the reference's
  `sections-filled-delta*` counters), accumulated on the device and read once.

  As in the reference: a section with no NaN in channel 0 is left alone; a
  current section whose mask is all True is skipped; a previous section whose
  mask is all True skips that look-back; a previous index outside the stack
  ends the section's look-backs.  Every round is the `flow_field()` call of
  :792-803 (previous section whole, current section cropped, `patch_size + 2 *
  search_radius` against `post_patch_size = patch_size`, the remaining nodes
  as selection mask, `max_masked` at its default), accepted by `clean_flow`
  with `max_deviation = 0`.  `attempts` counts every node whose raw x
  component came back finite, and the cap `attempts <= max_attempts` is
  evaluated before each round, so a node gets `max_attempts + 1` counted
  attempts (the reference's off-by-one, kept); with `max_attempts < 0` nothing
  is estimated.  A round with no selected patch launches nothing, which gives
  what the reference's `break` / empty call gives.

  A `curr_slice` whose flow grid is not (ny, nx), or a patch / search patch
  that is not a multiple of `stride` (:571-582), raises ValueError.
  """
  import torch
  from . import _dev, flow_field as ff
  search_patch_size = _check_patch(patch_size, stride, search_radius)
  dev = _dev.device()
  flow_d = _dev.as_device_f32(flow, dev, copy=False)
  if flow_d.ndim != 4 or flow_d.shape[0] != 2:
    raise ValueError('flow must be [2, nz, ny, nx]')
  nz, ny, nx = (int(v) for v in flow_d.shape[1:])
  img, dtype = _dev.as_device_image(images, dev)
  if img.ndim != 3:
    raise ValueError('images must be [nzi, y, x]')
  nzi = int(img.shape[0])
  if curr_slice is None:
    curr_slice = tuple(slice(search_radius, search_radius + (n - 1) * stride + patch_size)
                       for n in (ny, nx))
  ys, xs = curr_slice
  curr_shape = tuple(int(v) for v in img[0, ys, xs].shape)
  grid = tuple((s - (patch_size - stride)) // stride for s in curr_shape)
  if grid != (ny, nx):
    raise ValueError(f'curr_slice gives a flow grid of {grid}, the flow has {(ny, nx)}')
  if z0 is None:
    z0 = max_delta_z if delta_z > 0 else 0
  masks_d = _dev.as_device_mask(masks, dev)
  if masks_d is not None and tuple(masks_d.shape) != tuple(img.shape):
    raise ValueError('masks must have the shape of images')
  sel_d = _dev.as_device_mask(selection_mask, dev)
  if sel_d is not None and tuple(sel_d.shape) != (nz, ny, nx):
    raise ValueError('selection_mask must be [nz, ny, nx]')
  deltas = search_deltas(delta_z, max_delta_z)

  out = torch.empty((3, nz, ny, nx), dtype=torch.float32, device=dev)
  out[:2] = flow_d
  out[2] = float(delta_z)
  filled = torch.zeros((nz, len(deltas)), dtype=torch.int64, device=dev)

  # what the host decides with, read once for the stack: sections that hold a
  # NaN, and the all-True tests of the masks (:743, :754, :780)
  tests = [torch.isnan(flow_d[0]).flatten(1).any(1)]
  if masks_d is not None:
    tests += [masks_d.flatten(1).all(1), masks_d[:, ys, xs].flatten(1).all(1)]
  tests = torch.cat(tests).cpu().numpy().astype(bool)
  has_nan, prev_all, curr_all = tests[:nz], tests[nz:nz + nzi], tests[nz + nzi:]

  calc = calculator or ff.JAXMaskedXCorrWithStatsCalculator()
  patch, search_patch, step = (patch_size,) * 2, (search_patch_size,) * 2, (stride,) * 2
  capacity = (ny * nx + batch_size - 1) // batch_size * batch_size
  positions = torch.empty((capacity, 2), dtype=torch.int32, device=dev)
  counts = torch.empty((2,), dtype=torch.int32, device=dev)
  pre_counts = {}      # section index -> masked pixels per search patch, reused across rounds
  for z in range(nz):
    if not has_nan[z] or max_attempts < 0 or not deltas:
      continue
    ci = z0 + z
    if not 0 <= ci < nzi:
      raise ValueError(f'section {z} of the flow is section {ci} of a stack of {nzi}')
    if masks_d is not None and curr_all[ci]:
      continue
    mask = (~torch.isfinite(out[0, z])).to(torch.uint8)
    if sel_d is not None:
      mask &= sel_d[z]
    attempts = torch.zeros((ny, nx), dtype=torch.int32, device=dev)
    curr = curr_mask = post_counts = None
    for k, dz in enumerate(deltas):
      pi = ci - dz
      if pi < 0 or pi >= nzi:
        break
      if masks_d is not None and prev_all[pi]:
        continue
      if curr is None:
        curr = img[ci, ys, xs].contiguous()
        if masks_d is not None:
          curr_mask = masks_d[ci, ys, xs].contiguous()
          post_counts = ff._masked_counts(curr_mask, patch, step, on_device=True)
      if masks_d is not None and pi not in pre_counts:
        pre_counts[pi] = ff._masked_counts(masks_d[pi], search_patch, step, on_device=True)
      select_patches(mask, batch_size, positions, counts,
                     pre_counts=pre_counts.get(pi), pre_area=search_patch_size ** 2,
                     post_counts=post_counts, post_area=patch_size ** 2)
      n = int(counts[0].item())            # the one host read of a round: it sizes the launches
      if n == 0:
        if masks_d is None:
          break                            # nothing left to estimate in this section
        continue
      total = (n + batch_size - 1) // batch_size * batch_size
      res = ff._Resident.of_device(img[pi], curr,
                                   None if masks_d is None else masks_d[pi], curr_mask,
                                   dtype, dev)
      plan = dict(out_shape=[ny, nx], n=n, positions=positions, tg=None, po=None,
                  starts=patch_starts(positions, total, search_patch, patch, step,
                                      tuple(img.shape[1:]), curr_shape))
      field = calc.field_from_plan(res, plan, search_patch, patch, batch_size,
                                   mask_only_for_patch_selection)
      missing_flow_update(field, (out[0, z], out[1, z], out[2, z]), mask, attempts,
                          filled.data_ptr() + (z * len(deltas) + k) * 8,
                          min_peak_ratio=min_peak_ratio,
                          min_peak_sharpness=min_peak_sharpness,
                          max_magnitude=max_magnitude, delta_z=dz, max_attempts=max_attempts)
  filled_h = filled.cpu().numpy()
  return (_dev.DeviceArray(out) if device_output else out.cpu().numpy()), filled_h
