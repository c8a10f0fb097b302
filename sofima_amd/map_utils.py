"""Coordinate-map composition, inversion and geometry helpers on MI355X.

Drop-ins for `map_utils.compose_maps_fast` of the reference
(map_utils.py:616-734), `map_utils.mask_irregular` (:737-786), the 2-D
branch of `map_utils.invert_map` (:392-463) and the helpers that the
reference's renderers call around them: `to_absolute` / `to_relative`
(:150-224), `outer_box` (:307-342), `inner_box` (:345-389, maps without NaN),
`make_affine_map` (:789-811), the nearest-node branch of `fill_missing`
(:227-304 with `interpolate_first=False`), the linear `resample_map`
(:490-546) and `compose_maps` (:549-611).  The helpers are one pass over
memory each and take and return `DeviceArray`s, so a map produced by
`invert_map` or `compose_maps_fast` is shifted or measured without a host
round trip.  `invert_map` triangulates the deformed positions, so its Delaunay
triangulation is unique and the device result has a parity contract.
`resample_map`, `compose_maps` and the `interpolate_first=True` branch of
`fill_missing` triangulate the regular lattice, where every quad is
co-circular and Qhull picks the diagonals arbitrarily.  `resample_map` and
`compose_maps` run on the engine of `invert_map` under the contract that does
exist there: the interpolant of one verified, deterministic Delaunay
triangulation, equal to the reference wherever all Delaunay triangulations
agree and one of the admissible values elsewhere (see their docstrings);
`compose_maps` asks at arbitrary points, which the engine locates in the
triangulation with exact tests.  The `interpolate_first=True` branch of
`fill_missing` stays host geometry and out of scope (and with that branch,
`inner_box` of a map that holds NaN).
`fill_missing(extrapolate=True, interpolate_first=False)` never touches Qhull:
every invalid node takes the nearest valid node, an exact integer feature
transform on the device with a stated tie rule.
"""
from __future__ import annotations

import collections.abc
import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _abi
from . import _dev
from ._dev import DeviceArray


def _as_vec(value, dim):
  if not isinstance(value, collections.abc.Sequence):
    return (value,) * dim
  assert len(value) == dim, f'Dimension mismatch: {value=} vs {dim=}'
  return tuple(value)


def compose_maps_fast(map1, start1: Sequence[float], stride1, map2,
                      start2: Sequence[float], stride2,
                      mode: str = 'nearest') -> DeviceArray:
  """Composes two coordinate maps: map2(map1(z, y, x)) over map1's area.

  Same contract as the reference: maps are [2 or 3, z, y, x] in relative
  format, `start*` are [z]yx origins, `stride*` scalars or [z]yx tuples; `mode`
  is 'nearest' or 'constant' (out-of-range samples are NaN, like the
  reference's cval).  Invalid (NaN) entries are not interpolated.
  """
  assert np.shape(map1)[0] == np.shape(map2)[0]
  dim = np.shape(map1)[0]
  if mode not in ('nearest', 'constant'):
    raise NotImplementedError(mode)
  stride1 = _as_vec(stride1, dim)
  stride2 = _as_vec(stride2, dim)
  dev = _dev.device()
  m1 = _dev.as_device_f32(map1, dev, copy=False)
  m2 = _dev.as_device_f32(map2, dev, copy=False)
  if m1.ndim != 4 or m2.ndim != 4:
    raise ValueError('maps must be [2 or 3, z, y, x]')
  d = _abi.SfmComposeDesc()
  d.ncomp = dim
  d.mode = 0 if mode == 'nearest' else 1
  d.shape1 = (C.c_int32 * 3)(*m1.shape[1:])
  d.shape2 = (C.c_int32 * 3)(*m2.shape[1:])

  def zyx(v, fill):
    v = [float(a) for a in np.asarray(v).ravel()][-dim:]
    return (C.c_float * 3)(*([fill] * (3 - dim) + v))

  d.start1 = zyx(start1, 0.0)
  d.start2 = zyx(start2, 0.0)
  d.stride1 = zyx(stride1, 1.0)
  d.stride2 = zyx(stride2, 1.0)
  d.map1 = m1.data_ptr()
  d.map2 = m2.data_ptr()
  d.stream = _dev.stream_ptr()
  out = torch.empty_like(m1)
  _abi.check(_abi.load().sfm_compose_maps(C.byref(d), out.data_ptr()))
  return DeviceArray(out)


def _irregular_desc(shape, stride_x, stride_y, frac, max_frac, dilation_iters):
  d = _abi.SfmMaskIrregularDesc()
  d.shape = (C.c_int32 * 2)(int(shape[1]), int(shape[2]))
  d.dilation_iters = int(dilation_iters)
  frac, max_frac = float(frac), float(max_frac)
  d.stride = (C.c_double * 2)(stride_x, stride_y)
  d.min_dist = (C.c_double * 2)(frac * stride_x, frac * stride_y)
  d.max_dist = (C.c_double * 2)(max_frac * stride_x, max_frac * stride_y)
  d.stream = _dev.stream_ptr()
  return d


def mask_irregular(coord_map, stride: Sequence[float], frac: float,
                   max_frac: float | None = None,
                   dilation_iters: int = 1) -> np.ndarray:
  """Masks stretched / folded parts of a [2, y, x] relative coordinate map.

  Same contract as the reference (map_utils.py:737-786): masked entries are
  replaced with NaN IN PLACE (NumPy arrays are written back; torch tensors /
  DeviceArrays are modified on the device) and the bool mask [y, x] is
  returned.  `stride` is (x, y).

  Arithmetic: the neighbour differences are taken in float32; the stride is
  added and the sums are compared with `frac * stride` / `max_frac * stride`
  in double, the limits being formed on the host as Python floats.  That is
  what the reference computes for a float32 map under NumPy >= 2 (NEP 50: the
  float64 stride scalar promotes the sum), and it is the high-precision
  answer.  NumPy 1.x's value-based casting would have added the stride in
  float32 instead.  `stride` is read as float64 whatever its dtype.  A
  float64 map is still narrowed to float32 first: the result equals the
  reference's when its values are float32-representable and their differences
  exact in float32, and can differ from it by the narrowing otherwise.
  """
  shape = np.shape(coord_map)
  assert len(shape) == 3
  assert shape[0] == 2
  if max_frac is None:
    max_frac = 2 - frac
  stride_x, stride_y = (float(v) for v in np.asarray(stride).ravel())
  dev = _dev.device()
  host = coord_map if isinstance(coord_map, np.ndarray) else None
  m = _dev.as_device_f32(coord_map, dev, copy=host is not None)
  d = _irregular_desc(shape, stride_x, stride_y, frac, max_frac, dilation_iters)
  bad = torch.empty(tuple(shape[1:]), dtype=torch.uint8, device=dev)
  _abi.check(_abi.load().sfm_mask_irregular(C.byref(d), m.data_ptr(), bad.data_ptr()))
  bad_h = bad.cpu().numpy().astype(bool)
  if host is not None:
    # in-place contract: the masked map computed on the device is copied back
    # (unmasked entries round-trip through float32 unchanged for float32 input)
    if host.dtype == np.float32:
      host[...] = m.cpu().numpy()
    else:
      host[:, bad_h] = np.nan
  return bad_h


def mask_irregular_f64(coord_map, stride: Sequence[float], frac: float,
                       max_frac: float | None = None,
                       dilation_iters: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
  """`mask_irregular` for a float64 [2, y, x] map that lives on the device (a
  contiguous torch tensor or DeviceArray), without narrowing: the neighbour
  differences are taken in double, as the reference does for a float64 map
  (map_utils.py:769-775).  The map is masked in place.  Nothing comes to the
  host: returns (mask [y, x] uint8, n_valid), both device tensors; n_valid is
  the number of nodes that keep a component that is not NaN, so
  `n_valid == 0` is the reference's `np.all(np.isnan(coord_map))`.
  """
  m = coord_map.tensor if isinstance(coord_map, DeviceArray) else coord_map
  if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float64 and
          m.is_contiguous() and m.ndim == 3 and m.shape[0] == 2):
    raise ValueError('mask_irregular_f64 needs a contiguous float64 [2, y, x] device tensor')
  if max_frac is None:
    max_frac = 2 - frac
  stride_x, stride_y = (float(v) for v in np.asarray(stride).ravel())
  d = _irregular_desc(m.shape, stride_x, stride_y, frac, max_frac, dilation_iters)
  bad = torch.empty(tuple(m.shape[1:]), dtype=torch.uint8, device=m.device)
  n_valid = torch.empty((), dtype=torch.int32, device=m.device)
  _abi.check(_abi.load().sfm_mask_irregular_f64(C.byref(d), m.data_ptr(), bad.data_ptr(),
                                                n_valid.data_ptr()))
  return bad, n_valid


# reasons of a refused slice (SFM_INVMAP_* in include/sofima_amd.h)
_INVMAP_REASONS = (
    (1, 'folded or degenerate quad'),
    (2, 'edge not locally Delaunay'),
    (4, 'more than 7936 boundary nodes'),
    (8, 'completion tables overflowed'),
    (16, 'overlapping triangles'),
    (32, 'border edge off the convex hull'),
    (64, 'triangles do not tile the convex hull'),
    (128, 'valid node left out of the triangulation'),
)


def _box_xy(box, name):
  start = [int(v) for v in np.asarray(box.start).ravel()]
  size = [int(v) for v in np.asarray(box.size).ravel()]
  if len(start) < 2 or len(size) < 2:
    raise ValueError(f'{name} needs at least x and y in start and size')
  return start, size


def invert_map(coord_map, src_box, dst_box, stride) -> DeviceArray:
  """Inverts a [2, z, y, x] coordinate map: (x, y) -> (u, v) becomes (u, v) -> (x, y).

  Same contract as the 2-D branch of the reference: `coord_map` is in relative
  format (NumPy, torch or DeviceArray, float32 or float64; never modified),
  `src_box` / `dst_box` have `.start` / `.size` in xyz order (only x and y are
  used), `stride` is a scalar or a (y, x) pair.  Per z slice the valid nodes
  (both channels finite) are triangulated at their absolute positions
  (Delaunay) and the source lattice coordinates are interpolated linearly at
  the dst lattice; queries outside the convex hull and slices with fewer than
  3 valid or only collinear nodes are NaN (a slice that has a quad of four
  valid nodes on one line or at one point is refused as degenerate instead).
  A dst box of size 0 on an axis gives an empty result.  Computed in float64
  on the device; returns a float64 [2, z, dst y, dst x] DeviceArray in
  relative format.

  The triangulation is verified on the device (one host sync reads the
  per-slice status).  A slice that cannot be answered exactly -- folded, more
  than 7936 boundary nodes, or a lattice part that is not Delaunay -- raises
  SofimaAmdError naming the first such slice and its reason, the refused
  slices, and the reason of each that differs; it is never answered wrongly.
  """
  shape = _map_shape(coord_map)
  if len(shape) != 4:
    raise ValueError(f'coord_map must be [2, z, y, x], got shape {shape}')
  dim = shape[0]
  if dim == 3:
    raise NotImplementedError(
        'invert_map of 3-D maps (tetrahedra) is not on the device; it is a '
        'follow-up of the 2-D inversion')
  if dim != 2:
    raise NotImplementedError(f'invert_map: {dim} channels')
  sy, sx = (float(v) for v in _as_vec(stride, dim))
  if not (np.isfinite(sx) and np.isfinite(sy) and sx > 0 and sy > 0):
    raise ValueError(f'stride must be finite and positive, got {stride}')
  src_start, dst_start, dst_size = _engine_boxes(shape, src_box, dst_box)
  dev = _dev.device()
  m = _engine_map(coord_map, dev, keep_f32=False)
  d = _abi.SfmInvertMapDesc()
  d.src_start = _i32_pair('src_box.start - dst_box.start', src_start[1] - dst_start[1],
                          src_start[0] - dst_start[0])
  d.stride = (C.c_double * 2)(sy, sx)
  lib = _abi.load()
  out, status = _engine_run(d, lib.sfm_invert_map_workspace_bytes, lib.sfm_invert_map, m,
                            dst_size, dev)
  _raise_refused('invert_map', status)
  return DeviceArray(out)


# -- what invert_map and resample_map share: one engine, one descriptor tail --


def _map_shape(coord_map):
  if isinstance(coord_map, (torch.Tensor, DeviceArray)):
    return tuple(coord_map.shape)
  return tuple(int(v) for v in np.shape(coord_map))


def _engine_boxes(shape, src_box, dst_box):
  """(src start xy.., dst start xy.., dst size xy..) of the boxes of a
  [2, z, y, x] map, checked against its shape."""
  src_start, src_size = _box_xy(src_box, 'src_box')
  dst_start, dst_size = _box_xy(dst_box, 'dst_box')
  if (shape[3], shape[2]) != (src_size[0], src_size[1]):
    raise ValueError(f'box shape ({src_size}) mismatch with coord map ({shape})')
  if min(shape[1:]) < 1 or dst_size[0] < 0 or dst_size[1] < 0:
    raise ValueError(f'empty map or box: {shape}, {dst_size}')
  return src_start, dst_start, dst_size


def _engine_map(coord_map, dev, keep_f32):
  """The map as a contiguous device tensor: float64, or with `keep_f32` its own
  float32 / float64 (a resident contiguous tensor of that type is not copied)."""
  if isinstance(coord_map, DeviceArray):
    coord_map = coord_map.tensor
  if isinstance(coord_map, torch.Tensor):
    f64 = not keep_f32 or coord_map.dtype == torch.float64
    return coord_map.to(device=dev, dtype=torch.float64 if f64 else torch.float32).contiguous()
  host = np.asarray(coord_map)
  f64 = not keep_f32 or host.dtype == np.float64
  return _dev.upload(np.ascontiguousarray(host, dtype=np.float64 if f64 else np.float32), dev)


def _i32_pair(name, y, x):
  """A (y, x) pair of the descriptor; ctypes would truncate silently."""
  for v in (y, x):
    if not -2**31 <= v < 2**31:
      raise ValueError(f'{name} {v} does not fit 32 bits')
  return (C.c_int32 * 2)(y, x)


def _engine_run(d, workspace_bytes, run, m, dst_size, dev):
  """Fills the part of the descriptor the two entry points share (shapes, map,
  status, workspace, stream) and launches; returns (out, status [z] int32) of
  the map's dtype, both device tensors, without reading the status."""
  nz = int(m.shape[1])
  d.shape = (C.c_int32 * 3)(*m.shape[1:])
  d.dst_shape = (C.c_int32 * 2)(dst_size[1], dst_size[0])
  d.coord_map = m.data_ptr()
  status = torch.empty(nz, dtype=torch.int32, device=dev)
  d.status = status.data_ptr()
  ws = _dev.workspace(workspace_bytes(C.byref(d)), dev)
  d.workspace = ws.data_ptr()
  d.workspace_bytes = ws.numel()
  d.stream = _dev.stream_ptr()
  out = torch.empty((2, nz, dst_size[1], dst_size[0]), dtype=m.dtype, device=dev)
  _abi.check(run(C.byref(d), out.data_ptr()))
  return out, status


def _raise_refused(name, status):
  """Reads the per-slice status of the triangulation engine (the one host sync
  of `invert_map` / `resample_map` / `compose_maps`) and raises for refused
  slices."""
  st = status.cpu().numpy()
  bad = np.flatnonzero(st)
  if bad.size:
    def why(k):
      return ', '.join(r for bit, r in _INVMAP_REASONS if st[k] & bit)

    z = int(bad[0])
    more = ''
    if bad.size > 1:
      # the listed slices that were refused for another reason than the first
      other = ''.join(f'; slice {int(k)}: {why(k)}' for k in bad[1:8] if st[k] != st[z])
      more = f' ({bad.size} slices refused: {bad.tolist()[:8]}{other})'
    raise _abi.SofimaAmdError(f'{name}: slice {z} refused: {why(z)}{more}')


def resample_map(coord_map, src_box, dst_box, src_stride: float, dst_stride: float,
                 method='linear') -> DeviceArray:
  """Resamples a [2, z, y, x] coordinate map (or flow) onto another lattice.

  Same signature and box convention as the reference (map_utils.py:490-546):
  `src_box` / `dst_box` have `.start` / `.size` in xyz order (only x and y are
  used), node (i, j) of the map lies at ((j + src start x) * src_stride,
  (i + src start y) * src_stride) and the result is sampled at
  ((u + dst start x) * dst_stride, (w + dst start y) * dst_stride).  Per z
  slice the nodes whose channel 0 is finite are triangulated (Delaunay) and
  both channels are interpolated linearly in float64; queries outside the
  convex hull and slices with fewer than 3 valid or only collinear nodes are
  NaN, and a NaN in channel 1 of a valid node propagates.  `coord_map` is a
  NumPy array, a CUDA tensor or a DeviceArray, float32 or float64; a resident
  contiguous input is read where it lies and never modified.  Returns a
  [2, z, dst y, dst x] DeviceArray of the input's dtype; an empty dst box gives
  an empty result.

  Contract.  The valid nodes lie on a lattice, where Delaunay triangulations
  are not unique (every full quad is co-circular) and Qhull's choice is
  arbitrary.  The device interpolates over one verified, deterministic
  Delaunay triangulation (a full quad is split from (i, j + 1) to (i + 1, j)):
  the result equals the reference wherever all Delaunay triangulations agree
  (nodes, cell edges, affine data, ...) and is the interpolant over some
  Delaunay triangle that contains the query everywhere else.

  Only `method='linear'` is built: 'nearest' is a k-d tree with arbitrary ties
  on a lattice and 'cubic' is Clough-Tocher; both raise NotImplementedError.
  A slice with more than 7936 boundary nodes raises SofimaAmdError naming the
  slice and the reason, as in `invert_map`; it is never answered wrongly.
  """
  if method != 'linear':
    raise NotImplementedError(
        f"resample_map: method {method!r} is not on the device (only 'linear')")
  out, status = _resample_launch(coord_map, src_box, dst_box, src_stride, dst_stride)
  _raise_refused('resample_map', status)
  return DeviceArray(out)


def _resample_launch(coord_map, src_box, dst_box, src_stride, dst_stride):
  """`resample_map` up to the status read: (out, status [z] int32), both device
  tensors; a slice with a non-zero status holds nothing to be used."""
  shape = _map_shape(coord_map)
  if len(shape) != 4 or shape[0] != 2:
    raise ValueError(f'coord_map must be [2, z, y, x], got shape {shape}')
  src_stride, dst_stride = float(src_stride), float(dst_stride)
  for s in (src_stride, dst_stride):
    if not (np.isfinite(s) and s > 0):
      raise ValueError(f'strides must be finite and positive, got {src_stride}, {dst_stride}')
  src_start, dst_start, dst_size = _engine_boxes(shape, src_box, dst_box)
  dev = _dev.device()
  m = _engine_map(coord_map, dev, keep_f32=True)
  d = _abi.SfmResampleMapDesc()
  d.src_start = _i32_pair('src_box.start', src_start[1], src_start[0])
  d.dst_start = _i32_pair('dst_box.start', dst_start[1], dst_start[0])
  d.src_stride = src_stride
  d.dst_stride = dst_stride
  d.f64 = int(m.dtype == torch.float64)
  lib = _abi.load()
  return _engine_run(d, lib.sfm_resample_map_workspace_bytes, lib.sfm_resample_map, m,
                     dst_size, dev)


def compose_maps(map1, box1, stride1: float, map2, box2, stride2: float) -> DeviceArray:
  """Composes two [2, z, y, x] coordinate maps: map2(map1(x, y)) over map1's nodes.

  Same signature and box convention as the reference (map_utils.py:549-611):
  both maps are in relative format, `box1` / `box2` have `.start` / `.size` in
  xyz order (only x and y are used) and must agree with the maps.  Per z slice
  the nodes of map2 where both channels of its absolute form are finite are
  triangulated (Delaunay) at their lattice positions ((j + box2 start x) *
  stride2, (i + box2 start y) * stride2), and map2's absolute form is
  interpolated linearly in float64 at the absolute positions of map1's nodes;
  the result is rounded to map1's dtype and made relative in it, as
  `to_relative` does.  A node of map1 with NaN or inf in either channel is NaN
  in both outputs, so are queries outside the convex hull of map2's valid
  nodes and slices where map2 has fewer than 3 valid or only collinear nodes;
  invalid nodes of map2 inside the hull are interpolated over.  The maps are
  NumPy arrays, CUDA tensors or DeviceArrays, float32 or float64 in any
  pairing; resident contiguous inputs are read where they lie and never
  modified.  Returns a DeviceArray of map1's shape and dtype.

  Contract (that of `resample_map`, carried to arbitrary queries).  The nodes
  of map2 lie on a lattice, where Delaunay triangulations are not unique and
  Qhull's choice is arbitrary.  The device interpolates over one verified,
  deterministic Delaunay triangulation (a full quad is split from (i, j + 1) to
  (i + 1, j); a query on a shared edge or vertex is answered by the
  lowest-keyed triangle that contains it): the result equals the reference
  wherever all Delaunay triangulations agree (an affine map2, holes included)
  and is the interpolant over some Delaunay triangle that contains the query
  everywhere else.

  A slice of map2 with more than 7936 boundary nodes (valid nodes that are not
  interior vertices of the full-quad lattice: a checkerboard of holes, not a
  map with blob holes) raises SofimaAmdError naming the slice and the reason,
  as in `invert_map`; it is never answered wrongly.  At most 2^21 nodes per
  slice of map2.
  """
  if _map_shape(map1)[1:2] != _map_shape(map2)[1:2]:
    raise ValueError(f'z mismatch: map1 {_map_shape(map1)}, map2 {_map_shape(map2)}')
  out, status = _compose_launch(map1, box1, stride1, map2, box2, stride2)
  _raise_refused('compose_maps', status)
  return DeviceArray(out)


def _compose_launch(map1, box1, stride1, map2, box2, stride2, scale2=None):
  """`compose_maps` up to the status read: (out, status [z of map2] int32),
  both device tensors.  Beyond the public call, map2 may have one z slice that
  serves every slice of map1 (triangulated once), and `scale2` (a float64
  device vector [z of map1]) multiplies map2's relative values in map2's
  dtype, the reference's `offset * scale`."""
  shape1, shape2 = _map_shape(map1), _map_shape(map2)
  for name, shape in (('map1', shape1), ('map2', shape2)):
    if len(shape) != 4 or shape[0] != 2:
      raise ValueError(f'{name} must be [2, z, y, x], got shape {shape}')
    if min(shape[1:]) < 1:
      raise ValueError(f'empty {name}: {shape}')
  if shape2[1] not in (1, shape1[1]):
    raise ValueError(f'map2 has {shape2[1]} z slices, map1 {shape1[1]}')
  stride1, stride2 = float(stride1), float(stride2)
  for s in (stride1, stride2):
    if not (np.isfinite(s) and s > 0):
      raise ValueError(f'strides must be finite and positive, got {stride1}, {stride2}')
  starts = []
  for name, shape, b in (('box1', shape1, box1), ('box2', shape2, box2)):
    start, size = _box_xy(b, name)
    if (shape[3], shape[2]) != (size[0], size[1]):
      raise ValueError(f'{name} shape ({size}) mismatch with coord map ({shape})')
    starts.append(start)
  dev = _dev.device()
  m1 = _engine_map(map1, dev, keep_f32=True)
  m2 = _engine_map(map2, dev, keep_f32=True)
  d = _abi.SfmComposeTriDesc()
  d.shape1 = (C.c_int32 * 3)(*m1.shape[1:])
  d.shape2 = (C.c_int32 * 3)(*m2.shape[1:])
  d.start1 = _i32_pair('box1.start', starts[0][1], starts[0][0])
  d.start2 = _i32_pair('box2.start', starts[1][1], starts[1][0])
  d.stride1, d.stride2 = stride1, stride2
  d.f64_1 = int(m1.dtype == torch.float64)
  d.f64_2 = int(m2.dtype == torch.float64)
  d.map1, d.map2 = m1.data_ptr(), m2.data_ptr()
  if scale2 is not None:
    if not (scale2.is_cuda and scale2.dtype == torch.float64 and scale2.is_contiguous() and
            tuple(scale2.shape) == (m1.shape[1],)):
      raise ValueError('scale2 must be a contiguous float64 device vector [z of map1]')
    d.scale2 = scale2.data_ptr()
  status = torch.empty(int(m2.shape[1]), dtype=torch.int32, device=dev)
  d.status = status.data_ptr()
  lib = _abi.load()
  ws = _dev.workspace(lib.sfm_compose_maps_tri_workspace_bytes(C.byref(d)), dev)
  d.workspace = ws.data_ptr()
  d.workspace_bytes = ws.numel()
  d.stream = _dev.stream_ptr()
  out = torch.empty_like(m1)
  _abi.check(lib.sfm_compose_maps_tri(C.byref(d), out.data_ptr()))
  return out, status


# -- geometry helpers: to_absolute / to_relative / outer_box / inner_box /
# -- make_affine_map ------------------------------------------------------------


def _box(box):
  """(start xyz, size xyz) of a bounding box object or (start, size) pair."""
  if hasattr(box, 'start') and hasattr(box, 'size'):
    return np.asarray(box.start), np.asarray(box.size)
  return np.asarray(box[0]), np.asarray(box[1])


def _make_box(like, start, size):
  """A box of the kind of `like`: its own type, or a (start, size) pair of int
  arrays when `like` is a pair (the assignment into an int array truncates, as
  the reference's `start[i] = ...` does)."""
  if hasattr(like, 'start') and hasattr(like, 'size'):
    return type(like)(start=start, size=size)
  return np.array(start).astype(np.int64), np.array(size).astype(np.int64)


def _device_map(coord_map, dev) -> torch.Tensor:
  """[2 or 3, z, y, x] float32 / float64 contiguous device tensor; the dtype is
  kept (other dtypes become float64, NumPy's result of adding float64 offsets)."""
  if isinstance(coord_map, DeviceArray):
    coord_map = coord_map.tensor
  if isinstance(coord_map, torch.Tensor):
    t = coord_map
    if t.dtype not in (torch.float32, torch.float64):
      t = t.to(torch.float64)
    t = t.to(dev).contiguous()
  else:
    arr = np.asarray(coord_map)
    if arr.dtype not in (np.float32, np.float64):
      arr = arr.astype(np.float64)
    t = _dev.upload(np.ascontiguousarray(arr), dev)
  if t.ndim != 4 or t.shape[0] not in (2, 3):
    raise ValueError(f'coord_map must be [2 or 3, z, y, x], got shape {tuple(t.shape)}')
  if t.numel() == 0:
    raise ValueError(f'empty coord_map: {tuple(t.shape)}')
  return t


def _zyx3(values, dim, fill):
  """[z]yx values padded to 3 doubles (the z entry of 2-channel maps is `fill`)."""
  return (C.c_double * 3)(*([fill] * (3 - dim) + [float(v) for v in values]))


def _box_offsets(m, stride, box):
  """(stride zyx, box.start * stride zyx) as the reference forms them."""
  dim = m.shape[0]
  stride = _as_vec(stride, dim)
  start = [0.0] * dim
  if box is not None:
    b_start, b_size = _box(box)
    if not np.all(tuple(m.shape)[-dim:][::-1] == b_size[:dim]):
      raise ValueError(
          f'box shape ({b_size}) mismatch with coord map ({tuple(m.shape)})')
    # float64 like NumPy: int64 start times a Python / NumPy scalar stride
    start = [float(np.float64(s) * np.float64(st))
             for s, st in zip(b_start[:dim][::-1], stride)]
  return stride, start


def _shift(coord_map, stride, box, direction) -> DeviceArray:
  dev = _dev.device()
  m = _device_map(coord_map, dev)
  dim = m.shape[0]
  stride, start = _box_offsets(m, stride, box)
  out = torch.empty_like(m)
  d = _abi.SfmMapShiftDesc()
  d.ncomp = dim
  d.f64 = int(m.dtype == torch.float64)
  d.direction = direction
  d.shape = (C.c_int32 * 3)(*m.shape[1:])
  d.stride = _zyx3(stride, dim, 1.0)
  d.start = _zyx3(start, dim, 0.0)
  d.coord_map = m.data_ptr()
  d.out = out.data_ptr()
  d.stream = _dev.stream_ptr()
  _abi.check(_abi.load().sfm_map_shift(C.byref(d)))
  return DeviceArray(out)


def to_absolute(coord_map, stride, box=None) -> DeviceArray:
  """Converts a [2 or 3, z, y, x] map from relative to absolute representation.

  Same contract as the reference (map_utils.py:150-185): `stride` is a scalar
  or a [z]yx sequence; `box` (`.start` / `.size` in xyz, or a (start, size)
  pair) places the origin, and its size must agree with the map.  The map
  (NumPy, torch or DeviceArray, float32 or float64) is never written; the
  result has its dtype.  Arithmetic is NumPy's in-place `+=` of a float64
  offset array: index * stride (+ start * stride) is formed in double, added to
  the widened element and the sum narrowed once.
  """
  return _shift(coord_map, stride, box, _abi.SHIFT_TO_ABSOLUTE)


def to_relative(coord_map, stride, box=None) -> DeviceArray:
  """Converts a [2 or 3, z, y, x] map from absolute to relative representation
  (map_utils.py:188-224); the inverse bookkeeping of `to_absolute`, with the
  same argument meaning and rounding."""
  return _shift(coord_map, stride, box, _abi.SHIFT_TO_RELATIVE)


def _extents(coord_map, stride, box, mode):
  """The 8 doubles of sfm_map_extents (one host sync) and the map's NumPy dtype."""
  dev = _dev.device()
  m = _device_map(coord_map, dev)
  dim = m.shape[0]
  stride, start = _box_offsets(m, stride, box)
  result = torch.empty(8, dtype=torch.float64, device=dev)
  ws = _dev.workspace(_abi.MAP_EXTENTS_WORKSPACE_BYTES, dev)
  d = _abi.SfmMapExtentsDesc()
  d.ncomp = dim
  d.f64 = int(m.dtype == torch.float64)
  d.mode = mode
  d.shape = (C.c_int32 * 3)(*m.shape[1:])
  d.stride = _zyx3(stride, dim, 1.0)
  d.start = _zyx3(start, dim, 0.0)
  d.coord_map = m.data_ptr()
  d.result = result.data_ptr()
  d.workspace = ws.data_ptr()
  d.workspace_bytes = ws.numel()
  d.stream = _dev.stream_ptr()
  _abi.check(_abi.load().sfm_map_extents(C.byref(d)))
  dtype = np.float64 if m.dtype == torch.float64 else np.float32
  return result.cpu().numpy(), dtype, dim, stride


def outer_box(coord_map, box, stride, target_len=None):
  """Returns a bounding box covering all target nodes (map_utils.py:307-342).

  `coord_map` is in relative format, `box` the box it was extracted from,
  `target_len` the node spacing of the output box ([z]yx or a scalar, defaults
  to `stride`).  The device reduces nanmin / nanmax per channel of the absolute
  map in one pass without storing it; the reference's integer expressions are
  applied to those scalars on the host.  An all-NaN channel raises ValueError,
  as `int(nan)` does in the reference.  The box is of the type of `box`.
  """
  res, dtype, dim, stride = _extents(coord_map, stride, box, _abi.EXTENTS_OUTER)
  target_len_xyz = _as_vec(target_len if target_len is not None else stride, dim)[::-1]
  b_start, b_size = _box(box)
  start = np.array(b_start).copy()
  size = np.array(b_size).copy()
  for i, tl in enumerate(target_len_xyz):
    if res[2 * i] == np.inf and res[2 * i + 1] == -np.inf:   # no finite or infinite value
      x_min = x_max = dtype(np.nan)
    else:
      x_min, x_max = dtype(res[2 * i]), dtype(res[2 * i + 1])
    x_min = int(x_min) // tl
    start[i] = x_min
    size[i] = -(int(-x_max) // tl) - x_min + 1
  return _make_box(box, start, size)


def inner_box(coord_map, box, stride):
  """Returns a box within which all nodes are mapped to by the map
  (map_utils.py:345-389), for maps WITHOUT NaN.

  The reference first extrapolates invalid entries with `fill_missing` and its
  default `interpolate_first=True`, which returns a NaN-free map unchanged; that
  branch has no parity contract (see the module docstring), so a map that holds
  a NaN raises NotImplementedError.
  The device returns the max of the per-line minima and the min of the per-line
  maxima of the absolute map along x, y[, z] in the map's dtype; the
  reference's `//` expressions are applied to NumPy scalars of that dtype.
  """
  res, dtype, dim, stride = _extents(coord_map, stride, box, _abi.EXTENTS_INNER)
  if res[6] != 0:
    raise NotImplementedError(
        'inner_box: the map holds NaN; the reference extrapolates them with '
        'fill_missing, which is not on the device')
  x0, x1, y0, y1, z0, z1 = (dtype(v) for v in res[:6])
  b_start, b_size = _box(box)

  x0 = int(-(-x0 // stride[-1]))
  y0 = int(-(-y0 // stride[-2]))
  x1 = x1 // stride[-1]
  y1 = y1 // stride[-2]

  if dim == 2:
    return _make_box(box, (x0, y0, b_start[2]),
                     (x1 - x0 + 1, y1 - y0 + 1, b_size[2]))

  z0 = int(-(-z0 // stride[0]))
  z1 = z1 // stride[0]
  return _make_box(box, (x0, y0, z0), (x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1))


def fill_missing(coord_map, *, extrapolate=False, invalid_to_zero=False,
                 interpolate_first=True) -> DeviceArray:
  """Fills missing entries of a [2 or 3, z, y, x] coordinate map
  (map_utils.py:227-304), without the reference's Delaunay interpolation.

  Name, keywords and defaults are the reference's; `coord_map` is NumPy, a CUDA
  tensor or a DeviceArray, float32 or float64 (TypeError otherwise; other
  channel counts raise ValueError), is never written, and the result is a new
  DeviceArray of its dtype.  A 2-channel map is filled per z slice, a 3-channel
  map as one volume.

  * A map without NaN is returned unchanged (a copy); `inf` entries stay.
  * `interpolate_first=True` -- the default -- on a map that holds NaN raises
    NotImplementedError: that branch triangulates the regular lattice, whose
    quads are co-circular, so Qhull's pick of diagonals is arbitrary and the
    result has no parity contract.  So `fill_missing(m)` with the default
    arguments raises for a map with NaN; pass `interpolate_first=False`.
  * A node is valid when all its channels are finite (`inf` makes it invalid).
    A slice (volume) without a valid node becomes all zeros with
    `invalid_to_zero`, else all NaN with `extrapolate` (SciPy's
    NearestNDInterpolator over an empty point set), else stays as it is.
  * `interpolate_first=False, extrapolate=True`: every invalid node gets, in all
    channels, the bits of the valid node at the smallest squared Euclidean
    distance in node indices (isotropic, strides ignored; z counts for 3-channel
    maps only).  Among equidistant nodes the lowest C-order index of [z,] y, x
    wins -- SciPy's pick there is an artefact of its k-d tree, so the result
    equals the reference's wherever the nearest node is unique.  Valid nodes
    keep their bits.
  * `interpolate_first=False, extrapolate=False`: only the `invalid_to_zero`
    rule applies.

  Distances are exact 32-bit integers: an axis holds at most 16384 nodes and
  the map fewer than 2^31 nodes per channel (ValueError above).  Nothing comes
  to the host except, with `interpolate_first=True`, the NaN flag.
  """
  if isinstance(coord_map, DeviceArray):
    coord_map = coord_map.tensor
  shape = tuple(coord_map.shape) if isinstance(coord_map, torch.Tensor) else np.shape(coord_map)
  if len(shape) != 4 or shape[0] not in (2, 3):
    raise ValueError(f'coord_map must be [2 or 3, z, y, x], got shape {tuple(shape)}')
  dev = _dev.device()
  if isinstance(coord_map, torch.Tensor):
    if coord_map.dtype not in (torch.float32, torch.float64):
      raise TypeError(f'fill_missing: float32 or float64 maps, got {coord_map.dtype}')
    m = coord_map.to(dev).contiguous()
  else:
    arr = np.asarray(coord_map)
    if arr.dtype not in (np.float32, np.float64):
      raise TypeError(f'fill_missing: float32 or float64 maps, got {arr.dtype}')
    m = _dev.upload(np.ascontiguousarray(arr), dev)
  if min(shape[1:]) < 1:
    raise ValueError(f'empty coord_map: {tuple(shape)}')
  if max(shape[1:]) > _abi.FILL_MISSING_MAX_AXIS or m[0].numel() >= 2**31:
    raise ValueError(
        f'fill_missing: at most {_abi.FILL_MISSING_MAX_AXIS} nodes per axis and fewer than '
        f'2^31 per channel, got shape {tuple(shape)}')
  out = torch.empty_like(m)
  has_nan = torch.empty(1, dtype=torch.int32, device=dev)
  d = _abi.SfmFillMissingDesc()
  d.ncomp = shape[0]
  d.f64 = int(m.dtype == torch.float64)
  d.shape = (C.c_int32 * 3)(*shape[1:])
  # with interpolate_first the call only copies the map and reports the flag
  d.invalid_to_zero = int(bool(invalid_to_zero) and not interpolate_first)
  d.extrapolate = int(bool(extrapolate) and not interpolate_first)
  d.coord_map = m.data_ptr()
  d.out = out.data_ptr()
  d.has_nan = has_nan.data_ptr()
  lib = _abi.load()
  ws = _dev.workspace(lib.sfm_fill_missing_nearest_workspace_bytes(C.byref(d)), dev)
  d.workspace = ws.data_ptr()
  d.workspace_bytes = ws.numel()
  d.stream = _dev.stream_ptr()
  _abi.check(lib.sfm_fill_missing_nearest(C.byref(d)))
  if interpolate_first and int(has_nan.item()):
    raise NotImplementedError(
        'fill_missing: the map holds NaN and interpolate_first=True asks for a Delaunay '
        'interpolation over the regular lattice, where every quad is co-circular and Qhull '
        'picks the diagonals arbitrarily; it is not on the device.  '
        'interpolate_first=False fills by the nearest valid node')
  return DeviceArray(out)


def make_affine_map(matrix, box, stride) -> DeviceArray:
  """Builds a [3, z, y, x] float64 coordinate map for an affine transform
  (map_utils.py:789-811): `matrix` is [3, 4] in the format of
  ndimage.affine_transform with xyz rows and columns, `box` the box to
  generate the map for, `stride` zyx or a scalar.  Node positions are
  index * stride + box.start; the map is matrix[:, :3] @ p + matrix[:, 3] - p in
  plain left-to-right float64 (the reference's np.dot may fuse or reorder the
  three products: the results agree to a few ulp of the largest term).
  """
  matrix = np.asarray(matrix, dtype=np.float64)
  if matrix.shape != (3, 4):
    raise ValueError(f'matrix must be [3, 4], got {matrix.shape}')
  b_start, b_size = _box(box)
  shape = tuple(int(v) for v in b_size[::-1])
  if len(shape) != 3 or min(shape) < 1:
    raise ValueError(f'box size must be 3 positive entries, got {b_size}')
  stride = _as_vec(stride, 3)
  dev = _dev.device()
  out = torch.empty((3,) + shape, dtype=torch.float64, device=dev)
  d = _abi.SfmAffineMapDesc()
  d.shape = (C.c_int32 * 3)(*shape)
  d.stride = _zyx3(stride, 3, 1.0)
  d.start = _zyx3(b_start[:3][::-1], 3, 0.0)
  d.matrix = (C.c_double * 12)(*matrix.ravel())
  d.out = out.data_ptr()
  d.stream = _dev.stream_ptr()
  _abi.check(_abi.load().sfm_affine_map(C.byref(d)))
  return DeviceArray(out)
