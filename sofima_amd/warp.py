"""Image warping by coordinate maps on MI355X.

Drop-in for `warp.warp_subvolume` of the reference (warp.py:58-186), the
rendering step that follows mesh relaxation.  Every
section is ONE kernel (`sfm_warp_section`): linear interpolation of the map
nodes to the output pixels (scipy RegularGridInterpolator in the reference),
conversion to OpenCV's 1/32-pixel fixed-point map format and the `cv2.remap`
resampling are fused, so the two dense float maps per section never exist.

Parity note: OpenCV is not available to the test suite, so the resampling
semantics (convertMaps rounding, the 32 x 32-phase weight tables of
initInterTab2D with 15-bit fixed point for 8-bit images, constant zero border)
are restated from OpenCV's published algorithm.  Pinned: the reference's own
tests (tests/warp_test.py:27-82), and tap geometry, interpolation kernels,
border handling and the 1/32-pixel coordinate quantisation against an
independent float64 resampling reference written from the definitions
(tests/test_gpu_postflow_edges.py: integer images within 1 count, float32
images within 1.64e-6 of the image maximum).  Not pinned: bit parity with a
real OpenCV build (which tap takes a table's rounding remainder).
`ndimage_warp` (warp.py:189-335), the SciPy-only rendering path, is built as
well and IS pinned: the reference function runs through the golden shim and
the kernel reproduces its output bit for bit (tests/golden/ndimage_warp.npz),
for the spline orders 2 to 5 as well (ndimage_warp_spline.npz): those sample
B-spline coefficients that a device prefilter computes in SciPy's operation
order (sfm_spline_prefilter), and are opt-in (SFM_SPLINE_ORDERS=1).
`warp_points` (warp.py:541-605) maps point sets through a coordinate map: one
kernel, every point reads its four map nodes directly, pinned against the
reference function through the golden shim (tests/golden/mapgeom.npz).
`ndimage_warp` also takes SciPy's sampler with a boundary mode and a fill value
(`map_coordinates=functools.partial(scipy.ndimage.map_coordinates, mode=...,
cval=...)`, as decorators/warp.py calls it), and `affine_transform` is
scipy.ndimage.affine_transform as one fused kernel that reads no coordinate
map; both are pinned to SciPy bit for bit (tests/test_gpu_ndwarp_modes.py,
tests/test_gpu_affine_warp.py).
`ndimage_warp` and `affine_transform` take resident images (CUDA tensors,
DeviceArrays) and return DeviceArrays on request, and `ndimage_warp` reads a
float32 / float64 coordinate map RELATIVE, in its own dtype and where it lies
(`sfm_ndimage_warp_rel`): the kernel forms the absolute source coordinate of each
node it reads, with the roundings of the reference's NumPy statements, so
invert_map / compose_maps_fast / make_affine_map -> ndimage_warp is one device
chain with no host copy of the map (tests/test_gpu_warp_device.py).
render_tiles has no parity contract and stays out of scope.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from . import _abi
from . import _dev
from . import _spline
from . import map_utils

_INTER = {'nearest': 0, 'linear': 1, 'cubic': 2, 'lanczos': 3}
_TAB = 32            # INTER_TAB_SIZE
_COEF_SCALE = 1 << 15  # INTER_REMAP_COEF_SCALE


def _coeffs_1d(kind: int) -> np.ndarray:
  """[32, ksize] float32 tap weights per sub-pixel phase."""
  x = np.arange(_TAB, dtype=np.float32) / np.float32(_TAB)
  if kind == 1:
    return np.stack([1 - x, x], axis=1).astype(np.float32)
  if kind == 2:
    a = np.float32(-0.75)
    c0 = ((a * (x + 1) - 5 * a) * (x + 1) + 8 * a) * (x + 1) - 4 * a
    c1 = ((a + 2) * x - (a + 3)) * x * x + 1
    c2 = ((a + 2) * (1 - x) - (a + 3)) * (1 - x) * (1 - x) + 1
    return np.stack([c0, c1, c2, 1 - c0 - c1 - c2], axis=1).astype(np.float32)
  # Lanczos, a = 4: sin(pi t) sin(pi t / 4) / t^2 through the angle-addition
  # table OpenCV uses for the eight taps
  s45 = 0.70710678118654752440084436210485
  cs = np.array([[1, 0], [-s45, -s45], [0, 1], [s45, -s45], [-1, 0], [s45, s45],
                 [0, -1], [-s45, s45]])
  out = np.zeros((_TAB, 8), np.float32)
  for i, xv in enumerate(x):
    if xv < np.finfo(np.float32).eps:
      out[i, 3] = 1
      continue
    y0 = -(float(xv) + 3) * np.pi * 0.25
    s0, c0 = np.sin(y0), np.cos(y0)
    y = -(float(xv) + 3 - np.arange(8)) * np.pi * 0.25
    c = ((cs[:, 0] * s0 + cs[:, 1] * c0) / (y * y)).astype(np.float32)
    out[i] = c * (np.float32(1) / c.sum(dtype=np.float32))
  return out


@functools.lru_cache(maxsize=None)
def _inter_tab(kind: int, fixed: bool) -> np.ndarray:
  """[32 * 32, ksize * ksize] 2-d weights (phase = 32 * fy + fx); int16 with 15
  fractional bits when `fixed` (8-bit images), rounding error folded into one
  tap the way OpenCV does it."""
  c = _coeffs_1d(kind)
  ks = c.shape[1]
  tab = (c[:, None, :, None] * c[None, :, None, :]).reshape(_TAB * _TAB, ks * ks)
  tab = tab.astype(np.float32)
  if not fixed:
    return np.ascontiguousarray(tab)
  it = np.clip(np.rint(tab * np.float32(_COEF_SCALE)), -32768, 32767).astype(np.int32)
  # OpenCV's initInterTab2D, statement for statement: the rounding error of a
  # phase goes to the largest (deficit) / smallest (excess) of the taps
  # (k1, k2) in [ks/2, ks/2 + 2)^2, found with strict compares starting from
  # (ks/2, ks/2), and the corrected tap is cast to short.  The tables of all
  # phases are one array filled phase by phase, and for the 2 x 2 bilinear
  # kernel that index range runs past the phase's own taps into the (still
  # zero) taps of the following phases: the scan sees those zeros, and a
  # correction written there is overwritten when that phase is filled.
  kk = ks * ks
  flat = np.zeros((_TAB * _TAB + 4) * kk, np.int64)
  h = ks // 2
  scan = [k1 * ks + k2 for k1 in (h, h + 1) for k2 in (h, h + 1)]
  for e in range(_TAB * _TAB):
    base = e * kk
    flat[base:base + kk] = it[e]
    diff = int(it[e].sum()) - _COEF_SCALE
    if diff:
      big = small = base + scan[0]
      for off in scan:
        v = flat[base + off]
        if v < flat[small]:
          small = base + off
        elif v > flat[big]:
          big = base + off
      k = big if diff < 0 else small
      flat[k] = ((int(flat[k]) - diff + 32768) & 0xffff) - 32768   # (short)
  it = flat[:_TAB * _TAB * kk].reshape(_TAB * _TAB, kk)
  return np.ascontiguousarray(it.astype(np.int16))


_box = map_utils._box


def _make_contiguous(image: np.ndarray):
  """uint64 segment ids -> dense int32 ids (0 stays 0) and the inverse table."""
  ids, inv = np.unique(image, return_inverse=True)
  if ids[0] != 0:
    ids = np.concatenate([[0], ids]).astype(np.uint64)
    inv = inv + 1
  assert len(ids) < 2**31
  return inv.reshape(image.shape).astype(np.int32), ids


def warp_subvolume(image: np.ndarray, image_box, coord_map: np.ndarray, map_box,
                   stride: float, out_box, interpolation: str | None = None,
                   offset: float = 0.0, parallelism: int = 1) -> np.ndarray:
  """Warps a subvolume of data according to a coordinate map (warp.py:58-186).

  image: [n, z, y, x] uint8 / uint16 / float32 data, or uint64 segmentation
  (nearest neighbour on contiguous ids, mapped back afterwards); coord_map:
  [2, z, y, x] xy 'inverse' map in relative format; boxes: objects with
  `.start` / `.size` in xyz (or (start, size) pairs); `stride`: image pixels
  per map node.  Sections whose map is all NaN are skipped (left zero).
  `parallelism` is accepted for compatibility: sections are enqueued back to
  back on the GPU.  Image and map are host arrays and the result is one: this
  OpenCV-semantics path is not part of the resident chain that `ndimage_warp`
  and `affine_transform` serve (it prepares its absolute map on the host).
  """
  del parallelism
  dev = _dev.device()
  image = np.asarray(image)
  ids = None
  orig_dtype = image.dtype
  if image.dtype == np.uint64:
    kind = 0
    image, ids = _make_contiguous(image)
    dtype = _abi.DTYPE_I32
  else:
    kind = 3 if interpolation is None else _INTER[interpolation]
    if image.dtype == np.uint32:
      if image.max() >= 2**16:
        raise ValueError(
            'Image warping supported up to uint16 only. For segmentation data, '
            'use uint64.')
      image = image.astype(np.uint16)
    if image.dtype == np.uint8:
      dtype = _abi.DTYPE_U8
    elif image.dtype == np.uint16:
      dtype = _abi.DTYPE_U16
    else:
      image = image.astype(np.float32, copy=False)
      dtype = _abi.DTYPE_F32
  img_start, _ = _box(image_box)
  map_start, _ = _box(map_box)
  out_start, out_size = _box(out_box)
  coord_map = np.asarray(coord_map)
  skipped = np.all(np.isnan(coord_map), axis=(0, 2, 3))

  if coord_map.shape[1] < image.shape[1] or int(out_size[2]) < image.shape[1]:
    # the reference indexes abs_map[:, z] and warped[:, z] for every z of image
    raise ValueError(
        f'z extents disagree: image {image.shape[1]}, coord_map {coord_map.shape[1]}, '
        f'out_box {int(out_size[2])}')

  # absolute source coordinates in the local frame of `image`
  # (map_utils.to_absolute + the box shift, warp.py:125-128): the reference
  # adds both in place, i.e. rounds twice to the MAP's dtype, and interpolates
  # the dense coordinates from those values -- same here, float32 or float64
  my, mx = coord_map.shape[2:]
  hy, hx = np.mgrid[:my, :mx]
  shift = map_start[:2] * stride - img_start[:2] + offset
  map_dtype = np.float64 if coord_map.dtype == np.float64 else np.float32
  abs_map = coord_map.astype(map_dtype, copy=True)
  abs_map[0] += hx * stride
  abs_map[1] += hy * stride
  abs_map += np.asarray(shift, np.float64).reshape(2, 1, 1)[:, None]
  map_t = torch.from_numpy(abs_map).to(dev)

  img_t = torch.from_numpy(np.ascontiguousarray(image).view(
      np.int16 if image.dtype == np.uint16 else image.dtype)).to(dev)
  out_t = torch.zeros((image.shape[0], int(out_size[2]), int(out_size[1]),
                       int(out_size[0])), dtype=img_t.dtype, device=dev)
  d = _abi.SfmWarpDesc()
  d.dtype = dtype
  d.interpolation = _abi.WARP_NEAREST if kind == 0 else _abi.WARP_TABLE
  tab_t = None
  if kind != 0:
    tab = _inter_tab(kind, dtype == _abi.DTYPE_U8)
    tab_t = torch.from_numpy(tab).to(dev)
    d.ksize = int(round(np.sqrt(tab.shape[1])))
    d.weights = tab_t.data_ptr()
  d.image_shape = (C.c_int32 * 2)(*image.shape[2:])
  d.map_shape = (C.c_int32 * 2)(my, mx)
  d.out_shape = (C.c_int32 * 2)(int(out_size[1]), int(out_size[0]))
  d.map_origin = (C.c_double * 2)(
      float(map_start[1] * stride - out_start[1] + offset),
      float(map_start[0] * stride - out_start[0] + offset))
  d.stride = float(stride)
  d.coord_map_f64 = 1 if map_dtype == np.float64 else 0
  d.stream = _dev.stream_ptr()
  lib = _abi.load()
  for z in range(image.shape[1]):
    if skipped[z]:
      continue
    zmap = map_t[:, z].contiguous()   # kept alive until the launches are enqueued
    d.coord_map = zmap.data_ptr()
    for c in range(image.shape[0]):
      d.image = img_t[c, z].data_ptr()
      d.out = out_t[c, z].data_ptr()
      _abi.check(lib.sfm_warp_section(C.byref(d)))
  warped = out_t.cpu().numpy()
  if ids is not None:
    return ids[warped]
  if orig_dtype == np.uint16 or image.dtype == np.uint16:
    warped = warped.view(np.uint16)
  return warped.astype(orig_dtype)


def _scipy_sampler(map_coordinates):
  """(mode, cval) of a `map_coordinates` argument that the device reproduces:
  scipy.ndimage.map_coordinates itself, or a functools.partial of it with no
  positional arguments and keywords among mode and cval.  None otherwise."""
  try:
    import scipy.ndimage
  except ImportError:
    return None
  kw = {}
  if isinstance(map_coordinates, functools.partial):
    if map_coordinates.args or not set(map_coordinates.keywords) <= {'mode', 'cval'}:
      return None
    kw = map_coordinates.keywords
    map_coordinates = map_coordinates.func
  if map_coordinates is not scipy.ndimage.map_coordinates:
    return None
  return kw.get('mode', 'constant'), kw.get('cval', 0.0)


def _boundary(what: str, mode, cval, order, dtype) -> tuple[int, float]:
  """(SFM_MODE_*, cval) of SciPy's `mode` / `cval`, or the error of what is not built."""
  if mode not in _abi.MODES:
    raise ValueError(f'{what}: boundary mode {mode!r} (one of {sorted(_abi.MODES)})')
  _spline.check_mode(mode, order, what)
  cval = float(cval)
  if np.dtype(dtype).kind != 'f' and not np.isfinite(cval):
    raise ValueError(f'{what}: cval {cval} for a {np.dtype(dtype)} image')
  return _abi.MODES[mode], cval


_TORCH_DTYPES = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.float32: np.float32,
                 torch.float64: np.float64, torch.uint64: np.uint64}


def _resident(x):
  """The tensor of a DeviceArray or CUDA tensor; a NumPy array of anything else (a
  CPU tensor is host data like an array)."""
  if isinstance(x, _dev.DeviceArray):
    x = x.tensor
  if isinstance(x, torch.Tensor):
    return x if x.is_cuda else x.numpy()
  return np.asarray(x)


def _np_dtype(x, what: str) -> np.dtype:
  """NumPy dtype of an array or of a device tensor."""
  if not isinstance(x, torch.Tensor):
    return x.dtype
  if x.dtype not in _TORCH_DTYPES:
    raise NotImplementedError(f'{what}: {x.dtype} device tensors')
  return np.dtype(_TORCH_DTYPES[x.dtype])


def _image_tensor(image, view, dev) -> torch.Tensor:
  """Contiguous device tensor of an image; uint16 is held as int16, the type torch
  has kernels for (a view: the library reads the bits as unsigned)."""
  if isinstance(image, torch.Tensor):
    if image.dtype == torch.uint16:
      image = image.view(torch.int16)
    return image.to(dev).contiguous()
  return torch.from_numpy(np.ascontiguousarray(image).view(view)).to(dev)


def _warped(out_t: torch.Tensor, dtype: np.dtype, device_output: bool):
  """The result as a DeviceArray of the image's dtype, or downloaded."""
  if device_output:
    return _dev.DeviceArray(out_t.view(torch.uint16) if dtype == np.uint16 else out_t)
  warped = out_t.cpu().numpy()
  if dtype == np.uint16:
    warped = warped.view(np.uint16)
  return warped.astype(dtype)


def _transpose_resident(t: torch.Tensor) -> torch.Tensor:
  """Axes reversed (xyz <-> zyx) on the device, contiguous."""
  if t.dtype == torch.uint16:
    return t.view(torch.int16).permute(*reversed(range(t.ndim))).contiguous().view(torch.uint16)
  return t.permute(*reversed(range(t.ndim))).contiguous()


def ndimage_warp(image, coord_map, stride, work_size, overlap,
                 order=1, map_coordinates=None, image_box=None, map_box=None, out_box=None,
                 parallelism: int = 1, out_scale=(1.0, 1.0, 1.0),
                 device_output: bool | None = None):
  """Warps a subvolume of data using map_coordinates semantics (warp.py:189-335).

  image: [z, ] y, x data (uint8 / uint16 / float32); coord_map: [N, [z,] y, x]
  relative coordinate map; stride: [z,] y, x image voxels per map node;
  image_box / map_box / out_box: objects with `.start` / `.size` in xyz (or
  (start, size) pairs); out_scale: xy[z] out_voxel / source_voxel.

  `image` and `coord_map` may each be a NumPy array, a CUDA torch tensor or a
  DeviceArray (a CPU tensor counts as an array); device images are uint8, uint16
  or float32 tensors.  device_output: True returns a DeviceArray of the image's
  dtype, False a NumPy array, None (the default) follows the image.  A float32 or
  float64 map is read RELATIVE and in its own dtype (`sfm_ndimage_warp_rel`): a
  NumPy map is uploaded once as it is, a resident one is read where it lies, and
  the kernel forms the absolute source coordinate of every node it reads with
  the reference's roundings.  With image and map resident and a
  device output the call copies nothing to the host and does not wait for the
  compute stream (orders 2 to 5 upload the prefilter's table on a side stream).
  A NumPy map of another dtype is made absolute on the host in NumPy's own
  arithmetic, as before; a resident map of another dtype raises TypeError.

  One kernel computes, per output voxel, what the reference computes with two
  rounds of scipy.ndimage.map_coordinates per work box (dense coordinates by
  order-1 interpolation of the absolute map, then order-`order` sampling of the
  image), in double and in SciPy's operation order -- bit for bit the
  reference's output (tests/golden/ndimage_warp.npz, ndimage_warp_spline.npz).
  For orders 2 to 5 SciPy samples B-spline coefficients of the image: they are
  computed once per call into a float64 workspace of 8 bytes per voxel
  (`_spline.prefilter`; a request beyond the free-memory budget raises
  MemoryError) and the same kernel samples them.  `work_size`, `overlap` and
  `parallelism` only shape the reference's host loop and do not change the
  result for any order (the reference prefilters the WHOLE image again for
  every work box); they are validated and otherwise unused.  Built: orders 0
  and 1, and with the switch SFM_SPLINE_ORDERS=1 (`_abi.set_option`) orders 2
  to 5, with the default `map_coordinates`; without the switch orders above 1
  raise NotImplementedError as they always did; custom samplers and uint64
  label volumes raise it too (use `warp_subvolume` for label volumes).

  `map_coordinates` may be scipy.ndimage.map_coordinates or a functools.partial
  of it that sets `mode` and / or `cval` (decorators/warp.py:237-242): the
  kernel then applies that boundary mode and fill value to BOTH steps, as the
  reference passes the callable to both -- outside the node grid the dense
  coordinate is `cval` in source voxels (or the folded node value), and the
  image sample follows the same rule.  Orders 0 and 1 take every mode of SciPy,
  orders 2 to 5 'constant', 'mirror' and 'wrap', and with the switch
  SFM_SPLINE_MODES=1 the others too: 'nearest', 'reflect' ('grid-mirror'),
  'grid-constant' and 'grid-wrap' have B-spline prefilters of their own, and
  'nearest' and 'grid-constant' filter the image padded by 12 samples per axis, as
  SciPy does (the workspace is then 8 bytes per padded voxel); an integer image needs a
  finite `cval` and takes it through the conversion of a sampled value.  A NaN
  coordinate or one of magnitude 2**31 and above gives `cval` (SciPy's result
  there is an undefined cast, except under 'constant').
  """
  del parallelism
  image = _resident(image)
  coord_map = _resident(coord_map)
  img_dtype = _np_dtype(image, 'ndimage_warp')
  shape = tuple(coord_map.shape[1:])
  dim = len(shape)
  assert dim == len(stride)
  assert dim == len(overlap)
  assert dim == len(work_size)
  if dim != image.ndim:
    raise ValueError(f'Dimension mismatch: image: {image.ndim} vs coord map: {dim}')
  boundary = None
  if map_coordinates is not None:
    boundary = _scipy_sampler(map_coordinates)
    if boundary is None:
      raise NotImplementedError(
          'ndimage_warp: custom map_coordinates callables run on the host only '
          '(scipy.ndimage.map_coordinates, or a functools.partial of it with mode / cval, '
          'runs on the device)')
    if boundary == ('constant', 0.0):
      boundary = None
  if img_dtype == np.uint64:
    raise NotImplementedError('ndimage_warp: uint64 label volumes (use warp_subvolume)')
  _spline.check_order(order, 'ndimage_warp')
  mode = 'constant'
  if boundary is not None:
    mode = boundary[0]
    boundary = _boundary('ndimage_warp', boundary[0], boundary[1], order, img_dtype)
  if dim not in (2, 3):
    raise ValueError(f'ndimage_warp: {dim}-d data')
  if map_box is not None and image_box is None:
    raise ValueError('image_box has to be specified when map_box is used.')
  if isinstance(coord_map, torch.Tensor) and coord_map.dtype not in (torch.float32,
                                                                     torch.float64):
    raise TypeError(f'ndimage_warp: {coord_map.dtype} device maps (float32, float64)')

  # The absolute source map (warp.py:250-265) is formed by the kernel from the
  # relative one, with NumPy's roundings, when those are the ones of a float32 /
  # float64 map and a float64 out_scale product; any other map is made absolute
  # here in NumPy's own arithmetic.
  scale = np.array(out_scale[:dim])
  map_dtype = _np_dtype(coord_map, 'ndimage_warp')
  relative = (map_dtype in (np.float32, np.float64) and scale.dtype.kind in 'iuf' and
              np.result_type(map_dtype, scale.dtype) == np.float64)
  shift = None
  if relative and map_box is not None:
    map_start, _ = _box(map_box)
    img_start, _ = _box(image_box)
    shift = np.asarray(map_start[:dim] * np.asarray(stride)[::-1] -
                       img_start[:dim] / np.asarray(out_scale)[:dim], dtype=np.float64)
  if not relative:
    if isinstance(coord_map, torch.Tensor):
      coord_map = coord_map.cpu().numpy()
    coord_map = _absolute_map(coord_map, stride, image_box, map_box, out_scale)

  if out_box is not None:
    out_start, out_size = _box(out_box)
    out_shape = tuple(int(v) for v in np.asarray(out_size)[::-1][-dim:])
  else:
    out_start = np.zeros(3, np.int64)
    out_shape = tuple(image.shape)
  if map_box is not None:
    map_start, _ = _box(map_box)
    offset = (map_start * np.asarray(stride)[::-1] - out_start)[::-1]
  else:
    offset = (0,) * dim

  dtype, view = _image_dtype(img_dtype, 'ndimage_warp')
  if device_output is None:
    device_output = isinstance(image, torch.Tensor)
  dev = _dev.device()
  img_t = _image_tensor(image, view, dev)
  if isinstance(coord_map, torch.Tensor):
    map_t = coord_map.to(dev).contiguous()
  else:
    map_t = torch.from_numpy(np.ascontiguousarray(coord_map)).to(dev)
  out_t = torch.empty(out_shape, dtype=img_t.dtype, device=dev)
  pad = (1,) * (3 - dim)
  d = _abi.SfmNdWarpRelDesc() if relative else _abi.SfmNdWarpDesc()
  d.ndim = dim
  d.dtype = dtype
  d.order = int(order)
  d.image_shape = (C.c_int32 * 3)(*(pad + tuple(image.shape)))
  d.map_shape = (C.c_int32 * 3)(*(pad + shape))
  d.out_shape = (C.c_int32 * 3)(*(pad + out_shape))
  d.stride = (C.c_double * 3)(*((1.0,) * (3 - dim) + tuple(float(v) for v in stride)))
  d.offset = (C.c_double * 3)(*((0.0,) * (3 - dim) + tuple(float(v) for v in offset[-dim:])))
  d.image = img_t.data_ptr()
  d.out = out_t.data_ptr()
  d.stream = _dev.stream_ptr()
  coeffs = _sample_coefficients(d, pad + tuple(image.shape), img_dtype, dev, mode,
                                boundary[1] if boundary else None)
  if relative:
    d.rel_map = map_t.data_ptr()
    d.map_f64 = int(map_dtype == np.float64)
    d.scale = (C.c_double * 3)(*(tuple(float(v) for v in scale) + (1.0,) * (3 - dim)))
    if shift is not None:
      d.has_shift = 1
      d.shift = (C.c_double * 3)(*(tuple(float(v) for v in shift) + (0.0,) * (3 - dim)))
    if boundary is not None:
      d.has_boundary = 1
      d.mode, d.cval = boundary
  else:
    d.src_map = map_t.data_ptr()
  _abi.check(_ndimage_warp_call(d, boundary, order in _spline.ORDERS))
  del coeffs    # (read by the launch above; the stream orders its release)
  return _warped(out_t, img_dtype, device_output)


def _sample_coefficients(d, shape, img_dtype, dev, mode, cval):
  """Orders 2 to 5 sample B-spline coefficients: prefilters the dense image d.image
  of zyx `shape` (ndim, dtype and order are filled in; cval None: no boundary mode)
  and points d.image to the result, which is returned and has to live until the
  launch is issued.  None, and `d` as it is, for orders 0 and 1."""
  if d.order not in _spline.ORDERS:
    return None
  coeffs, _ = _spline.prefilter(
      [(d.image, shape, (shape[1] * shape[2], shape[2], 1))], d.dtype, d.order, dev,
      mode, d.ndim, 0.0 if cval is None else _spline.pad_value(cval, img_dtype))
  d.image = coeffs.data_ptr()
  return coeffs


def _ndimage_warp_call(d, boundary, spline: bool) -> int:
  """Runs the entry point of a filled descriptor: a relative map has one for all
  cases, an absolute map one with a boundary mode, one for orders 2 to 5 and one for
  orders 0 and 1."""
  lib = _abi.load()
  if isinstance(d, _abi.SfmNdWarpRelDesc):
    return lib.sfm_ndimage_warp_rel(C.byref(d))
  if boundary is not None:
    return lib.sfm_ndimage_warp_mode(C.byref(d), boundary[0], boundary[1])
  if spline:
    return lib.sfm_ndimage_warp_spline(C.byref(d))
  return lib.sfm_ndimage_warp(C.byref(d))


def _absolute_map(coord_map: np.ndarray, stride, image_box, map_box, out_scale) -> np.ndarray:
  """The float64 absolute source map on the host, operation for operation
  (map_utils.to_absolute adds in place in the map's dtype; the out_scale product
  is NumPy's): warp.py:250-265.  For the maps the kernel does not read relative."""
  shape = coord_map.shape[1:]
  dim = len(shape)
  src = np.array(coord_map, copy=True)
  idx = np.mgrid[tuple(slice(0, s) for s in shape)]
  off_zyx = [h * st for h, st in zip(idx, stride)]
  for i in range(dim):
    src[i, ...] += off_zyx[-(i + 1)]
  if map_box is not None:
    map_start, _ = _box(map_box)
    img_start, _ = _box(image_box)
    src += (map_start[:dim] * np.asarray(stride)[::-1] -
            img_start[:dim] / np.asarray(out_scale)[:dim]).reshape((dim,) + (1,) * dim)
  reshaper = (slice(None),) + (np.newaxis,) * dim
  return np.ascontiguousarray(src.copy() * np.array(out_scale[:dim])[reshaper], dtype=np.float64)


def _image_dtype(dtype: np.dtype, what: str):
  """(_abi.DTYPE_*, the NumPy type the bits are uploaded as) of an image dtype."""
  if dtype == np.uint8:
    return _abi.DTYPE_U8, np.uint8
  if dtype == np.uint16:
    return _abi.DTYPE_U16, np.int16
  if dtype == np.float32:
    return _abi.DTYPE_F32, np.float32
  raise NotImplementedError(f'{what}: {dtype} images (uint8, uint16, float32)')


def affine_transform(image, matrix, offset=0.0, order=1, mode='constant', cval=0.0,
                     output_shape=None, output=None, device_output: bool | None = None):
  """scipy.ndimage.affine_transform on the device, 2-D and 3-D, bit for bit.

  image: [z, ] y, x data (uint8 / uint16 / float32); matrix: (dim, dim), with
  `offset` a scalar or a vector, or (dim, dim + 1) / (dim + 1, dim + 1), whose
  last column is the offset, as SciPy takes them.  The output has the input's
  shape and dtype.  One kernel forms the source coordinate of every output voxel
  from the matrix (products added in axis order, the offset last: SciPy's
  rounding) and samples the image there; no coordinate map is built.  Orders,
  the switch for orders 2 to 5, `mode` and `cval` as in `ndimage_warp`.  Not
  covered: `output_shape`, `output`, and 1-D (diagonal) matrices, which SciPy
  sends down its separate zoom-and-shift route; they raise NotImplementedError.
  `image` may be resident (a CUDA tensor or a DeviceArray) and `device_output`
  chooses a DeviceArray or a NumPy result, as in `ndimage_warp`.
  """
  image = _resident(image)
  img_dtype = _np_dtype(image, 'affine_transform')
  dim = image.ndim
  if output_shape is not None or output is not None:
    raise NotImplementedError('affine_transform: output_shape and output')
  if dim not in (2, 3):
    raise ValueError(f'affine_transform: {dim}-d data')
  matrix = np.asarray(matrix, dtype=np.float64)
  if matrix.ndim == 1:
    raise NotImplementedError('affine_transform: 1-d (diagonal) matrices')
  if matrix.shape in ((dim + 1, dim + 1), (dim, dim + 1)):
    if matrix.shape[0] == dim + 1:
      expected = [0.0] * dim + [1.0]
      if not np.all(matrix[dim] == expected):
        raise ValueError(f'Expected homogeneous transformation matrix with shape '
                         f'{matrix.shape} for image shape {tuple(image.shape)}, but bottom row was '
                         f'not equal to {expected}')
    offset = matrix[:dim, dim]
    matrix = matrix[:dim, :dim]
  elif matrix.shape != (dim, dim):
    raise RuntimeError(f'affine_transform: matrix shape {matrix.shape} for {dim}-d data')
  offset = np.asarray(offset, dtype=np.float64)
  if offset.ndim == 0:
    offset = np.full(dim, float(offset))
  if offset.shape != (dim,):
    raise RuntimeError('offset shape not correct')
  if img_dtype == np.uint64:
    raise NotImplementedError('affine_transform: uint64 label volumes')
  _spline.check_order(order, 'affine_transform')
  mode_id, cval = _boundary('affine_transform', mode, cval, order, img_dtype)
  dtype, view = _image_dtype(img_dtype, 'affine_transform')
  if device_output is None:
    device_output = isinstance(image, torch.Tensor)

  dev = _dev.device()
  img_t = _image_tensor(image, view, dev)
  out_t = torch.empty(tuple(image.shape), dtype=img_t.dtype, device=dev)
  shape = (1,) * (3 - dim) + tuple(image.shape)
  full = np.zeros((3, 3), np.float64)
  full[3 - dim:, 3 - dim:] = matrix
  d = _abi.SfmAffineWarpDesc()
  d.ndim = dim
  d.dtype = dtype
  d.order = int(order)
  d.mode = mode_id
  d.shape = (C.c_int32 * 3)(*shape)
  d.matrix = (C.c_double * 9)(*full.ravel())
  d.offset = (C.c_double * 3)(*((0.0,) * (3 - dim) + tuple(float(v) for v in offset)))
  d.cval = cval
  d.image = img_t.data_ptr()
  d.out = out_t.data_ptr()
  d.stream = _dev.stream_ptr()
  coeffs = _sample_coefficients(d, shape, img_dtype, dev, mode, cval)
  _abi.check(_abi.load().sfm_affine_warp(C.byref(d)))
  del coeffs    # (read by the launch above; the stream orders its release)
  return _warped(out_t, img_dtype, device_output)


_POINT_DTYPES = {np.dtype(np.float32): _abi.POINT_F32, np.dtype(np.float64): _abi.POINT_F64,
                 np.dtype(np.int32): _abi.POINT_I32, np.dtype(np.int64): _abi.POINT_I64}


def warp_points(points: np.ndarray, coord_map, map_box, stride: float) -> np.ndarray:
  """Warps a collection of points (warp.py:541-605).

  points: [n, 3] in xyz order (float32, float64, int32 or int64; other integer
  dtypes are computed as int64 and cast back); coord_map: [2, z, y, x]
  relative map (NumPy, torch or DeviceArray, float32 or float64); map_box: the
  map's box (`.start` / `.size` in xyz, or a (start, size) pair); stride: map
  stride in pixels, a scalar.  Returns a NumPy array of the points' dtype: z
  unchanged, x and y mapped; integer dtypes are rounded half to even.

  Only in-plane warping, like the reference.  A point's section is
  `int(z - map_box.start[2])`, indexed like NumPy (negative values wrap,
  anything outside [-nz, nz) raises IndexError, checked before the launch).
  Each of the four nodes around the point is the absolute map value, rounded
  twice in the map's dtype as the reference's `to_absolute` and `+= origin` do;
  they are combined with bilinear weights in float64 in the order of SciPy's
  RegularGridInterpolator (linear extrapolation from the edge cell outside the
  grid) and narrowed to float32.  Nothing per section is materialised.
  """
  points = np.array(points)
  assert points.ndim == 2
  assert points.shape[1] == 3
  dev = _dev.device()
  m = map_utils._device_map(coord_map, dev)
  assert m.shape[0] == 2
  nz, ny, nx = (int(v) for v in m.shape[1:])
  if ny < 2 or nx < 2:
    raise ValueError(
        f'There are {min(ny, nx)} points and at least 2 are required in '
        f'dimension {0 if ny < 2 else 1}')
  stride = float(stride)
  if not (np.isfinite(stride) and stride > 0):
    raise ValueError('The points in dimension 0 must be strictly ascending')
  ret = points.copy()
  n = points.shape[0]
  if n == 0:
    return ret
  map_start, _ = _box(map_box)
  map_start = [int(v) for v in map_start[:3]]

  dtype = points.dtype
  if dtype not in _POINT_DTYPES:
    if not np.issubdtype(dtype, np.integer):
      raise NotImplementedError(f'warp_points: {dtype} points')
    points = points.astype(np.int64)
  # section of every point: int(z - start) of a NumPy scalar and an int64 start
  # (float32 z is widened to float64 first), then Python indexing
  z = points[:, 2]
  if np.issubdtype(z.dtype, np.integer):
    z_rel = z.astype(np.int64) - map_start[2]
  else:
    dz = z.astype(np.float64) - np.float64(map_start[2])
    if not np.all(np.isfinite(dz)):
      raise ValueError('cannot convert float NaN or infinity to integer')
    outside = np.abs(dz) >= 2.0**31
    if outside.any():
      raise IndexError(f'index {int(dz[outside][0])} is out of bounds for axis 1 with size {nz}')
    z_rel = np.trunc(dz).astype(np.int64)
  bad = (z_rel < -nz) | (z_rel >= nz)
  if bad.any():
    raise IndexError(
        f'index {int(z_rel[bad][0])} is out of bounds for axis 1 with size {nz}')
  z_rel = np.where(z_rel < 0, z_rel + nz, z_rel).astype(np.int32)

  pts_t = _dev.upload(np.ascontiguousarray(points), dev)
  sec_t = _dev.upload(np.ascontiguousarray(z_rel), dev)
  out_t = pts_t.clone()
  d = _abi.SfmWarpPointsDesc()
  d.f64 = int(m.dtype == torch.float64)
  d.point_dtype = _POINT_DTYPES[points.dtype]
  d.shape = (C.c_int32 * 3)(nz, ny, nx)
  d.n = n
  d.stride = stride
  d.origin = (C.c_double * 2)(float(np.float64(map_start[0]) * stride),
                              float(np.float64(map_start[1]) * stride))
  d.grid_start = (C.c_int64 * 2)(map_start[0], map_start[1])
  d.coord_map = m.data_ptr()
  d.points = pts_t.data_ptr()
  d.section = sec_t.data_ptr()
  d.out = out_t.data_ptr()
  d.stream = _dev.stream_ptr()
  _abi.check(_abi.load().sfm_warp_points(C.byref(d)))
  ret[...] = out_t.cpu().numpy().astype(dtype, copy=False)
  return ret
