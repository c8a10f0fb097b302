"""The array-level warps of the reference's decorators/warp.py on MI355X: the two
functions that sit between coarse (affine) alignment and the elastic pipeline.

`warp_affine` is `_warp_affine` (decorators/warp.py:36-116) and `warp_coord_map`
is `_warp_coord_map` (:221-243); the private names are kept as aliases.  Both take
and return NumPy arrays in xyz axis order, or resident images and maps (CUDA
tensors, DeviceArrays), which stay on the device.  The TensorStore decorator classes
around them (WarpAffine, WarpCoordMap) are volume I/O and are not built.

Pinned: the reference's own functions run through the golden shim
(tests/golden/warp_decorators.npz) and these reproduce their output bit for bit
(tests/test_gpu_decorators_warp.py).
"""
from __future__ import annotations

import functools
import types
from typing import Optional, Sequence

import numpy as np
import torch

from . import _dev
from . import map_utils
from . import warp
from ._dev import DeviceArray


def warp_affine(img_xyz, matrix_xyz: np.ndarray, order: int = 1,
                implementation: str = 'scipy', device_output: bool | None = None, **warp_args):
  """Warp affine in 2D/3D (decorators/warp.py:36-116).

  img_xyz: 2-D or 3-D uint8 / uint16 / float32 image; matrix_xyz: the forward
  transform, (dim, dim + 1) or its homogeneous form (dim + 1, dim + 1).
  implementation 'scipy': the matrix is inverted on the host (np.linalg.inv, as
  the reference does) and `warp.affine_transform` resamples in one fused kernel.
  'sofima' (3-D only): `map_utils.make_affine_map` at stride 1, then
  `warp.ndimage_warp` of the transposed image, both on the device: the map goes
  from one to the other as the DeviceArray it is; `warp_args` go to
  `ndimage_warp`.  The image may be resident (a CUDA tensor or a DeviceArray); it
  is then transposed on the device and the result is a contiguous DeviceArray;
  device_output: as in `warp.ndimage_warp`.  'opencv' needs cv2, which is
  neither available nor pinned here (like `warp.warp_subvolume`'s resampling),
  and raises NotImplementedError.
  """
  img_xyz = warp._resident(img_xyz)
  matrix_xyz = np.asarray(matrix_xyz)
  dim = img_xyz.ndim
  if dim not in (2, 3):
    raise ValueError(f'2 or 3 image dimensions are required, but got {dim}.')
  if matrix_xyz.ndim != 2:
    raise ValueError(f'2 matrix dimensions are required, but got {matrix_xyz.ndim}.')
  rows, cols = matrix_xyz.shape
  if cols != dim + 1:
    raise ValueError(f'{dim + 1} matrix cols are required, but got {cols}.')
  if rows not in (dim, dim + 1):
    raise ValueError(f'{dim} or {dim + 1} matrix rows are required, but got {rows}.')
  homogeneous = np.eye(dim + 1)
  homogeneous[:rows] = matrix_xyz

  if implementation == 'opencv':
    if dim != 2:
      raise RuntimeError('Only 2D images are supported with `implementation=opencv`.')
    raise NotImplementedError(
        'warp_affine: implementation=opencv needs cv2, which is not available here')
  if implementation == 'scipy':
    return warp.affine_transform(img_xyz, np.linalg.inv(homogeneous), order=order,
                                 device_output=device_output)
  if implementation != 'sofima':
    raise ValueError(
        f'implementation must be `opencv`, `scipy`, or `sofima`, but got `{implementation}.')
  if dim != 3:
    raise RuntimeError('Only 3D images are supported with `implementation=sofima`.')
  box = types.SimpleNamespace(start=np.zeros(3, np.int64),
                              size=np.array(tuple(img_xyz.shape), np.int64))
  coord_map = map_utils.make_affine_map(np.linalg.inv(homogeneous)[:3, :], box, [1, 1, 1])
  warp_args.setdefault('work_size', tuple(img_xyz.shape))
  return _transposed(warp.ndimage_warp(
      _transposed(img_xyz), coord_map, stride=[1, 1, 1], order=order, overlap=[0, 0, 0],
      device_output=device_output, **warp_args))


def _transposed(a):
  """xyz <-> zyx: a view of a NumPy array, as the reference takes `.T`; a resident
  image is transposed on the device into a contiguous one."""
  if isinstance(a, DeviceArray):
    return DeviceArray(warp._transpose_resident(a.tensor))
  if isinstance(a, torch.Tensor):
    return warp._transpose_resident(a)
  return a.T


def _scaled_map(coord_map, scale_xyz):
  """coord_map * scale_xyz per channel, in NumPy's result type: a resident map is
  multiplied on the device (float32 x float64 factors widen to float64 first, as
  NumPy promotes them: the same rounding)."""
  scale = np.array(scale_xyz)
  if isinstance(coord_map, DeviceArray):
    coord_map = coord_map.tensor
  if not (isinstance(coord_map, torch.Tensor) and coord_map.is_cuda):
    if isinstance(coord_map, torch.Tensor):
      coord_map = coord_map.numpy()
    return coord_map * scale.reshape(-1, 1, 1, 1)
  if coord_map.dtype not in (torch.float32, torch.float64):
    raise TypeError(f'warp_coord_map: {coord_map.dtype} device maps (float32, float64)')
  own = np.float32 if coord_map.dtype == torch.float32 else np.float64
  res = np.result_type(own, scale.dtype)
  if res not in (np.float32, np.float64):
    raise TypeError(f'warp_coord_map: scale_xyz of dtype {scale.dtype}')
  dt = torch.float32 if res == np.float32 else torch.float64
  # (on the side stream of _dev.upload: a copy from pageable memory on the compute
  # stream would make the host wait for everything launched so far)
  factors = _dev.upload(np.ascontiguousarray(scale.astype(res).reshape(-1, 1, 1, 1)),
                        coord_map.device)
  return coord_map.to(dt) * factors


def warp_coord_map(img_xyz, coord_map, mode: str = 'constant',
                   cval: float | int = 0.0, scale_xyz: Optional[Sequence[float]] = None,
                   device_output: bool | None = None, **warp_args):
  """Warp by coord map in 3D (decorators/warp.py:221-243).

  coord_map: [3, z, y, x] relative map; `mode` / `cval`: SciPy's boundary mode
  and fill value, applied to the map interpolation and to the image sample
  alike (see `warp.ndimage_warp`: orders 2 to 5 take 'constant', 'mirror' and
  'wrap', and the other modes with the switch SFM_SPLINE_MODES=1); scale_xyz:
  factors for the map's channels;
  `warp_args` (stride, overlap, order, boxes ...) go to `warp.ndimage_warp`,
  `work_size` defaults to the image shape.  Image and map may be resident (CUDA
  tensors or DeviceArrays): the `scale_xyz` product and the transposes then run on
  the device, and with device_output (the default for a resident image) the
  result is a contiguous DeviceArray and nothing is copied to the host.
  """
  import scipy.ndimage
  img_xyz = warp._resident(img_xyz)
  if img_xyz.ndim != 3:
    raise RuntimeError('Only 3D images are supported.')
  warp_args.setdefault('work_size', tuple(img_xyz.shape))
  if scale_xyz is not None:
    coord_map = _scaled_map(coord_map, scale_xyz)
  sampler = functools.partial(scipy.ndimage.map_coordinates, cval=cval, mode=mode)
  return _transposed(warp.ndimage_warp(_transposed(img_xyz), coord_map, map_coordinates=sampler,
                                       device_output=device_output, **warp_args))


_warp_affine = warp_affine
_warp_coord_map = warp_coord_map
