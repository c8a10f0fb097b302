"""Flow-field clean-up on MI355X.

Drop-ins for `flow_utils.clean_flow` (flow_utils.py:37-78), the quality
filter between flow estimation and mesh relaxation, and
`flow_utils.reconcile_flows` (flow_utils.py:81-135), which merges flows and
filters them before the mesh solve.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _abi
from . import _dev
from ._dev import DeviceArray


def clean_flow(flow, min_peak_ratio: float, min_peak_sharpness: float,
               max_magnitude: float, max_deviation: float,
               dim: int = 2) -> DeviceArray:
  """Removes flow vectors that do not fulfill quality requirements.

  Same contract as the reference: `flow` is [c, z, y, x] with c = dim (vectors
  only) .. dim + 2 (vectors, peak sharpness, peak ratio); the result is the
  [dim, z, y, x] vector field with NaN where the sharpness / ratio / magnitude
  / deviation-from-the-3x3(x3)-median criteria fail.  Accepts NumPy arrays,
  torch tensors or DeviceArrays; the result stays on the device (np.asarray()
  copies it back) and is computed in float32.  The thresholds compare as in
  NumPy: in float32 against a Python number or float32 scalar, in float64
  against a float64 scalar (see `_f32_threshold`).
  """
  assert dim in (2, 3)
  dev = _dev.device()
  f = _dev.as_device_f32(flow, dev, copy=False)
  if f.ndim != 4:
    raise ValueError('flow must be [c, z, y, x]')
  assert dim <= f.shape[0] <= dim + 2
  d = _abi.SfmCleanFlowDesc()
  d.dim = dim
  d.channels = f.shape[0]
  d.shape = (C.c_int32 * 3)(*f.shape[1:])
  (d.min_peak_ratio, d.min_peak_sharpness, d.max_magnitude,
   d.max_deviation) = _clean_thresholds(min_peak_ratio, min_peak_sharpness, max_magnitude,
                                        max_deviation)
  d.flow = f.data_ptr()
  d.stream = _dev.stream_ptr()
  out = torch.empty((dim,) + tuple(f.shape[1:]), dtype=torch.float32, device=dev)
  _abi.check(_abi.load().sfm_clean_flow(C.byref(d), out.data_ptr()))
  return DeviceArray(out)


def _f32_threshold(t) -> float:
  """The double to compare a float32 quantity with so that the result is NumPy's
  `float32_array > t`: a Python number or a float32 / float16 scalar is cast to
  float32 first (NEP 50), a float64 (or int64) scalar compares in float64."""
  if np.result_type(np.float32, t) == np.float32:
    return float(np.float32(t))
  return float(t)


def _positive_f32_threshold(t) -> float:
  """`_f32_threshold` of a limit that is applied only when it is > 0.  A positive
  threshold that float32 rounds to 0 still enables the test: for a float32 x,
  `x > 0` is `x > 5e-324` in double."""
  return max(_f32_threshold(t), 5e-324) if t > 0 else 0.0


def _clean_thresholds(min_peak_ratio, min_peak_sharpness, max_magnitude, max_deviation):
  """clean_flow's thresholds as the doubles SfmCleanFlowDesc carries."""
  return (_f32_threshold(min_peak_ratio), _f32_threshold(min_peak_sharpness),
          _positive_f32_threshold(max_magnitude), _positive_f32_threshold(max_deviation))


def _reconcile_thresholds(max_gradient, max_deviation, min_patch_size, min_delta_z=0):
  """reconcile_flows' thresholds as SfmReconcileDesc carries them."""
  return (
      # np.diff's zero padding makes the gradient float64 whatever the threshold
      float(max_gradient) if max_gradient > 0 else 0.0,
      _positive_f32_threshold(max_deviation),
      # integer sizes: size < m <=> size < ceil(m)
      max(0, min(int(math.ceil(min_patch_size)), 2**62)),
      _f32_threshold(min_delta_z))


def reconcile_flows(flows, max_gradient: float, max_deviation: float,
                    min_patch_size: int, min_delta_z: float = 0) -> DeviceArray:
  """Reconciles multiple flows.

  Same contract as the reference: `flows` is a sequence of [c, z, y, x] flows
  (c = 2 or 3, all of one shape), or one [K, c, z, y, x] array, in order of
  decreasing preference; later flows fill where the merged channel 0 is NaN
  (for c = 3 only where |dz| >= `min_delta_z`), then vectors are invalidated where the gradient of channel
  0 / 1 exceeds `max_gradient`, where channel 0 / 1 deviates from the 3 x 3
  median by more than `max_deviation`, and where their 4-connected component
  in the z slice has fewer than `min_patch_size` vectors (each test only when
  its threshold is > 0).  Accepts NumPy arrays, torch tensors or DeviceArrays,
  mixed; computes in float32 on the device without modifying the inputs and
  returns a [c, z, y, x] DeviceArray.  The thresholds compare as in NumPy:
  the gradient in float64 (np.diff's zero padding promotes the field), the
  median deviation and |dz| in float32 against a Python number or float32
  scalar and in float64 against a float64 scalar.
  """
  dev = _dev.device()
  if isinstance(flows, (np.ndarray, torch.Tensor, DeviceArray)):
    # one stacked array holds the K flows along its first axis
    if len(flows.shape) != 5:
      raise ValueError('a single array of flows must be [K, c, z, y, x]')
    packed = _dev.as_device_f32(flows, dev, copy=False)
    shape = tuple(packed.shape[1:])
  else:
    flows = list(flows)
    if not flows:
      raise ValueError('flows must hold at least one flow')
    ts = [_dev.as_device_f32(f, dev, copy=False) for f in flows]
    shape = tuple(ts[0].shape)
    if any(tuple(t.shape) != shape for t in ts):
      raise ValueError('all flows must have the same shape')
    # [K, c, z, y, x]; one flow is passed as it is (never written)
    packed = ts[0][None] if len(ts) == 1 else torch.stack(ts)
  if len(shape) != 4 or shape[0] not in (2, 3) or min(shape) < 1 or packed.shape[0] < 1:
    raise ValueError(f'flows must be [c, z, y, x] with c in (2, 3), got {shape}')
  d = _abi.SfmReconcileDesc()
  d.channels = shape[0]
  d.shape = (C.c_int32 * 3)(*shape[1:])
  d.num_flows = packed.shape[0]
  (d.max_gradient, d.max_deviation, d.min_patch_size,
   d.min_delta_z) = _reconcile_thresholds(max_gradient, max_deviation, min_patch_size,
                                          min_delta_z)
  d.flows = packed.data_ptr()
  lib = _abi.load()
  nbytes = lib.sfm_reconcile_flows_workspace_bytes(C.byref(d))
  ws = _dev.workspace(nbytes, dev)
  d.workspace = ws.data_ptr()
  d.workspace_bytes = ws.numel()
  d.stream = _dev.stream_ptr()
  out = torch.empty(shape, dtype=torch.float32, device=dev)
  _abi.check(lib.sfm_reconcile_flows(C.byref(d), out.data_ptr()))
  return DeviceArray(out)


def apply_mask(flow: np.ndarray, mask: np.ndarray) -> None:
  """In-place NaN masking of a host flow array (flow_utils.py:32-34)."""
  for i in range(flow.shape[0]):
    flow[i, ...][mask] = np.nan
