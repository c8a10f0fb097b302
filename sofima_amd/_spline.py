"""B-spline coefficients on the device (sfm_spline_prefilter): the prefilter that
`scipy.ndimage.map_coordinates` runs before it samples with an order above 1,
shared by `warp.ndimage_warp` and `processor_warp.render`.

Orders 2 to 5 are opt-in: the switch SFM_SPLINE_ORDERS=1 (`_abi.set_option`, or
the environment variable as the default) turns them on.  Without it the two
functions behave as they did before these orders were built and raise
NotImplementedError for them, which callers and tests rely on; with it a call
claims a float64 workspace of 8 bytes per voxel.

At these orders the boundary modes 'constant', 'mirror' and 'wrap' share one
prefilter.  SciPy's other modes -- 'nearest', 'reflect' ('grid-mirror'),
'grid-constant' and 'grid-wrap' -- use other initialisations of the recursion, and
'nearest' and 'grid-constant' filter the image padded by 12 samples per axis
(sfm_spline_prefilter_mode).  They are opt-in as well, behind a
switch of their own, SFM_SPLINE_MODES=1, which lifts the mode restriction only:
the order switch is still needed.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np
import torch

from . import _abi
from . import _dev

ORDERS = (2, 3, 4, 5)
OPTION = 'SFM_SPLINE_ORDERS'
MODES_OPTION = 'SFM_SPLINE_MODES'
MIRROR_MODES = ('constant', 'mirror', 'wrap')     # the modes of sfm_spline_prefilter
# initialisations whose SfmSplineItem.zn is pow(pole, len), not pow(pole, len - 1)
_REFLECT_MODES = ('reflect', 'grid-mirror', 'nearest')


def enabled() -> bool:
  return _abi.get_option(OPTION) not in (None, '', '0')


def modes_enabled() -> bool:
  return _abi.get_option(MODES_OPTION) not in (None, '', '0')


def check_mode(mode, order, what: str) -> None:
  """Orders 2 to 5: 'constant', 'mirror' and 'wrap' always, SciPy's other modes with
  the switch SFM_SPLINE_MODES; NotImplementedError otherwise."""
  if order not in ORDERS or mode in MIRROR_MODES or modes_enabled():
    return
  raise NotImplementedError(
      f'{what}: boundary mode {mode!r} at interpolation order {order} (orders 2 to 5 take '
      "'constant', 'mirror' and 'wrap'; the other modes need another B-spline prefilter, "
      f'which the switch {MODES_OPTION}=1 turns on, see sofima_amd._abi.set_option)')


def mode_pad(mode: str) -> int:
  """Samples that SciPy pads the image by, per axis, before it filters for `mode`."""
  pad = _abi.load().sfm_spline_mode_pad(_abi.MODES[mode])
  _abi.check(min(pad, 0))
  return pad


def pad_value(cval, np_dtype) -> float:
  """`cval` as np.pad stores it in an array of the image's type: what SciPy's padded
  image holds around the data under 'grid-constant'."""
  a = np.empty(1, np.dtype(np_dtype))
  with np.errstate(all='ignore'):
    a[...] = np.float64(cval)
  return float(a[0])


def check_order(order, what: str) -> None:
  """Orders 0 and 1 always; 2 to 5 with the switch; NotImplementedError otherwise."""
  if order in (0, 1) or (order in ORDERS and enabled()):
    return
  if order in ORDERS:
    raise NotImplementedError(
        f'{what}: interpolation order {order} (0 and 1 are built in; orders 2 to 5 need the '
        f'switch {OPTION}=1, see sofima_amd._abi.set_option)')
  raise NotImplementedError(f'{what}: interpolation order {order} (0 to 5 are built)')


# SciPy's literals (ni_splines.c); the library holds the same ones.  Here they only
# form pow(pole, len - 1) with the host's libm, which the device cannot reproduce.
_POLES = {
    2: (-0.171572875253809902396622551580603843,),
    3: (-0.267949192431122706472553658494127633,),
    4: (-0.361341225900220177092212841325675255, -0.013725429297339121360331226939128204),
    5: (-0.430575347099973791851434783493520110, -0.043096288203264653822712376822550182),
}
WORKSPACE_FRACTION = 0.6   # of the HBM that is free when the call is planned
SMALL_WORKSPACE = 1 << 30  # requests below this are not checked against the budget


def workspace(n_voxels: int, dev) -> torch.Tensor:
  """float64 tensor of one coefficient per voxel.  A request beyond the budget (a
  fraction of the free HBM, as flow_field sizes its workspace) raises: the
  coefficients of an image cannot be computed in parts."""
  need = 8 * int(n_voxels)
  if need > SMALL_WORKSPACE:
    free, _ = torch.cuda.mem_get_info(dev)
    cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    budget = int(WORKSPACE_FRACTION * (free + max(cached, 0)))
    if need > budget:
      raise MemoryError(
          f'spline prefilter: {need} bytes of coefficients for {n_voxels} voxels exceed the '
          f'workspace budget of {budget} bytes')
  return torch.empty(max(int(n_voxels), 1), dtype=torch.float64, device=dev)


def prefilter(regions: Sequence[tuple[int, Sequence[int], Sequence[int]]], dtype: int,
              order: int, dev, mode: str = 'constant', ndim: int = 3,
              pad_value: float = 0.0) -> tuple[torch.Tensor, list[int]]:
  """Coefficients of every region, dense and back to back in one workspace.

  regions: (device address of the region's first element, zyx shape, zyx element
  pitch within its array) per region; dtype: _abi.DTYPE_* of all of them.  One
  batch of launches (one per axis) for the whole table.  Returns the workspace
  and the element offset of every region in it.

  mode: the boundary mode the coefficients will be sampled under; 'constant',
  'mirror' and 'wrap' are the default prefilter, the others
  sfm_spline_prefilter_mode.  ndim: the real dimensionality of the regions (2:
  shape[0] is 1).  Under 'nearest' and 'grid-constant' the coefficients of a
  region are those of the region padded by `mode_pad(mode)` samples on each of
  its `ndim` axes, dense in the padded shape; `pad_value` is what 'grid-constant'
  pads with (`pad_value(cval, dtype)`).
  """
  assert order in ORDERS
  pad = 0 if mode in MIRROR_MODES else mode_pad(mode)
  power = 0 if mode in _REFLECT_MODES else 1
  table = (_abi.SfmSplineItem * max(len(regions), 1))()
  offsets, total = [], 0
  for it, (ptr, shape, pitch) in zip(table, regions):
    shape = tuple(int(v) for v in shape)
    assert len(shape) == 3 and all(v >= 1 for v in shape)
    it.image = ptr
    it.shape = (C.c_int32 * 3)(*shape)
    it.pitch = (C.c_int64 * 3)(*(int(v) for v in pitch))
    it.coeff_offset = total
    shape = tuple(n + (2 * pad if k >= 3 - ndim else 0) for k, n in enumerate(shape))
    for k, n in enumerate(shape):
      for p, z in enumerate(_POLES[order]):
        it.zn[k][p] = math.pow(z, n - power)
    offsets.append(total)
    total += shape[0] * shape[1] * shape[2]
  ws = workspace(total, dev)
  if not regions:
    return ws, offsets
  table_t = _dev.upload(np.frombuffer(table, dtype=np.uint8).copy(), dev)
  d = _abi.SfmSplinePrefilterDesc()
  d.dtype = dtype
  d.order = int(order)
  d.n_items = len(regions)
  d.items_host = table
  d.items = table_t.data_ptr()
  d.coeffs = ws.data_ptr()
  d.coeffs_len = total
  d.stream = _dev.stream_ptr()
  if mode in MIRROR_MODES:
    _abi.check(_abi.load().sfm_spline_prefilter(C.byref(d)))
  else:
    _abi.check(_abi.load().sfm_spline_prefilter_mode(C.byref(d), _abi.MODES[mode], int(ndim),
                                                     float(pad_value)))
  # (table_t is read by launches that are enqueued, not finished: the caching
  # allocator reuses its block only for work on the same stream, behind them)
  return ws, offsets
