"""B-spline coefficients on the device (sfm_spline_prefilter): the prefilter that
`scipy.ndimage.map_coordinates` runs before it samples with an order above 1,
shared by `warp.ndimage_warp` and `processor_warp.render`.

Orders 2 to 5 are opt-in: the switch SFM_SPLINE_ORDERS=1 (`_abi.set_option`, or
the environment variable as the default) turns them on.  Without it the two
functions behave as they did before these orders were built and raise
NotImplementedError for them, which callers and tests rely on; with it a call
claims a float64 workspace of 8 bytes per voxel.
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


def enabled() -> bool:
  return _abi.get_option(OPTION) not in (None, '', '0')


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
              order: int, dev) -> tuple[torch.Tensor, list[int]]:
  """Coefficients of every region, dense and back to back in one workspace.

  regions: (device address of the region's first element, zyx shape, zyx element
  pitch within its array) per region; dtype: _abi.DTYPE_* of all of them.  One
  batch of launches (one per axis) for the whole table.  Returns the workspace
  and the element offset of every region in it.
  """
  assert order in ORDERS
  table = (_abi.SfmSplineItem * max(len(regions), 1))()
  offsets, total = [], 0
  for it, (ptr, shape, pitch) in zip(table, regions):
    shape = tuple(int(v) for v in shape)
    assert len(shape) == 3 and all(v >= 1 for v in shape)
    it.image = ptr
    it.shape = (C.c_int32 * 3)(*shape)
    it.pitch = (C.c_int64 * 3)(*(int(v) for v in pitch))
    it.coeff_offset = total
    for k, n in enumerate(shape):
      for p, z in enumerate(_POLES[order]):
        it.zn[k][p] = math.pow(z, n - 1)
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
  _abi.check(_abi.load().sfm_spline_prefilter(C.byref(d)))
  # (table_t is read by launches that are enqueued, not finished: the caching
  # allocator reuses its block only for work on the same stream, behind them)
  return ws, offsets
