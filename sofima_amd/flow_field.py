"""Flow-field estimation by patch cross-correlation on MI355X.

Drop-in for the reference's `sofima/flow_field.py`: the same public names,
signatures, argument meaning and result layout, with the device work done by
hand-written HIP kernels behind the C ABI of libsofima_amd.so
(include/sofima_amd.h).  There is no JAX and no CPU fallback.

  JAXMaskedXCorrWithStatsCalculator  <-> flow_field.py:449-712
  masked_xcorr                       <-> flow_field.py:36-156
  _batched_peaks                     <-> flow_field.py:205-275
  batched_xcorr_peaks                <-> flow_field.py:374-441

Flow fields are [dim + 2, *grid] float32 with channels x, y[, z], peak
sharpness, peak ratio (vector components in the REVERSE of the image axis
order); NaN marks entries that were not or could not be estimated.

Host-side differences from the reference that do not change results: the start
coordinates of ALL batches are computed up front and uploaded once, the
batches are enqueued back to back on the current HIP stream and read back with
a single copy (the reference blocks on a device->host copy per batch and
scatters results patch by patch in Python).  Batch membership -- which the
reference's results depend on -- is unchanged.
"""
from __future__ import annotations

import collections.abc
import ctypes as C
import itertools
import os
import threading
from typing import Callable, Iterator, Sequence, TypeVar

import numpy as np
import torch

from . import _abi
from . import _dev

T = TypeVar("T")
# The uint8 2-D unmasked path runs on the int8 matrix cores (csrc/sfm_mfma.h).
MFMA_I8_AVAILABLE = True
Array = np.ndarray


def _silent_fn(x: list[T]) -> Iterator[T]:
  for item in x:
    yield item


def _pad3(vals, fill):
  vals = [int(v) for v in vals]
  return [fill] * (3 - len(vals)) + vals


def _i3(vals):
  return (C.c_int32 * 3)(*vals)


# ---------------------------------------------------------------------------
# patch selection helpers (integral image over the mask)
# ---------------------------------------------------------------------------
def _integral_image(mask):
  """Summed-volume table with a zero plane in front of every axis.

  Replaces flow_field._integral_image (flow_field.py:159-175) + the
  `connectomics` integral_image helper.  The table is tiny compared with the
  correlation work and is consumed by host index arithmetic, so it is built
  with NumPy in int64 (the reference switches to int64 for large masks too).
  """
  if mask is None:
    return None
  ii = np.asarray(mask).astype(np.int64)
  for axis in range(ii.ndim):
    ii = np.cumsum(ii, axis=axis)
  return np.pad(ii, [(1, 0)] * ii.ndim)


def _query_integral_image(svt, diam, stride):
  nd = svt.ndim
  hi = [np.s_[diam[i]::stride[i]] for i in range(nd)]
  lo = [np.s_[:-diam[i]:stride[i]] for i in range(nd)]
  total = 0
  for bits in itertools.product((0, 1), repeat=nd):
    sel = tuple(hi[i] if b else lo[i] for i, b in enumerate(bits))
    total = total + (-1) ** (nd - sum(bits)) * svt[sel]
  return total


def _host_masked_counts(mask, patch_size, step):
  """Host form of the patch-selection counts (summed-area table, as in the
  reference): for planning without a GPU (`plan(..., counts_fn=...)`) and as the
  comparison in the tests.  flow_field() never uses it."""
  return _query_integral_image(_integral_image(mask), patch_size, step)


def _masked_counts(mask, patch_size, step, on_device=False):
  """Number of masked pixels in every grid patch, [*(shape - patch)//step + 1].

  Device replacement for `_integral_image` + the summed-area-table query of
  the reference (flow_field.py:575-589): `sfm_mask_patch_counts`.  Needs the
  GPU like every other compute step (no fallback).
  """
  dev = _dev.device()
  m = _dev.as_device_mask(mask, dev)
  nd = m.ndim
  d = _abi.SfmMaskCountDesc()
  d.ndim = nd
  d.shape = _i3(_pad3(m.shape, 1))
  d.patch = _i3(_pad3(patch_size, 1))
  d.step = _i3(_pad3(step, 1))
  d.mask = m.data_ptr()
  d.stream = _dev.stream_ptr()
  grid = [(int(s) - int(p)) // int(t) + 1
          for s, p, t in zip(m.shape, patch_size, step)]
  out = torch.empty(grid, dtype=torch.int32, device=dev)
  _abi.check(_abi.load().sfm_mask_patch_counts(C.byref(d), out.data_ptr()))
  return out if on_device else out.cpu().numpy()


# ---------------------------------------------------------------------------
# C-ABI call helpers
# ---------------------------------------------------------------------------
class _Resident:
  """Images / masks of one flow_field() call, resident in HBM."""

  def __init__(self, pre_image, post_image, pre_mask, post_mask, dev):
    self.dev = dev
    self.pre, self.dtype = _dev.as_device_image(pre_image, dev)
    self.post, dt2 = _dev.as_device_image(post_image, dev)
    if dt2 != self.dtype:
      # Mixed inputs: correlate in float32.
      self.pre = self.pre.to(torch.float32)
      self.post = self.post.to(torch.float32)
      self.dtype = _abi.DTYPE_F32
    self.pre_mask = _dev.as_device_mask(pre_mask, dev)
    self.post_mask = _dev.as_device_mask(post_mask, dev)
    self.ndim = self.pre.ndim

  @classmethod
  def of_device(cls, pre, post, pre_mask, post_mask, dtype, dev):
    """From tensors that are already what __init__ would make of them:
    contiguous device images of one dtype (tag `dtype`), uint8 masks or None.
    Nothing is converted or copied."""
    res = cls.__new__(cls)
    res.dev = dev
    res.pre, res.post, res.dtype = pre, post, dtype
    res.pre_mask, res.post_mask = pre_mask, post_mask
    res.ndim = pre.ndim
    return res


def _make_desc(res: _Resident, patch_size, post_patch_size, mean, min_distance,
               threshold_rel, peak_radius, method) -> _abi.SfmXcorrDesc:
  nd = res.ndim
  d = _abi.SfmXcorrDesc()
  d.ndim = nd
  d.dtype = res.dtype
  d.pre_image = res.pre.data_ptr()
  d.post_image = res.post.data_ptr()
  d.pre_shape = _i3(_pad3(res.pre.shape, 1))
  d.post_shape = _i3(_pad3(res.post.shape, 1))
  if res.pre_mask is not None:
    d.pre_mask = res.pre_mask.data_ptr()
    d.pre_mask_shape = _i3(_pad3(res.pre_mask.shape, 1))
  if res.post_mask is not None:
    d.post_mask = res.post_mask.data_ptr()
    d.post_mask_shape = _i3(_pad3(res.post_mask.shape, 1))
  d.patch = _i3(_pad3(patch_size, 1))
  d.post_patch = _i3(_pad3(post_patch_size, 1))
  d.use_mean = 0 if mean is None else 1
  d.mean = 0.0 if mean is None else float(mean)
  if isinstance(min_distance, collections.abc.Sequence):
    # The reference leaves `size` undefined for sequences (flow_field.py:232).
    raise NotImplementedError('min_distance must be a scalar')
  d.min_distance = int(min_distance)
  d.threshold_rel = float(threshold_rel)
  if not isinstance(peak_radius, collections.abc.Sequence):
    peak_radius = (peak_radius,) * nd
  d.peak_radius = _i3(_pad3([int(r) for r in peak_radius], 0))
  d.method = method
  d.stream = _dev.stream_ptr()
  return d


# Patches per C call (a multiple of the reference batch is used).  One launch
# carries a whole 8192^2 section pair (40401 patches of 160^2, 26 GB of
# workspace -- sized for the 288 GB of an MI355X): every launch ends with a
# tail in which the CUs run dry one by one (the slower workgroup of a CU needs
# ~400 us per patch), so 1 launch instead of 10 is worth 3-4 % (22.8 vs 23.7 ms).
LAUNCH_PATCHES = int(os.environ.get('SFM_LAUNCH_PATCHES', '45056'))
_FITTED = {}              # (device index, fraction) -> largest workspace that passed the budget check
WORKSPACE_FRACTION = 0.6  # of the HBM that is free when a call is planned
SMALL_WORKSPACE = 1 << 30  # calls below this are not checked against the budget


def _workspace_budget(dev) -> int:
  """Bytes one flow_field() call may claim as workspace: a fraction of what
  the driver reports free plus what torch's caching allocator holds unused."""
  free, _ = torch.cuda.mem_get_info(dev)
  cached = torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
  return int(WORKSPACE_FRACTION * (free + max(cached, 0)))


def _fitted_key(dev):
  return (torch.device(dev).index, WORKSPACE_FRACTION)


def _size_call(desc: _abi.SfmXcorrDesc, batch_size: int, per_call: int, dev):
  """(reference batches per C call, workspace bytes of such a call), at most
  `per_call` batches.  The workspace grows with patches x surface area (26 GB for
  a whole 8192^2 pair of 160^2 patches), so the call size is halved until its
  workspace fits a fraction of the memory that is free right now (other ranks /
  threads / jobs may share the GPU)."""
  lib = _abi.load()
  budget = None
  while True:
    desc.batch = per_call * batch_size
    need = lib.sfm_xcorr_workspace_bytes(C.byref(desc))
    if need == 0:
      _abi.check(-1)
    # (the allocator statistics behind the budget cost 0.2 ms: asked for only
    # when a call wants more than SMALL_WORKSPACE)
    if per_call == 1 or need <= SMALL_WORKSPACE:
      return per_call, need
    # (nor when a workspace of at least this size passed the check on this device
    # before: the production loop asks for the same bytes section after section,
    # and torch's caching allocator still holds the block)
    if need <= _FITTED.get(_fitted_key(dev), 0):
      return per_call, need
    if budget is None:
      budget = _workspace_budget(dev)
    if need <= budget:
      _FITTED[_fitted_key(dev)] = max(_FITTED.get(_fitted_key(dev), 0), need)
      return per_call, need
    per_call //= 2


def _run_batches_dev(res: _Resident, desc: _abi.SfmXcorrDesc, starts: torch.Tensor,
                     batch_size: int, progress_fn=None) -> torch.Tensor:
  """Enqueues every batch on the current stream; `starts` is the device tensor
  [2, n, dim] of pre / post start coordinates.  Returns the device peaks
  [n, dim + 2]."""
  lib = _abi.load()
  nd = res.ndim
  n = starts.shape[1]
  assert n % batch_size == 0
  n_batches = n // batch_size
  peaks = torch.empty((n, nd + 2), dtype=torch.float32, device=res.dev)
  # One C call carries several reference batches (`group` rows each keep the
  # batch-coupled behaviours): fewer, larger launches fill the chip even when
  # the reference batch is small.  LAUNCH_PATCHES is an upper bound only.
  desc.group = batch_size
  desc.pre_starts = starts.data_ptr()
  desc.post_starts = starts.data_ptr()
  per_call = min(max(1, LAUNCH_PATCHES // batch_size), n_batches)
  while True:
    per_call, need = _size_call(desc, batch_size, per_call, res.dev)
    try:
      ws = _dev.workspace(need, res.dev)
      break
    except torch.OutOfMemoryError:
      # a size that passed the budget earlier (_FITTED) no longer fits: memory
      # pressure grew or the cached block was released.  Forget it and go on
      # with smaller calls -- the field is the same.
      _FITTED.pop(_fitted_key(res.dev), None)
      if per_call == 1:
        raise
      per_call //= 2
  desc.workspace = ws.data_ptr()
  desc.workspace_bytes = ws.numel()
  desc.stream = torch.cuda.current_stream(res.dev).cuda_stream
  row_bytes = batch_size * nd * 4
  it = iter(range(n_batches) if progress_fn is None else progress_fn)
  for bi in range(0, n_batches, per_call):
    nb = min(per_call, n_batches - bi)
    desc.batch = nb * batch_size
    desc.pre_starts = starts.data_ptr() + bi * row_bytes
    desc.post_starts = starts.data_ptr() + (n_batches + bi) * row_bytes
    out_ptr = peaks.data_ptr() + bi * batch_size * (nd + 2) * 4
    _abi.check(lib.sfm_xcorr_peaks(C.byref(desc), out_ptr))
    for _ in range(nb):
      next(it, None)
  return peaks


def _run_batches(res: _Resident, desc: _abi.SfmXcorrDesc, pre_starts: np.ndarray,
                 post_starts: np.ndarray, batch_size: int,
                 progress_fn=None, starts_cache=None) -> np.ndarray:
  """Host-array form: uploads the start coordinates (or reuses the cached
  device copy) and returns peaks [n_batches * batch_size, dim + 2] on the host."""
  starts = None if starts_cache is None else starts_cache.get(res.dev)
  if starts is None:
    starts = torch.from_numpy(
        np.ascontiguousarray(
            np.stack([pre_starts, post_starts]).astype(np.int32))).to(res.dev)
    if starts_cache is not None:
      starts_cache[res.dev] = starts
  return _run_batches_dev(res, desc, starts, batch_size, progress_fn).cpu().numpy()


# ---------------------------------------------------------------------------
# public: functions taking pre-extracted patches / surfaces
# ---------------------------------------------------------------------------
def masked_xcorr(prev: Array, curr: Array, prev_mask: Array | None = None,
                 curr_mask: Array | None = None, use_jax: bool = False,
                 dim: int = 2, method: int = _abi.XCORR_AUTO,
                 mean: float | None = 0.0) -> np.ndarray:
  """Cross-correlation between two (masked) image batches.

  Same contract as flow_field.masked_xcorr (flow_field.py:36-156): full linear
  correlation over the last `dim` axes (leading axes are batch); RAW values
  without masks, Padfield-normalised values in [-1, 1] with masks; the
  normalisation tolerances use maxima over the whole batch.  `use_jax` is
  accepted for signature compatibility; the computation always runs on the
  GPU in float32.  `mean` (an extension) is subtracted from both inputs first:
  0.0 = the reference's behaviour (inputs are used as they are), None = every
  patch's own mean like `_batched_xcorr` does (flow_field.py:340-353).
  """
  del use_jax
  dev = _dev.device()
  prev = np.asarray(prev)
  curr = np.asarray(curr)
  if dim not in (2, 3):
    raise NotImplementedError('dim must be 2 or 3')
  lead = prev.shape[:-dim]
  if curr.shape[:-dim] != lead:
    raise ValueError('prev and curr need identical batch dimensions')
  b = int(np.prod(lead)) if lead else 1
  p = prev.shape[-dim:]
  q = curr.shape[-dim:]

  def stack(a, sz):
    if a is None:
      return None
    a = np.asarray(a).reshape((b * sz[0],) + tuple(sz[1:]))
    return a

  if prev_mask is not None:
    prev_mask = np.broadcast_to(np.asarray(prev_mask), prev.shape)
  if curr_mask is not None:
    curr_mask = np.broadcast_to(np.asarray(curr_mask), curr.shape)
  if not (prev.dtype == np.uint8 and curr.dtype == np.uint8):
    # uint8 batches stay uint8 (eligible for the matrix-core kernel)
    prev = prev.astype(np.float32, copy=False)
    curr = curr.astype(np.float32, copy=False)
  res = _Resident(stack(prev, p), stack(curr, q),
                  stack(prev_mask, p), stack(curr_mask, q), dev)
  desc = _make_desc(res, p, q, mean, 2, 0.5, 5, method)
  st_pre = np.zeros((b, dim), np.int32)
  st_post = np.zeros((b, dim), np.int32)
  st_pre[:, 0] = np.arange(b) * p[0]
  st_post[:, 0] = np.arange(b) * q[0]
  starts = torch.from_numpy(np.stack([st_pre, st_post])).to(dev)
  desc.batch = b
  desc.pre_starts = starts.data_ptr()
  desc.post_starts = starts.data_ptr() + b * dim * 4
  lib = _abi.load()
  need = lib.sfm_xcorr_workspace_bytes(C.byref(desc))
  ws = _dev.workspace(need, dev)
  desc.workspace = ws.data_ptr()
  desc.workspace_bytes = ws.numel()
  s = tuple(int(a + c - 1) for a, c in zip(p, q))
  out = torch.empty((b,) + s, dtype=torch.float32, device=dev)
  _abi.check(lib.sfm_xcorr_surface(C.byref(desc), out.data_ptr()))
  return out.cpu().numpy().reshape(tuple(lead) + s)


def _batched_peaks(img, center_offset, min_distance: int, threshold_rel: float,
                   peak_radius: int | Sequence[int] = 5) -> np.ndarray:
  """Peak statistics for a batch of correlation surfaces -> [b, dim + 2].

  Same contract as flow_field._batched_peaks (flow_field.py:205-275),
  including its batch-coupled second-peak suppression.  A surface that holds a
  NaN has a NaN row, like the reference's; negative `min_distance` or
  `peak_radius` raise ValueError.
  """
  if not isinstance(min_distance, collections.abc.Sequence) and int(min_distance) < 0:
    raise ValueError(f'min_distance must be >= 0, got {min_distance}')
  radii = peak_radius if isinstance(peak_radius, collections.abc.Sequence) else (peak_radius,)
  if any(int(r) < 0 for r in radii):
    raise ValueError(f'peak_radius must be >= 0, got {peak_radius}')
  dev = _dev.device()
  surf = _dev.as_device_f32(img, dev, copy=False)
  dim = surf.ndim - 1
  if dim not in (2, 3):
    raise NotImplementedError('surfaces must be 2-D or 3-D')
  if isinstance(min_distance, collections.abc.Sequence):
    raise NotImplementedError('min_distance must be a scalar')
  if not isinstance(peak_radius, collections.abc.Sequence):
    peak_radius = (peak_radius,) * dim
  d = _abi.SfmPeaksDesc()
  d.ndim = dim
  d.batch = surf.shape[0]
  d.shape = _i3(_pad3(surf.shape[1:], 1))
  d.center_offset = (C.c_float * 3)(
      *([0.0] * (3 - dim) + [float(c) for c in center_offset]))
  d.min_distance = int(min_distance)
  d.threshold_rel = float(threshold_rel)
  d.peak_radius = _i3(_pad3([int(r) for r in peak_radius], 0))
  d.surface = surf.data_ptr()
  d.stream = _dev.stream_ptr()
  lib = _abi.load()
  ws = _dev.workspace(lib.sfm_peaks_workspace_bytes(C.byref(d)), dev)
  d.workspace = ws.data_ptr()
  d.workspace_bytes = ws.numel()
  out = torch.empty((surf.shape[0], dim + 2), dtype=torch.float32, device=dev)
  _abi.check(lib.sfm_peaks(C.byref(d), out.data_ptr()))
  return out.cpu().numpy()


def batched_xcorr_peaks(pre_image, post_image, pre_mask, post_mask,
                        patch_size: Sequence[int], starts, mean: float | None,
                        min_distance: int = 2, threshold_rel: float = 0.5,
                        peak_radius: int | Sequence[int] = 5,
                        post_patch_size: Sequence[int] | None = None,
                        post_starts=None,
                        method: int = _abi.XCORR_AUTO) -> np.ndarray:
  """One batch of patch correlations + peak statistics -> [b, dim + 2].

  Same contract as flow_field.batched_xcorr_peaks (flow_field.py:374-441).
  """
  dev = _dev.device()
  res = _Resident(pre_image, post_image, pre_mask, post_mask, dev)
  patch_size = tuple(int(p) for p in patch_size)
  post_patch_size = patch_size if post_patch_size is None else tuple(
      int(p) for p in post_patch_size)
  starts = np.asarray(starts).astype(np.int32)
  post_starts = starts if post_starts is None else np.asarray(
      post_starts).astype(np.int32)
  desc = _make_desc(res, patch_size, post_patch_size, mean, min_distance,
                    threshold_rel, peak_radius, method)
  return _run_batches(res, desc, starts, post_starts, starts.shape[0])


# ---------------------------------------------------------------------------
# public: the calculator
# ---------------------------------------------------------------------------
class JAXMaskedXCorrWithStatsCalculator:
  """Estimates optical flow using masked cross-correlation (GPU, HIP).

  Name, constructor and `flow_field` signature follow the reference class
  (flow_field.py:449-492) so existing drivers run unchanged.
  """

  non_spatial_flow_channels = 2  # peak sharpness, peak ratio

  def __init__(self, mean: float | None = None, peak_min_distance: float = 2,
               peak_radius: float = 5, method: int = _abi.XCORR_AUTO):
    self._mean = mean
    self._min_distance = peak_min_distance
    self._peak_radius = peak_radius
    self._method = method
    # geometry -> host plan of plain (un-masked, un-targeted) calls; LRU of 8,
    # guarded because one calculator may be shared between Python threads
    self._plans = collections.OrderedDict()
    self._plans_lock = threading.Lock()

  # -- host planning -------------------------------------------------------
  @staticmethod
  def _targeting(field, tstep, starts, psize, img_shape):
    """Integer [z]yx patch shifts from a targeting field, kept in bounds
    (flow_field.py:626-649 / :652-677)."""
    centre = (np.array(psize) // 2).reshape((1, -1))
    tstep = np.array(tstep).reshape((1, -1))
    query = np.round((starts + centre) / tstep).astype(int)
    q = [np.clip(query[:, i], 0, field.shape[i + 1] - 1)
         for i in range(query.shape[-1])]
    off = np.nan_to_num(field[(slice(None),) + tuple(q)].T).astype(int)[:, ::-1]
    new_starts = starts + off
    off = off - np.minimum(new_starts, 0)
    shape = np.array(img_shape)[None, ...]
    overshoot = np.maximum(new_starts + np.array(psize)[None, ...], shape) - shape
    return off - overshoot

  def plan(self, pre_shape, post_shape, patch_size, step, pre_mask=None,
           post_mask=None, selection_mask=None, max_masked=0.75,
           batch_size=4096, post_patch_size=None, pre_targeting_field=None,
           pre_targeting_step=None, post_targeting_field=None,
           post_targeting_step=None, counts_fn=None):
    """Everything flow_field() decides on the host before touching the GPU.

    `counts_fn(mask, patch, step)` overrides the device kernel that counts the
    masked pixels per grid patch (planning on a machine without a GPU).

    Returns a dict with the output shape, the row-major grid positions, the
    per-batch (edge-padded) pre/post start coordinates and targeting offsets.
    """
    nd = len(pre_shape)
    out_shape = (np.array(post_shape) - (np.array(post_patch_size) - step)) // step
    out_sel = tuple(slice(0, int(s)) for s in out_shape)
    if selection_mask is None:
      selection_mask = np.ones(out_shape, dtype=bool)
    else:
      selection_mask = np.array(selection_mask[out_sel], dtype=bool)
    for mask, psz in ((pre_mask, patch_size), (post_mask, post_patch_size)):
      if mask is None:
        continue
      s = (counts_fn or _masked_counts)(mask, psz, step)
      m = (s / np.prod(psz) >= max_masked)[out_sel]
      selection_mask[m] = False

    patch_offset = ((np.array(patch_size) - post_patch_size) // 2)[None, ...]
    oyx = np.array(np.where(selection_mask)).T.reshape(-1, nd)
    n = oyx.shape[0]
    n_batches = (n + batch_size - 1) // batch_size
    pad = n_batches * batch_size - n
    # Every batch is padded to `batch_size` by repeating its LAST position
    # (flow_field.py:614-618) so that batch-coupled results do not change.
    pos_all = oyx
    if pad:
      pos_all = np.concatenate([oyx, np.repeat(oyx[-1:], pad, axis=0)])
    post_starts = pos_all * np.array(step).reshape((1, -1))
    pre_starts = np.clip(post_starts - patch_offset, 0, np.inf).astype(int)
    tg_offsets = post_offsets = None
    if pre_targeting_field is not None and pre_targeting_step is not None:
      tg_offsets = self._targeting(pre_targeting_field, pre_targeting_step,
                                   pre_starts, patch_size, pre_shape)
      pre_starts = pre_starts + tg_offsets
    if post_targeting_field is not None and post_targeting_step is not None:
      post_offsets = self._targeting(post_targeting_field, post_targeting_step,
                                     post_starts, post_patch_size, post_shape)
      post_starts = post_starts + post_offsets
    pre_starts = np.clip(pre_starts, 0, np.inf).astype(int)
    post_starts = np.clip(post_starts, 0, np.inf).astype(int)
    return dict(out_shape=out_shape, positions=oyx, n_batches=n_batches,
                pre_starts=pre_starts, post_starts=post_starts,
                tg_offsets=tg_offsets, post_offsets=post_offsets)

  # -- the reference entry point ----------------------------------------------
  def flow_field(
      self,
      pre_image: np.ndarray,
      post_image: np.ndarray,
      patch_size: int | Sequence[int],
      step: int | Sequence[int],
      pre_mask=None,
      post_mask=None,
      mask_only_for_patch_selection=False,
      selection_mask=None,
      max_masked=0.75,
      batch_size=4096,
      post_patch_size: int | Sequence[int] | None = None,
      pre_targeting_field: np.ndarray | None = None,
      pre_targeting_step: int | Sequence[int] | None = None,
      post_targeting_field: np.ndarray | None = None,
      post_targeting_step: int | Sequence[int] | None = None,
      progress_fn: Callable[[list[T]], Iterator[T]] = _silent_fn,
      device_output: bool = False,
  ):
    """Computes the flow field from post to pre (flow_field.py:474-712).

    Arguments and result are those of the reference method.  Images may also
    be torch CUDA tensors (uint8 or float32) that are already resident in HBM.
    `device_output=True` (an extension) returns the field as a DeviceArray
    that stays in HBM, e.g. for flow_utils.clean_flow / compose_maps_fast.
    """
    assert pre_image.ndim == post_image.ndim
    nd = pre_image.ndim
    if not isinstance(patch_size, collections.abc.Sequence):
      patch_size = (patch_size,) * nd
    if post_patch_size is not None:
      if not isinstance(post_patch_size, collections.abc.Sequence):
        post_patch_size = (post_patch_size,) * nd
    else:
      post_patch_size = patch_size
    if not isinstance(step, collections.abc.Sequence):
      step = (step,) * nd
    if pre_targeting_step is not None and not isinstance(
        pre_targeting_step, collections.abc.Sequence):
      pre_targeting_step = (pre_targeting_step,) * nd
    if post_targeting_step is not None and not isinstance(
        post_targeting_step, collections.abc.Sequence):
      post_targeting_step = (post_targeting_step,) * nd
    assert len(patch_size) == nd
    assert len(post_patch_size) == nd
    assert len(step) == nd
    patch_size = tuple(int(p) for p in patch_size)
    post_patch_size = tuple(int(p) for p in post_patch_size)
    step = tuple(int(s) for s in step)

    # The reference's host loop (selection, start coordinates, targeting
    # lookups, scatter: flow_field.py:557-709) runs on the device; only the
    # finished [dim + 2, *grid] field crosses PCIe (or nothing with
    # device_output).  Section after section with the same geometry and no
    # masks / selection / targeting (the production loop) reuses the device plan.
    dev = _dev.device()
    res = _Resident(pre_image, post_image, pre_mask, post_mask, dev)
    plain = (pre_mask is None and post_mask is None and selection_mask is None and
             pre_targeting_field is None and post_targeting_field is None)
    key = (tuple(pre_image.shape), tuple(post_image.shape), patch_size, step,
           post_patch_size, int(batch_size), str(dev))
    plan = None
    if plain:
      with self._plans_lock:
        plan = self._plans.get(key)
        if plan is not None:
          self._plans.move_to_end(key)
    if plan is None:
      plan = self.device_plan(res, patch_size, step, selection_mask, max_masked,
                              batch_size, post_patch_size, pre_targeting_field,
                              pre_targeting_step, post_targeting_field,
                              post_targeting_step)
      if plain:
        with self._plans_lock:
          plan = self._plans.setdefault(key, plan)
          while len(self._plans) > 8:
            self._plans.popitem(last=False)   # its device tensors go with it
    out = self.field_from_plan(res, plan, patch_size, post_patch_size, batch_size,
                               mask_only_for_patch_selection, progress_fn)
    if device_output:
      return _dev.DeviceArray(out)
    return out.cpu().numpy()

  def field_from_plan(self, res: _Resident, plan: dict, patch_size, post_patch_size,
                      batch_size, mask_only_for_patch_selection=False,
                      progress_fn=_silent_fn) -> torch.Tensor:
    """What flow_field() does once the patches are planned: correlates the
    batches of a `device_plan()` and scatters the peaks into the NaN-filled
    [dim + 2, *grid] field, a device tensor.  `plan` needs out_shape, n,
    positions, starts, tg and po."""
    nd = res.ndim
    out_shape = plan['out_shape']
    out = torch.full([nd + 2] + list(out_shape), float('nan'), dtype=torch.float32,
                     device=res.dev)
    n = plan['n']
    if n > 0:
      if mask_only_for_patch_selection:
        res.pre_mask = res.post_mask = None
      desc = _make_desc(res, patch_size, post_patch_size, self._mean,
                        self._min_distance, 0.5, self._peak_radius, self._method)
      # progress_fn receives the per-batch grid positions like the reference's
      # (flow_field.py:610) and is only iterated for its side effects.
      progress = None
      if progress_fn is not _silent_fn:
        pos_h = plan['positions'][:n].cpu().numpy()
        progress = progress_fn([pos_h[i:i + batch_size]
                                for i in range(0, n, batch_size)])
      peaks = _run_batches_dev(res, desc, plan['starts'], batch_size, progress)
      sd = _abi.SfmFlowScatterDesc()
      sd.ndim = nd
      sd.n = n
      sd.grid = _i3(_pad3(out_shape, 1))
      sd.peaks = peaks.data_ptr()
      sd.positions = plan['positions'].data_ptr()
      if plan['tg'] is not None:
        sd.pre_offsets = plan['tg'].data_ptr()
      if plan['po'] is not None:
        sd.post_offsets = plan['po'].data_ptr()
      sd.out = out.data_ptr()
      sd.stream = _dev.stream_ptr()
      _abi.check(_abi.load().sfm_flow_scatter(C.byref(sd)))
    return out

  def device_plan(self, res: _Resident, patch_size, step, selection_mask=None,
                  max_masked=0.75, batch_size=4096, post_patch_size=None,
                  pre_targeting_field=None, pre_targeting_step=None,
                  post_targeting_field=None, post_targeting_step=None) -> dict:
    """What `plan()` decides, computed and kept on the device: selected grid
    positions (row-major), edge-padded to whole batches, the pre / post start
    coordinates [2, n_padded, dim] and the targeting offsets."""
    dev = res.dev
    nd = res.ndim
    pre_shape, post_shape = tuple(res.pre.shape), tuple(res.post.shape)
    out_shape = [int(v) for v in
                 (np.array(post_shape) - (np.array(post_patch_size) - step)) // step]
    out_sel = tuple(slice(0, s) for s in out_shape)
    if (int(np.prod(out_shape)) == 1 and selection_mask is None and
        pre_targeting_field is None and post_targeting_field is None):
      # ONE patch (whole-overlap correlations: stitch_rigid._estimate_offset).
      # The general plan below costs a dozen small launches and two host
      # round trips (~0.5 ms) to find out what one masked-pixel count per side
      # says: the patch at grid position 0 covers [0, patch) of its mask
      # (flow_field.py:570-589), starts are 0 on both sides.
      keep = True
      for mask, psz in ((res.pre_mask, patch_size), (res.post_mask, post_patch_size)):
        if mask is None:
          continue
        region = mask[tuple(slice(0, int(v)) for v in psz)]
        count = int(torch.count_nonzero(region).item())
        keep = keep and not (np.float64(count) / float(np.prod(psz)) >= max_masked)
      n = 1 if keep else 0
      total = int(batch_size) if keep else 0
      starts = None
      if keep:
        # post start 0; pre start = clip(0 - (patch - post_patch) // 2, 0, inf)
        # (flow_field.py:601-602, :621-622): +|offset| when the post patch is
        # the larger one, floor division like NumPy's
        starts = torch.zeros((2, total, nd), dtype=torch.int32, device=dev)
        pre0 = [max(0, -((int(p) - int(q)) // 2))
                for p, q in zip(patch_size, post_patch_size)]
        if any(pre0):
          starts[0] = torch.tensor(pre0, dtype=torch.int32, device=dev)
      return dict(out_shape=out_shape, n=n, n_batches=n,
                  positions=torch.zeros((total, nd), dtype=torch.int32, device=dev),
                  starts=starts, tg=None, po=None)
    if selection_mask is None:
      sel = torch.ones(out_shape, dtype=torch.bool, device=dev)
    else:
      sel = _dev.as_device_mask(np.asarray(selection_mask)[out_sel], dev).bool().clone()
    for mask, psz in ((res.pre_mask, patch_size), (res.post_mask, post_patch_size)):
      if mask is None:
        continue
      counts = _masked_counts(mask, psz, step, on_device=True)
      m = (counts.double() / float(np.prod(psz)) >= max_masked)[out_sel]
      sel[m] = False
    pos = torch.nonzero(sel).to(torch.int32)          # row-major, like np.where
    n = int(pos.shape[0])
    n_batches = (n + batch_size - 1) // batch_size
    pad = n_batches * batch_size - n
    if pad and n:
      # every batch is padded to `batch_size` by repeating the LAST position
      # (flow_field.py:614-618): batch-coupled results do not change
      pos = torch.cat([pos, pos[-1:].expand(pad, nd)])
    pos = pos.contiguous()
    plan = dict(out_shape=out_shape, n=n, n_batches=n_batches, positions=pos,
                starts=None, tg=None, po=None)
    if n == 0:
      return plan
    total = int(pos.shape[0])
    starts = torch.empty((2, total, nd), dtype=torch.int32, device=dev)
    d = _abi.SfmFlowStartsDesc()
    d.ndim = nd
    d.n = total
    d.step = _i3(_pad3(step, 1))
    d.patch = _i3(_pad3(patch_size, 1))
    d.post_patch = _i3(_pad3(post_patch_size, 1))
    d.pre_shape = _i3(_pad3(pre_shape, 1))
    d.post_shape = _i3(_pad3(post_shape, 1))
    d.positions = pos.data_ptr()
    keep = []
    for side, field, tstep in (('pre', pre_targeting_field, pre_targeting_step),
                               ('post', post_targeting_field, post_targeting_step)):
      if field is None or tstep is None:
        continue
      if isinstance(field, np.ndarray) and field.dtype == np.float64:
        # the reference truncates the float64 value (.astype(int),
        # flow_field.py:634): truncate before the float32 rounding can move a
        # value across an integer (pixel offsets are exact in float32)
        field = np.trunc(np.nan_to_num(field))
      f = _dev.as_device_f32(field, dev, copy=False)
      offs = torch.empty((total, nd), dtype=torch.int32, device=dev)
      keep += [f, offs]
      setattr(d, side + '_targeting_field', f.data_ptr())
      setattr(d, side + '_targeting_shape', _i3(_pad3(f.shape[1:], 1)))
      setattr(d, side + '_targeting_step', _i3(_pad3(tstep, 1)))
      setattr(d, side + '_offsets', offs.data_ptr())
      plan['tg' if side == 'pre' else 'po'] = offs
    d.pre_starts = starts[0].data_ptr()
    d.post_starts = starts[1].data_ptr()
    d.stream = _dev.stream_ptr()
    _abi.check(_abi.load().sfm_flow_starts(C.byref(d)))
    plan['starts'] = starts
    return plan

  # -- pieces shared with sofima_amd.dist ---------------------------------------
  def compute_batches(self, pre_image, post_image, pre_mask, post_mask,
                      patch_size, post_patch_size, plan, batch_size,
                      batch_ids=None, progress=None) -> np.ndarray:
    """Peaks [len(batch_ids) * batch_size, dim + 2] of the selected batches
    (all batches when `batch_ids` is None), computed on the current GPU."""
    dev = _dev.device()
    res = _Resident(pre_image, post_image, pre_mask, post_mask, dev)
    desc = _make_desc(res, patch_size, post_patch_size, self._mean,
                      self._min_distance, 0.5, self._peak_radius, self._method)
    pre_st, post_st = plan['pre_starts'], plan['post_starts']
    if batch_ids is not None:
      sel = np.concatenate([
          np.arange(b * batch_size, (b + 1) * batch_size) for b in batch_ids
      ]) if len(batch_ids) else np.zeros((0,), int)
      pre_st, post_st = pre_st[sel], post_st[sel]
      if len(sel) == 0:
        return np.zeros((0, res.ndim + 2), np.float32)
    # the device copy of the start coordinates lives with a reused plan
    if batch_ids is None:
      with self._plans_lock:
        cache = plan.setdefault('_starts_dev', {})
    else:
      cache = None
    return _run_batches(res, desc, pre_st, post_st, batch_size, progress, cache)

  @classmethod
  def assemble(cls, plan, nd, peaks) -> np.ndarray:
    """Scatters per-patch peaks (padding rows allowed at the end) into the
    [dim + 2, *grid] flow array, undoing the targeting offsets
    (flow_field.py:701-709)."""
    out_shape = plan['out_shape']
    output = np.full([cls.non_spatial_flow_channels + nd] + out_shape.tolist(),
                     np.nan, dtype=np.float32)
    pos = plan['positions']
    n = pos.shape[0]
    if n == 0:
      return output
    peaks = np.array(peaks[:n], dtype=np.float32)
    if plan['tg_offsets'] is not None:
      peaks[:, :nd] += plan['tg_offsets'][:n, ::-1]  # xy[z]
    if plan['post_offsets'] is not None:
      peaks[:, :nd] -= plan['post_offsets'][:n, ::-1]
    lin = plan.get('_lin')
    if lin is None:  # benign race: every thread computes the same array
      lin = plan['_lin'] = np.ravel_multi_index(tuple(pos.T), tuple(out_shape.tolist()))
    output.reshape(output.shape[0], -1)[:, lin] = peaks.T
    return output
