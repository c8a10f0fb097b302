"""A ragged last group through the C ABI (-m gpu).

`flow_field` pads its calls to whole reference batches, so only the ABI reaches
a call whose last group is shorter: batch = 11, group = 4 must give, bit for bit,
what three calls of 4, 4 and 3 rows with group = 0 give on the matching slices of
the start coordinates -- on every correlation path.
"""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage

from sofima_amd import _abi

pytestmark = pytest.mark.gpu

BATCH, GROUP = 11, 4
# name -> (dtype, patch, post patch, method, masked)
U8, F32 = np.uint8, np.float32
PATHS = {
    'mfma': (U8, (48, 48), (48, 48), _abi.XCORR_AUTO, False),
    'mfma_masked': (U8, (48, 48), (48, 48), _abi.XCORR_AUTO, True),
    'direct': (F32, (24, 24), (24, 20), _abi.XCORR_DIRECT, False),
    'direct_masked': (F32, (24, 24), (24, 20), _abi.XCORR_DIRECT, True),
    'fft': (F32, (24, 24), (24, 20), _abi.XCORR_FFT, False),
    'fft_masked': (F32, (24, 24), (24, 20), _abi.XCORR_FFT, True),
}


def _setup(gpu, path):
  """Descriptor (batch, group, starts and workspace still unset) + the device
  starts [2, BATCH, 2], some of them beyond the border (the gather clamps them)."""
  from sofima_amd import flow_field as ff
  dtype, patch, post_patch, method, masked = PATHS[path]
  rng = np.random.default_rng(5)
  base = ndimage.gaussian_filter(rng.standard_normal((100, 116)), 1.5)
  base = (base - base.min()) / (base.max() - base.min()) * 255
  pre, post = base[2:98, 3:115].astype(dtype), base[4:100, 1:113].astype(dtype)
  masks = (None, None)
  if masked:
    masks = (rng.random(pre.shape) < 0.05, rng.random(post.shape) < 0.05)
  res = ff._Resident(pre, post, masks[0], masks[1], gpu)
  desc = ff._make_desc(res, patch, post_patch, None, 2, 0.5, 5, method)
  hi = np.array(pre.shape) - np.array(patch)
  st = rng.integers(0, hi + 1, (2, BATCH, 2))
  st[1] = np.clip(st[0] + rng.integers(-3, 4, (BATCH, 2)), 0, None)
  st[:, 1] = (-4, 7)             # clamped at the low border
  st[:, 6] = hi + (9, 2)         # ... at the high border (the last row of a group)
  st[:, 10] = (hi[0] + 5, -1)    # ... and in the ragged group
  starts = torch.from_numpy(st.astype(np.int32)).to(gpu)
  return res, desc, starts


def _call(entry, desc, starts, lo, n, group, row_shape, gpu):
  lib = _abi.load()
  desc.batch, desc.group = n, group
  desc.pre_starts = starts.data_ptr() + lo * 2 * 4
  desc.post_starts = starts.data_ptr() + (BATCH + lo) * 2 * 4
  need = lib.sfm_xcorr_workspace_bytes(C.byref(desc))
  assert need > 0, lib.sfm_last_error()
  ws = torch.empty(need, dtype=torch.uint8, device=gpu)
  desc.workspace, desc.workspace_bytes = ws.data_ptr(), need
  out = torch.full((n,) + row_shape, -7.0, dtype=torch.float32, device=gpu)
  _abi.check(getattr(lib, entry)(C.byref(desc), out.data_ptr()))
  return out.cpu().numpy()


def _grouped_and_split(entry, path, row_shape, gpu):
  res, desc, starts = _setup(gpu, path)
  whole = _call(entry, desc, starts, 0, BATCH, GROUP, row_shape, gpu)
  parts = [_call(entry, desc, starts, lo, min(GROUP, BATCH - lo), 0, row_shape, gpu)
           for lo in range(0, BATCH, GROUP)]
  assert [len(p) for p in parts] == [4, 4, 3]
  return whole, np.concatenate(parts)


@pytest.mark.parametrize('path', list(PATHS))
def test_peaks_of_a_ragged_last_group_equal_group_by_group_calls(gpu, path):
  whole, split = _grouped_and_split('sfm_xcorr_peaks', path, (4,), gpu)
  assert np.isfinite(whole[:, :2]).any() and not (whole == -7.0).any()
  np.testing.assert_array_equal(whole, split)


@pytest.mark.parametrize('path', ['direct_masked', 'mfma_masked'])
def test_masked_surfaces_of_a_ragged_last_group_equal_group_by_group_calls(gpu, path):
  _, patch, post_patch, _, _ = PATHS[path]
  shape = tuple(p + q - 1 for p, q in zip(patch, post_patch))
  whole, split = _grouped_and_split('sfm_xcorr_surface', path, shape, gpu)
  assert (whole != 0).any(axis=(1, 2)).all() and not (whole == -7.0).any()
  np.testing.assert_array_equal(whole, split)
