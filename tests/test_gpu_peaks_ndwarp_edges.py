"""Edge tests of the stand-alone peak search and of warp.ndimage_warp (-m gpu).

Peak search (`sfm_peaks` behind `flow_field._batched_peaks`: peaks_first /
peaks_max / peaks_scan / peaks_first_finish / peaks_second kernels) against
oracle.flow_oracle.batched_peaks, and against tests.refs64.peaks64 where the
oracle has no answer (a surface smaller than the sharpness window).  Every
column is a coordinate difference or ONE float32 division of values read from
the surface, so the criterion is equality of bits, NaN patterns included.

warp.ndimage_warp (`ndimage_warp_kernel`) against
oracle.warp_oracle.ndimage_warp, which is scipy.ndimage.map_coordinates twice:
equal dtype, shape and elements.

The cases are built in tests/refs64.py on the boundaries the kernels draw
themselves (candidate capacity 2048, 2^18 elements, row widths 64 / 128 / 256,
four surfaces per second-pass workgroup, the 5 x 5 fast window; the range test,
the rounding and the zero-weight tap of the sampler) and with NaN and
infinities; tests/test_peaks_ndwarp_refs.py checks on the CPU that they reach
what they name.
"""
import ctypes as C
import types

import numpy as np
import pytest

from oracle import flow_oracle, warp_oracle
from tests import refs64
from tests.refs64 import NDWARP_CASE_GROUPS, PEAKS_CASE_GROUPS, peaks64

pytestmark = pytest.mark.gpu
f32 = np.float32


def assert_same_bits(got, want, name=''):
  """Equal shape and dtype, identical NaN pattern, every other element equal in
  its bits (so -0.0 is not 0.0)."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, name
  nan = np.isnan(want)
  np.testing.assert_array_equal(np.isnan(got), nan, err_msg=name)
  np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32),
                                err_msg=f'{name}\ngot\n{got}\nwant\n{want}')


# ---------------------------------------------------------------------------
# peaks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('group', list(PEAKS_CASE_GROUPS))
def test_batched_peaks_edges(gpu, group):
  """Before the surface maximum propagated NaN the 'special' group failed in its
  NaN cases, on 40 x 37 and on 512 x 512 alike: a surface holding a NaN came
  back as a finite row ([0, 0, 32, 1.6] for a NaN row), and its neighbour kept
  the candidate at index 0 the NaN row should have struck (ratio 4 / 3 for
  4 / 2.5)."""
  from sofima_amd import flow_field
  for c in PEAKS_CASE_GROUPS[group]():
    args = (c['img'], c['center'], c['min_distance'], c['threshold_rel'], c['radius'])
    got = flow_field._batched_peaks(*args)
    if c['oracle']:
      with np.errstate(invalid='ignore'):
        want = flow_oracle.batched_peaks(*args)
    else:
      want = peaks64(*args)
    assert_same_bits(got, want, c['name'])


def test_peaks_reject_negative_parameters(gpu):
  """ValueError from the Python entry, SFM_ERR_INVALID from sfm_peaks itself."""
  import torch
  from sofima_amd import _abi, flow_field
  img = np.zeros((2, 8, 9), f32)
  with pytest.raises(ValueError):
    flow_field._batched_peaks(img, (4, 4), -1, 0.5, 5)
  with pytest.raises(ValueError):
    flow_field._batched_peaks(img, (4, 4), 2, 0.5, (5, -1))
  lib = _abi.load()
  surf = torch.zeros((2, 8, 9), dtype=torch.float32, device=gpu)
  out = torch.full((2, 4), 7.0, dtype=torch.float32, device=gpu)

  def desc(min_distance, radius):
    d = _abi.SfmPeaksDesc()
    d.ndim, d.batch = 2, 2
    d.shape = (C.c_int32 * 3)(1, 8, 9)
    d.center_offset = (C.c_float * 3)(0, 4, 4)
    d.min_distance = min_distance
    d.threshold_rel = 0.5
    d.peak_radius = (C.c_int32 * 3)(*radius)
    d.surface = surf.data_ptr()
    return d

  good = desc(2, (0, 5, 5))
  ws = torch.zeros(lib.sfm_peaks_workspace_bytes(C.byref(good)), dtype=torch.uint8, device=gpu)
  for d in (desc(-1, (0, 5, 5)), desc(2, (0, -1, 5)), desc(2, (0, 5, -2))):
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    assert lib.sfm_peaks(C.byref(d), out.data_ptr()) == -1      # SFM_ERR_INVALID
    assert b'must be >= 0' in lib.sfm_last_error()
  torch.cuda.synchronize()
  assert (out.cpu().numpy() == 7.0).all()       # nothing was launched
  # (the unused z radius of 2-D surfaces is not looked at)
  good = desc(2, (-1, 5, 5))
  good.workspace, good.workspace_bytes = ws.data_ptr(), ws.numel()
  assert lib.sfm_peaks(C.byref(good), out.data_ptr()) == 0
  torch.cuda.synchronize()
  assert np.isnan(out.cpu().numpy()).all()      # all-zero surfaces: no peak


# ---------------------------------------------------------------------------
# ndimage_warp
# ---------------------------------------------------------------------------
def _gpu_warp(c):
  from sofima_amd import warp
  dim = c['image'].ndim
  kw = {}
  if c['boxes'] is not None:
    kw = {k + '_box': types.SimpleNamespace(start=np.array(c['boxes'][k][0]),
                                            size=np.array(c['boxes'][k][1]))
          for k in ('image', 'map', 'out')}
  if c['scale'] is not None:
    kw['out_scale'] = c['scale']
  return warp.ndimage_warp(c['image'], c['cmap'], c['stride'], (64,) * dim, (0,) * dim,
                           order=c['order'], **kw)


@pytest.mark.parametrize('group', list(NDWARP_CASE_GROUPS))
def test_ndimage_warp_edges(gpu, group):
  """With the range test `c < 0 || c > len - 1` and a clamped edge tap,
  'nonfinite' and 'edge_tap' failed: a NaN dense coordinate (NaN node, or
  0 x inf beside an infinite node) sampled the image at index 0 for order 0
  (e.g. 214 for 0) and gave NaN for float32 images at order 1; the output row
  exactly on the last node read a finite coordinate past a NaN node at index
  m - 2 (a pixel for 0); the voxel exactly on the last image sample stayed
  finite beside an inf / NaN sample (32.02 for NaN)."""
  for c in NDWARP_CASE_GROUPS[group]():
    got = _gpu_warp(c)
    want = warp_oracle.ndimage_warp(c['image'], c['cmap'], c['stride'],
                                    **refs64.ndwarp_oracle_args(c))
    assert got.dtype == want.dtype and got.shape == want.shape, c['name']
    np.testing.assert_array_equal(got, want, err_msg=c['name'])
