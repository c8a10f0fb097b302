"""Masked (Padfield) correlation, element by element against the exact reference
(-m gpu).

Every element of every surface is checked (tests/masked_exact_ref.py): cut
elements are exactly 0, kept ones are within the tolerance of the exact value,
and only the few elements whose exact denominator sits within the documented
rounding of the kernel's own may fall on either side.  The matrix-core path is
held to the bound its code documents (2^-20 relative on the denominator), in all
its builds; the float32 paths to constants measured on the reference's float32
form.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from sofima_amd import _abi
from tests import masked_exact_ref as ref

pytestmark = pytest.mark.gpu

MFMA_2D = ref.case_names(lambda c: c.mfma and c.group is None)
GROUPS = ref.case_names(lambda c: c.group is not None)
# the production shape runs once per build of the matrix-core path, not per method
F32_CASES = ref.case_names(lambda c: c.group is None and c.name != 'geo_160x160_160x160')
VARIANTS = {'default': {}, 'eight_pass': {'SFM_MASKED_FAST': '0'},
            'sweep_maxima': {'SFM_MASKED_AXISMAX': '0'},
            'no_dead_rows': {'SFM_MASKED_DEADROWS': '0'}}


def _surface(c, method):
  from sofima_amd import flow_field
  return flow_field.masked_xcorr(c.prev.copy(), c.curr.copy(), c.pm.copy(), c.cm.copy(),
                                 dim=c.dim, method=method, mean=None)


def _stacked(c):
  """The patches of a 2-D case one below the other, as images, and the start
  coordinates [2, b, 2] of every patch in them."""
  b = len(c.prev)
  (py, px), (qy, qx) = c.P, c.Q
  st = np.zeros((2, b, 2), np.int32)
  st[0, :, 0] = np.arange(b) * py
  st[1, :, 0] = np.arange(b) * qy
  return (c.prev.reshape(b * py, px).copy(), c.curr.reshape(b * qy, qx).copy(),
          c.pm.reshape(b * py, px).copy(), c.cm.reshape(b * qy, qx).copy(), st)


def _surface_abi(gpu, c, method):
  """sfm_xcorr_surface with `group` set (flow_field.masked_xcorr has one group)."""
  from sofima_amd import flow_field as ff
  pre, post, pm, cm, st = _stacked(c)
  b = len(c.prev)
  res = ff._Resident(pre, post, pm, cm, gpu)
  desc = ff._make_desc(res, c.P, c.Q, None, 2, 0.5, 5, method)
  starts = torch.from_numpy(st).to(gpu)
  lib = _abi.load()
  desc.batch, desc.group = b, c.group
  desc.pre_starts = starts.data_ptr()
  desc.post_starts = starts.data_ptr() + b * 2 * 4
  need = lib.sfm_xcorr_workspace_bytes(C.byref(desc))
  assert need > 0, lib.sfm_last_error()
  ws = torch.empty(need, dtype=torch.uint8, device=gpu)
  desc.workspace, desc.workspace_bytes = ws.data_ptr(), need
  shape = tuple(p + q - 1 for p, q in zip(c.P, c.Q))
  out = torch.full((b,) + shape, -7.0, dtype=torch.float32, device=gpu)
  _abi.check(lib.sfm_xcorr_surface(C.byref(desc), out.data_ptr()))
  return out.cpu().numpy()


def _check_mfma(got, c):
  ref.check(got, c.classify(ref.BAND_MFMA), ref.ATOL_MFMA)


def _check_f32(got, c):
  ref.check(got, c.classify(ref.BAND32), ref.ATOL32, exact_zero_den=False)


@pytest.mark.parametrize('name', MFMA_2D)
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_matrix_core_surface_is_exact_everywhere(gpu, monkeypatch, variant, name):
  """method 2 in every build of it: the fast forms, all eight passes, the
  maxima from a sweep, no dead rows."""
  for k, v in VARIANTS[variant].items():
    monkeypatch.setenv(k, v)
  c = ref.case(name)
  _check_mfma(_surface(c, _abi.XCORR_MFMA_I8), c)


@pytest.mark.parametrize('name', F32_CASES)
@pytest.mark.parametrize('method', [_abi.XCORR_DIRECT, _abi.XCORR_FFT])
def test_float32_surface_against_the_exact_reference(gpu, method, name):
  c = ref.case(name)
  _check_f32(_surface(c, method), c)


@pytest.mark.parametrize('name', GROUPS)
@pytest.mark.parametrize('method', [_abi.XCORR_MFMA_I8, _abi.XCORR_DIRECT, _abi.XCORR_FFT])
def test_groups_keep_their_own_maxima(gpu, method, name):
  """group = 2 through the C ABI (batch 4, and a ragged batch 5): the faint patch
  is cut beside the textured one and whole beside another faint one."""
  c = ref.case(name)
  got = _surface_abi(gpu, c, method)
  assert not (got == -7.0).any()
  if method == _abi.XCORR_MFMA_I8:
    _check_mfma(got, c)
    cls = c.classify(ref.BAND_MFMA)
    assert ((got[1] == 0) & (got[2] != 0) & cls['live'][1]).sum() > 100
  else:
    _check_f32(got, c)


@pytest.mark.parametrize('mean', [0.0, 37.5, 255.0, 1000.0, -3.0])
def test_matrix_core_surface_does_not_depend_on_the_subtracted_mean(gpu, mean):
  """A given mean moves the integer centre of every patch (clamped into the range
  the int8 operands allow); the surface is the same exact quantity."""
  from sofima_amd import flow_field
  for name in ('geo_20x48_20x48', 'faint_50x46_37x31'):
    c = ref.case(name)
    got = flow_field.masked_xcorr(c.prev.copy(), c.curr.copy(), c.pm.copy(), c.cm.copy(),
                                  method=_abi.XCORR_MFMA_I8, mean=mean)
    _check_mfma(got, c)


@pytest.mark.parametrize('name', MFMA_2D)
@pytest.mark.parametrize('variant', ['default', 'no_dead_rows', 'no_block_maxima'])
def test_matrix_core_peaks_sit_on_the_reference_maximum(gpu, monkeypatch, variant, name):
  """batched_xcorr_peaks, method 2, with masks: the first peak of every patch whose
  reference maximum leads the runner-up by more than 10 atol is the reference
  argmax (the surface / block maxima the assembly writes, dead rows included;
  also with the peak sweep reading every row / every block);
  a patch whose surface is all zero has no peak."""
  from sofima_amd import flow_field
  for k, v in {'default': {}, 'no_dead_rows': {'SFM_MASKED_DEADROWS': '0'},
               'no_block_maxima': {'SFM_MASKED_BLKMAX': '0'}}[variant].items():
    monkeypatch.setenv(k, v)
  c = ref.case(name)
  cls = c.classify(ref.BAND_MFMA)
  pre, post, pm, cm, st = _stacked(c)
  got = flow_field.batched_xcorr_peaks(pre, post, pm, cm, c.P, st[0], None, min_distance=2,
                                       threshold_rel=0.5, peak_radius=5, post_patch_size=c.Q,
                                       post_starts=st[1], method=_abi.XCORR_MFMA_I8)
  assert got.shape == (len(c.prev), 4)
  off = (np.array(c.P) + np.array(c.Q)) // 2 - 1
  n_checked = 0
  for k, w in enumerate(cls['want']):
    if cls['undecided'][k].any():
      continue
    if not w.any():
      assert np.isnan(got[k]).all(), (k, got[k])
      n_checked += 1
      continue
    top = np.sort(w, axis=None)[-2:]
    if top[1] <= 10 * ref.ATOL_MFMA or top[1] - top[0] <= 10 * ref.ATOL_MFMA:
      continue
    iy, ix = np.unravel_index(np.argmax(w), w.shape)
    assert (got[k, 0], got[k, 1]) == (ix - off[1], iy - off[0]), (k, got[k], iy, ix)
    n_checked += 1
  assert n_checked >= (1 if c.kind in ('degenerate', 'faint_only') else 2)
