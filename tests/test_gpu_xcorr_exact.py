"""Un-masked correlation, element by element against exact sums (-m gpu).

Every element of every surface of the matrix-core path (method 2, the un-pruned
launch that the pruned and lazy modes are pinned to bit for bit) is held to the bound
tests/xcorr_exact_ref.py derives from the roundings of the epilogue form the case
reaches; constant patches give exact zeros.  The same through the C ABI with images
and overshooting starts, the fused peak entry on the same cases, and the float direct
kernel (the yardstick of the older tests) against the same exact values.

Worst device error / bound seen on an MI355X, for information (nothing is tuned to
it): see DESIGN.md section 4.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from sofima_amd import _abi
from tests import xcorr_exact_ref as ref

pytestmark = pytest.mark.gpu

ALL = ref.case_names()
# (peaks: the cases masked_xcorr takes as they are stacked; the one-row / one-column
# shapes are left to the surface tests)
PEAKS = ref.case_names(lambda c: c.eligible and c.kind != 'degenerate')
SENTINEL = -7.0
UNPRUNED = {'SFM_MFMA_PRUNE': '0', 'SFM_MFMA_LAZY': '0'}


def _surface_abi(gpu, pre, post, starts, P, Q, mean, method):
  """sfm_xcorr_surface on images with start coordinates [2, b, 2]; the output is
  pre-filled with a sentinel."""
  from sofima_amd import flow_field as ff
  res = ff._Resident(pre, post, None, None, gpu)
  desc = ff._make_desc(res, P, Q, mean, 2, 0.5, 5, method)
  b = starts.shape[1]
  st = torch.from_numpy(np.ascontiguousarray(starts.astype(np.int32))).to(gpu)
  lib = _abi.load()
  desc.batch = b
  desc.pre_starts = st.data_ptr()
  desc.post_starts = st.data_ptr() + b * 2 * 4
  need = lib.sfm_xcorr_workspace_bytes(C.byref(desc))
  assert need > 0, lib.sfm_last_error()
  ws = torch.empty(need, dtype=torch.uint8, device=gpu)
  desc.workspace, desc.workspace_bytes = ws.data_ptr(), need
  shape = tuple(p + q - 1 for p, q in zip(P, Q))
  out = torch.full((b,) + shape, SENTINEL, dtype=torch.float32, device=gpu)
  _abi.check(lib.sfm_xcorr_surface(C.byref(desc), out.data_ptr()))
  return out.cpu().numpy()


def _stacked(c, min_bytes=16):
  """The patches one below the other as images (padded with rows of 255 up to
  `min_bytes`, the least the staging loads take) and their starts [2, b, 2]."""
  b = len(c.a)
  st = np.zeros((2, b, 2), np.int32)
  imgs = []
  for s, (x, (py, px)) in enumerate(((c.a, c.P), (c.c, c.Q))):
    st[s, :, 0] = np.arange(b) * py
    img = x.reshape(b * py, px)
    rows = -(-min_bytes // px)
    if img.shape[0] < rows:
      img = np.concatenate([img, np.full((rows - img.shape[0], px), 255, np.uint8)])
    imgs.append(np.ascontiguousarray(img))
  return imgs[0], imgs[1], st


def _report(name, form, worst):
  print(f'{name}: form {form} device error / bound {worst:.3f} '
        f'(x K = {worst * ref.K[form]:.3f} units of 2^-24 sum|terms|)')


@pytest.mark.parametrize('name', ALL)
def test_matrix_core_surface_every_element(gpu, name):
  """flow_field.masked_xcorr, method 2: |got - exact| <= bound everywhere, exact
  zeros where a patch is constant, nothing non-finite.  A shape whose stacked
  images are below the 16 bytes of a staging load is refused with the documented
  message and runs through the C ABI with padded images instead."""
  from sofima_amd import flow_field
  c = ref.case(name)
  r = c.reference()
  if c.eligible:
    got = flow_field.masked_xcorr(c.a.copy(), c.c.copy(), method=_abi.XCORR_MFMA_I8, mean=c.mean)
  else:
    with pytest.raises(_abi.SofimaAmdError, match=ref.REFUSAL):
      flow_field.masked_xcorr(c.a.copy(), c.c.copy(), method=_abi.XCORR_MFMA_I8, mean=c.mean)
    pre, post, st = _stacked(c)
    assert ref.eligible(c.P, c.Q, pre.size, post.size)
    got = _surface_abi(gpu, pre, post, st, c.P, c.Q, c.mean, _abi.XCORR_MFMA_I8)
    assert not (got == SENTINEL).any()
  _report(name, c.form, ref.check(got, r, c.P, c.Q, c.form, name))


# images whose width is no multiple of 16 or of 4; starts at the four corners, past
# every side, and one inside at an odd offset: a ragged batch of 5
ABI_CASES = {
    'same_exact_48': ((67, 53), (67, 53), (48, 48), (48, 48)),
    'wide_24x320': ((41, 331), (37, 171), (24, 320), (16, 160)),
}


@pytest.mark.parametrize('mean', [None, 0.0])
@pytest.mark.parametrize('name', sorted(ABI_CASES))
def test_matrix_core_surface_from_images_and_starts(gpu, name, mean):
  """The C ABI on images: patches at all four image corners, starts that overshoot
  on every side (clamped like lax.dynamic_slice), unaligned rows -- the 16-byte
  staging loads at the very end of an image included.  The expected patches are cut
  on the host with the same clamp."""
  pre_shape, post_shape, P, Q = ABI_CASES[name]
  rng = np.random.default_rng(len(name))
  pre = rng.integers(0, 256, pre_shape).astype(np.uint8)
  post = rng.integers(0, 256, post_shape).astype(np.uint8)
  # related content, so that the surfaces have structure: the post image repeats the pre
  hh, ww = min(pre_shape[0], post_shape[0]), min(pre_shape[1], post_shape[1])
  post[:hh, :ww] = np.where(rng.random((hh, ww)) < 0.7, pre[:hh, :ww], post[:hh, :ww])
  big = 10 ** 4
  raw = np.array([[[0, 0], [0, big], [big, 0], [big, big], [5, 3]],
                  [[-3, -7], [-1, big], [big, -2], [big + 7, big + 1], [9, 1]]], np.int32)
  st = np.stack([raw[0], raw[1]])

  def cut(img, starts, size):
    out = []
    for y, x in starts:
      y0 = min(max(int(y), 0), img.shape[0] - size[0])
      x0 = min(max(int(x), 0), img.shape[1] - size[1])
      out.append(img[y0:y0 + size[0], x0:x0 + size[1]])
    return np.stack(out)

  # (pre starts overshoot in the second half of the list as well)
  st[0, 3] = (big + 3, big + 5)
  st[0, 0] = (-4, -9)
  a, c = cut(pre, st[0], P), cut(post, st[1], Q)
  form = ref.choose_mode(P, Q)
  r = ref.reference(a, c, mean, form, restate=False)
  got = _surface_abi(gpu, pre, post, st, P, Q, mean, _abi.XCORR_MFMA_I8)
  assert got.shape[0] == 5 and not (got == SENTINEL).any()
  _report(f'{name} mean {mean}', form, ref.check(got, r, P, Q, form, name))


@pytest.mark.parametrize('name', PEAKS)
@pytest.mark.parametrize('variant', ['default', 'unpruned'])
def test_fused_peaks_sit_on_the_exact_maximum(gpu, monkeypatch, variant, name):
  """batched_xcorr_peaks, method 2, with the default pruning and lazy stores and with
  both switched off: the first peak of every patch whose exact maximum leads the
  runner-up by more than 10 bounds is the exact argmax; a patch with an all-zero
  surface has no peak."""
  from sofima_amd import flow_field
  if variant == 'unpruned':
    for k, v in UNPRUNED.items():
      monkeypatch.setenv(k, v)
  c = ref.case(name)
  r = c.reference()
  pre, post, st = _stacked(c)
  got = flow_field.batched_xcorr_peaks(pre, post, None, None, c.P, st[0], c.mean, min_distance=2,
                                       threshold_rel=0.5, peak_radius=5, post_patch_size=c.Q,
                                       post_starts=st[1], method=_abi.XCORR_MFMA_I8)
  assert got.shape == (len(c.a), 4)
  off = (np.array(c.P) + np.array(c.Q)) // 2 - 1
  # which patches are held to what is recorded per case (ref.PEAK_PATTERN, pinned to the
  # reference on the CPU): 'z' no peak, 'p' the exact argmax, '-' not checked
  pattern = ref.PEAK_PATTERN[name]
  assert len(pattern) == len(c.a)
  n_checked = 0
  for k, (what, w) in enumerate(zip(pattern, r['exact'])):
    if what == 'z':
      assert r['zero'][k].all()
      assert np.isnan(got[k]).all(), (k, got[k])
    elif what == 'p':
      o = np.argsort(w, axis=None)[-2:]
      bound = r['bound'][k].ravel()
      assert w.ravel()[o[1]] - w.ravel()[o[0]] > 10 * max(bound[o[0]], bound[o[1]])
      iy, ix = np.unravel_index(o[1], w.shape)
      assert (got[k, 0], got[k, 1]) == (ix - off[1], iy - off[0]), (k, got[k], iy, ix)
    else:
      continue
    n_checked += 1
  assert n_checked == len(pattern) - pattern.count('-')


@pytest.mark.parametrize('name', ALL)
@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_direct_kernel_against_the_exact_values(gpu, dtype, name):
  """method 1 -- the yardstick of the older matrix-core tests -- on uint8 patches and
  on the same patches as float32, every case and every mean: within TOL32 x E of the
  exact value everywhere (E = ||a - mu_a|| ||c - mu_c||; measured on the reference's
  float32 form, CPU), and exactly 0 where a patch is constant at mean=None."""
  from sofima_amd import flow_field
  c = ref.case(name)
  r = c.reference()
  a, cc = (c.a.copy(), c.c.copy()) if dtype == 'uint8' else (c.a.astype(np.float32),
                                                            c.c.astype(np.float32))
  got = flow_field.masked_xcorr(a, cc, method=_abi.XCORR_DIRECT, mean=c.mean)
  assert got.shape == r['exact'].shape and np.isfinite(got).all()
  E = ref.energy_scale(c)
  dev = np.abs(got.astype(np.float64) - r['exact']).max((1, 2))
  live = E > 0
  print(f'{name} {dtype}: deviation / E {np.max(dev[live] / E[live]) if live.any() else 0:.3g} '
        f'(TOL32 {ref.TOL32:.3g})')
  assert (dev[live] <= ref.TOL32 * E[live]).all(), (dev, ref.TOL32 * E)
  # E = 0: a patch equals the mean that is subtracted, every product is 0
  assert (got[~live] == 0).all()


def test_same_size_pair_161_wide_takes_another_path(gpu):
  """(24, 161) / (24, 161) picks a search-window variant and the same-size mode, which
  those variants do not have (the launch used to fail, for the default method too):
  method 2 refuses the shape with the documented message, the default method computes
  it on a float path."""
  from sofima_amd import flow_field
  a, cc = ref._geometry_patches((24, 161), (24, 161), 4000)
  c = ref.Case('same_24x161', a, cc, None, 'refused')
  assert not c.eligible
  with pytest.raises(_abi.SofimaAmdError, match=ref.REFUSAL):
    flow_field.masked_xcorr(a.copy(), cc.copy(), method=_abi.XCORR_MFMA_I8, mean=None)
  got = flow_field.masked_xcorr(a.copy(), cc.copy(), mean=None)
  exact = ref.exact(a, cc, None)
  assert got.shape == exact.shape and np.isfinite(got).all()
  dev = np.abs(got.astype(np.float64) - exact).max((1, 2))
  # (the float paths' usual 1e-5 of the scale: which of them serves the shape is not the point)
  assert (dev <= 1e-5 * ref.energy_scale(c)).all(), (dev, ref.energy_scale(c))
