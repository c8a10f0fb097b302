"""reconcile_flows without a GPU: a NumPy / SciPy restatement of the contract
pinned against the reference's golden output, and the C-ABI surface."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from sofima_amd import _abi, _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def reconcile_restated(flows, max_gradient, max_deviation, min_patch_size, min_delta_z=0):
  """float32 statement of flow_utils.reconcile_flows, written from its contract."""
  flows = [np.asarray(f, np.float32) for f in flows]
  cur = flows[0].copy()
  nc = cur.shape[0]
  assert nc in (2, 3)
  # 1. later flows fill, per vector and in order, where channel 0 is still NaN
  for f in flows[1:]:
    take = np.isnan(cur[0])
    if nc == 3:
      with np.errstate(invalid='ignore'):
        take &= np.abs(f[2]) >= min_delta_z     # NumPy's promotion rules (NEP 50)
    cur[:, take] = f[:, take]
  with np.errstate(invalid='ignore', over='ignore'):
    # 2. zero-padded differences: ch0 along x, ch1 along y, both sides; the
    #    integer zero of the padding promotes the field, so they are float64
    if max_gradient > 0:
      lim = np.float64(max_gradient)
      c0 = cur[0].astype(np.float64)
      c1 = cur[1].astype(np.float64)
      gx = np.abs(np.diff(np.pad(c0, ((0, 0), (0, 0), (1, 1))), axis=2))
      gy = np.abs(np.diff(np.pad(c1, ((0, 0), (1, 1), (0, 0))), axis=1))
      bad = (gx[:, :, :-1] > lim) | (gx[:, :, 1:] > lim)
      bad |= (gy[:, :-1] > lim) | (gy[:, 1:] > lim)
      cur[:, bad] = np.nan
    # 3. deviation from the 3 x 3 median of nan_to_num (per slice, mirrored
    #    borders that repeat the edge); NaN in either channel never marks
    if max_deviation > 0:
      dev = []
      for ch in (0, 1):
        v = np.nan_to_num(cur[ch])
        p = np.pad(v, ((0, 0), (1, 1), (1, 1)), mode='symmetric')
        ny, nx = v.shape[1:]
        win = np.stack([p[:, dy:dy + ny, dx:dx + nx] for dy in range(3) for dx in range(3)])
        med = np.sort(win, axis=0)[4]
        dev.append(np.abs(med - cur[ch]))
      worst = np.where(np.isnan(dev[0]) | np.isnan(dev[1]), np.nan,
                       np.maximum(dev[0], dev[1]))
      cur[:, worst > max_deviation] = np.nan   # float32 or float64 as NumPy promotes
  # 4. 4-connected components per slice; the invalid vectors count as one
  #    more component (label 0)
  if min_patch_size > 0:
    valid = ~np.isnan(cur).any(axis=0)
    bad = np.zeros(valid.shape, bool)
    for z in range(valid.shape[0]):
      lab, _ = ndimage.label(valid[z], structure=CROSS)
      sizes = np.bincount(lab.ravel())
      bad[z] = (sizes < min_patch_size)[lab]
    cur[:, bad] = np.nan
  return cur


def golden_cases(g):
  """(name, flows, params, expected); the thresholds are Python numbers, except
  in the f64thr_* cases, where the reference was given float64 scalars."""
  for i, name in enumerate(g['names']):
    p = g[f'params_{i}']
    flows = list(g[f'flows_{i}'])
    thr = np.float64 if str(name).startswith('f64thr_') else float
    yield (str(name), flows, (float(p[0]), thr(p[1]), int(p[2]), thr(p[3])),
           g[f'out_{i}'])


def test_restatement_matches_reference_golden(golden):
  g = golden('reconcile_flows')
  n = 0
  for name, flows, params, want in golden_cases(g):
    before = [f.copy() for f in flows]
    got = reconcile_restated(flows, *params)
    assert got.dtype == np.float32, name
    assert np.array_equal(got, want, equal_nan=True), name
    for f, b in zip(flows, before):
      assert np.array_equal(f, b, equal_nan=True), name
    n += 1
  assert n >= 30


def test_golden_covers_the_contract(golden):
  """Every stage changes something, and each quirk is present in the golden file."""
  g = golden('reconcile_flows')
  cases = {name: (flows, params, want) for name, flows, params, want in golden_cases(g)}
  # merge: [nan, nan], [nan, 7], [3, 4] -> [3, 4]
  flows, _, want = cases['merge_later_overwrites']
  np.testing.assert_array_equal(want[:, 0, 0, 0], [3, 4])
  # background quirk: a lone NaN in ch2 survives min 1 and spreads at min 2
  np.testing.assert_array_equal(cases['ccl_3ch_partial_min1'][2][:, 0, 2, 2], [1, 1, np.nan])
  assert np.isnan(cases['ccl_3ch_partial_min2'][2][:, 0, 2, 2]).all()
  # every single-stage case does some masking
  for name, (flows, params, want) in cases.items():
    # (median_thr_1p1 is the case where float32 comparison keeps everything)
    if (name.startswith(('gradient', 'median', 'ccl_2ch_min2', 'ccl_blobs'))
        and name != 'median_thr_1p1'):
      assert np.isnan(want).sum() > np.isnan(flows[0]).sum(), name
  shapes = {flows[0].shape[0] for flows, _, _ in cases.values()}
  assert shapes == {2, 3}
  assert any(f[0].shape[2] == 1 for f, _, _ in cases.values())
  assert any(f[0].shape[3] == 1 for f, _, _ in cases.values())
  assert any(p[3] > 0 for _, p, _ in cases.values())
  # thresholds float32 cannot hold: the gradient compares in float64 ...
  assert np.isnan(cases['gradient_thr_1p1_single'][2][0]).sum() == 3
  assert np.isnan(cases['gradient_round_edge'][2][0, 0, 0, :2]).all()
  # ... the deviation and |dz| in float32, unless the threshold is a float64 scalar
  assert not np.isnan(cases['median_thr_1p1'][2][:, 0, 1, 1]).any()
  assert np.isnan(cases['f64thr_median_1p1'][2][:, 0, 1, 1]).all()
  assert not np.isnan(cases['merge_3ch_dz0p7'][2][:, 0, 0]).any()
  assert np.isnan(cases['f64thr_merge_3ch_dz0p7'][2][:, 0, 0]).all()


def test_restatement_quirks():
  # NaN dz never merges, even at min_delta_z = 0
  a = np.full((3, 1, 1, 2), np.nan, np.float32)
  b = np.array([5, 6, np.nan], np.float32)[:, None, None, None] * np.ones((3, 1, 1, 2),
                                                                         np.float32)
  b[2, 0, 0, 1] = 0
  out = reconcile_restated([a, b], 0, 0, 0, 0)
  assert np.isnan(out[:, 0, 0, 0]).all()
  np.testing.assert_array_equal(out[:, 0, 0, 1], [5, 6, 0])
  # diagonal-only neighbours are separate components; nothing joins across z
  f = np.full((2, 2, 3, 3), np.nan, np.float32)
  f[:, 0, 0, 0] = f[:, 0, 1, 1] = 1
  f[:, 1, 0, 0] = 1
  out = reconcile_restated([f], 0, 0, 2)
  assert np.isnan(out).all()
  # inf is masked by the median test, NaN differences by no gradient test
  f = np.zeros((2, 1, 3, 3), np.float32)
  f[0, 0, 1, 1] = np.inf
  assert np.isnan(reconcile_restated([f], 0, 1.0, 0)[:, 0, 1, 1]).all()


def test_reconcile_desc_layout_matches_header():
  text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
  body = re.search(r'typedef struct SfmReconcileDesc \{(.*?)\} SfmReconcileDesc;', text,
                   re.S).group(1)
  names = []
  for decl in body.split(';'):
    decl = decl.strip()
    if decl:
      names.append(re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$', decl).group(1))
  assert names == [f[0] for f in _abi.SfmReconcileDesc._fields_]
  assert 'sfm_reconcile_flows' in _abi.SIGNATURES
  assert 'sfm_reconcile_flows_workspace_bytes' in _abi.SIGNATURES


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _desc(c, shape, k=1, grad=1.0, dev=1.0, patch=5):
  d = _abi.SfmReconcileDesc()
  d.channels = c
  d.shape = (ctypes.c_int32 * 3)(*shape)
  d.num_flows = k
  d.max_gradient = grad
  d.max_deviation = dev
  d.min_patch_size = patch
  return d


def test_workspace_bytes_positive_and_monotone(lib):
  prev = 0
  for shape in ((1, 1, 1), (1, 8, 8), (2, 8, 8), (2, 64, 64), (16, 205, 205),
                (1, 2048, 2048)):
    for c in (2, 3):
      n = lib.sfm_reconcile_flows_workspace_bytes(ctypes.byref(_desc(c, shape)))
      assert n > 0
      if c == 2:
        assert n >= prev
        prev = n
      else:
        assert n >= lib.sfm_reconcile_flows_workspace_bytes(ctypes.byref(_desc(2, shape)))
  # the components need int32 parents and sizes per vector
  assert prev >= 2 * 4 * 2048 * 2048
  assert lib.sfm_reconcile_flows_workspace_bytes(None) == 0


def test_null_descriptor_rejected(lib):
  assert lib.sfm_reconcile_flows(None, None) == -1
  assert b'NULL' in lib.sfm_last_error()
  d = _desc(2, (1, 4, 4))
  assert lib.sfm_reconcile_flows(ctypes.byref(d), None) == -1
  assert b'NULL' in lib.sfm_last_error()
