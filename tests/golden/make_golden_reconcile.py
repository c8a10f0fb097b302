"""Generates tests/golden/reconcile_flows.npz from the UNMODIFIED reference
`flow_utils.reconcile_flows` (pure NumPy / SciPy, so no stand-in is involved in
the computation; `_refshim` only makes `import sofima` resolve).

Build-container only.  Each case stores its flows packed as [K, c, z, y, x],
its parameters (max_gradient, max_deviation, min_patch_size, min_delta_z) and
the reference's output.  Run:  python tests/golden/make_golden_reconcile.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()
from sofima import flow_utils as rfu  # noqa: E402

NAN, INF = np.nan, np.inf


def blobs(rng, shape, sigma, frac):
  """Thresholded smoothed noise: components of every size, U shapes,
  diagonal-only contacts."""
  noise = ndimage.gaussian_filter(rng.standard_normal(shape), sigma)
  return noise > np.quantile(noise, 1 - frac)


def smooth_flow(rng, c, z, y, x, scale=3.0, outliers=0.05):
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, y, x)), (0, 2, 2)) * 20
                for _ in range(c)]).astype(np.float32)
  hit = rng.random((z, y, x)) < outliers
  f[:2, hit] += rng.choice([-1, 1], size=(2, hit.sum())) * rng.uniform(3, 30, (2, hit.sum()))
  return f * np.float32(scale / 3.0)


def with_holes(rng, f, frac=0.35, sigma=1.2):
  f = f.copy()
  holes = ~blobs(rng, f.shape[1:], sigma, 1 - frac)
  f[:, holes] = NAN
  return f


def main():
  rng = np.random.default_rng(7)
  cases = []

  def add(name, flows, max_gradient, max_deviation, min_patch_size, min_delta_z=0):
    flows = [np.asarray(f, np.float32) for f in flows]
    out = rfu.reconcile_flows([f.copy() for f in flows], max_gradient, max_deviation,
                              min_patch_size, min_delta_z)
    assert out.dtype == np.float32
    cases.append((name, np.stack(flows),
                  np.array([max_gradient, max_deviation, min_patch_size, min_delta_z],
                           np.float64), out))

  # -- merge -----------------------------------------------------------------
  a = np.full((2, 1, 2, 3), NAN, np.float32)
  b = np.full((2, 1, 2, 3), NAN, np.float32)
  b[1] = 7
  c = np.zeros((2, 1, 2, 3), np.float32)
  c[0], c[1] = 3, 4
  a[:, 0, 1, 2] = (1, 2)
  add('merge_later_overwrites', [a, b, c], 0, 0, 0)
  f1 = with_holes(rng, smooth_flow(rng, 2, 3, 11, 13), 0.4)
  f2 = with_holes(rng, smooth_flow(rng, 2, 3, 11, 13), 0.4)
  f3 = with_holes(rng, smooth_flow(rng, 2, 3, 11, 13), 0.2)
  add('merge_three_2ch', [f1, f2, f3], 0, 0, 0)
  add('merge_one_flow', [f1], 0, 0, 0)
  g1 = with_holes(rng, smooth_flow(rng, 3, 2, 9, 10), 0.5)
  g2 = smooth_flow(rng, 3, 2, 9, 10)
  g2[2] = rng.choice([0, 1, 2, 3, -2, -5, NAN], size=g2[2].shape)
  g3 = smooth_flow(rng, 3, 2, 9, 10)
  g3[2] = rng.choice([0, 1, 4, -3, NAN, INF], size=g3[2].shape)
  add('merge_3ch_dz0', [g1, g2, g3], 0, 0, 0, 0)
  add('merge_3ch_dz2', [g1, g2, g3], 0, 0, 0, 2)
  add('merge_3ch_dz3', [g1, g2], 0, 0, 0, 3)

  # -- gradient --------------------------------------------------------------
  h = smooth_flow(rng, 2, 2, 12, 14)
  h[0, 0, 5, 0] = 9       # x border: |ch0| itself over the limit
  h[0, 1, 3, 13] = -9
  h[1, 0, 0, 4] = 12      # y border
  h[1, 1, 11, 7] = -12
  h[0, 0, 7, 6] = NAN     # NaN differences never mask
  h[1, 1, 4, 4] = NAN
  h[0, 1, 8, 8] = INF
  h[1, 0, 9, 2] = -INF
  add('gradient_2ch', [h], 6.0, 0, 0)
  add('gradient_2ch_tight', [h], 1.5, 0, 0)
  h3 = smooth_flow(rng, 3, 2, 8, 9)
  h3[2, 0, 3, 3] = NAN
  add('gradient_3ch', [h3], 2.0, 0, 0)

  # -- median deviation ------------------------------------------------------
  m = smooth_flow(rng, 2, 3, 10, 12)
  m[0, 0, 4, 4] = INF
  m[1, 1, 6, 2] = -INF
  m[0, 2, 0, 0] = NAN       # partial NaN: the max propagates it, never bad
  m[:, 1, 9, 11] = NAN
  m[0, 0, 2, 2] += 50
  add('median_2ch', [m], 0, 4.0, 0)
  add('median_2ch_tight', [m], 0, 0.7, 0)
  m3 = smooth_flow(rng, 3, 3, 8, 7)
  m3[2] *= 40               # ch2 enters no comparison
  m3[2, 1, 3, 3] = NAN
  add('median_3ch', [m3], 0, 2.0, 0)

  # -- small components --------------------------------------------------------
  k = np.ones((2, 3, 9, 10), np.float32)
  valid = np.zeros((3, 9, 10), bool)
  valid[0, 1:4, 1:4] = True         # 9
  valid[0, 5, 1] = valid[0, 6, 2] = valid[0, 7, 3] = True  # diagonal-only singles
  valid[0, 4, 4] = True             # touches the square diagonally
  valid[0, 1:7, 8] = True           # U shape: 6 + 6 + 2
  valid[0, 1:7, 6] = True
  valid[0, 7, 6:9] = True
  valid[1, 1:4, 1:4] = True         # same (y, x) in the next slice: separate
  valid[2] = True
  valid[2, 4, 3] = False            # n0 = 1 -> background quirk
  k[:, ~valid] = NAN
  for mp in (1, 2, 4, 9, 10, 15):
    add(f'ccl_2ch_min{mp}', [k], 0, 0, mp)
  k3 = np.ones((3, 1, 4, 5), np.float32)
  k3[2, 0, 2, 2] = NAN              # a single NaN in ch2 only
  add('ccl_3ch_partial_min1', [k3], 0, 0, 1)
  add('ccl_3ch_partial_min2', [k3], 0, 0, 2)
  k3b = np.ones((3, 2, 6, 6), np.float32)
  k3b[0, 0, 1, :] = NAN
  k3b[2, 0, 4, 1:5] = NAN
  k3b[1, 1, :, 3] = NAN
  add('ccl_3ch_partial_min5', [k3b], 0, 0, 5)
  add('ccl_3ch_partial_min40', [k3b], 0, 0, 40)
  fz = np.ones((2, 4, 16, 17), np.float32)
  fz[:, ~blobs(rng, (4, 16, 17), 1.0, 0.5)] = NAN
  for mp in (2, 5, 17):
    add(f'ccl_blobs_min{mp}', [fz], 0, 0, mp)
  fz[:, 2] = 1          # a slice without invalid vectors
  add('ccl_blobs_full_slice', [fz], 0, 0, 3)

  # -- thin slices -------------------------------------------------------------
  t = smooth_flow(rng, 2, 3, 1, 23)
  t[:, 0, 0, 5] = NAN
  t[:, 1, 0, 11:13] = NAN
  t[0, 2, 0, 0] = 8
  add('y1_all', [t], 4.0, 1.5, 3)
  t2 = smooth_flow(rng, 2, 3, 1, 23)
  add('y1_merge', [t, t2], 4.0, 1.5, 3)
  u = smooth_flow(rng, 2, 3, 19, 1)
  u[:, 0, 4, 0] = NAN
  u[1, 1, 0, 0] = 8
  add('x1_all', [u], 4.0, 1.5, 3)
  add('x1_merge', [u, smooth_flow(rng, 2, 3, 19, 1)], 4.0, 1.5, 3)
  add('single_vector', [np.full((2, 1, 1, 1), 2.0, np.float32)], 1.0, 1.0, 2)
  add('single_vector_min1', [np.full((3, 2, 1, 1), 0.5, np.float32)], 1.0, 1.0, 1, 1)

  # -- all stages --------------------------------------------------------------
  for i in range(4):
    cc = 2 + (i % 2)
    shape = (cc, 3, 24, 27)
    fl = [with_holes(rng, smooth_flow(rng, *shape), 0.3 + 0.15 * j) for j in range(1 + i % 3)]
    fl[0][0, 0, 3, 3] = INF
    fl[0][1, 1, 7, 9] = -INF
    if cc == 3:
      fl[0][2, 2, 5, 5] = NAN
    add(f'all_{cc}ch_k{len(fl)}_{i}', fl, 5.0, 2.5, 6, 1 if cc == 3 else 0)
  fl = [with_holes(rng, smooth_flow(rng, 2, 4, 30, 28), 0.45) for _ in range(2)]
  add('all_2ch_em_like', fl, 0, 20, 12)
  add('all_2ch_loose', fl, 8.0, 20, 400)

  # -- thresholds that float32 cannot hold -------------------------------------
  # The gradient is float64 (np.diff's integer zero promotes the field) for any
  # threshold; the deviation and |dz| compare in float32 against a Python number
  # and in float64 against a float64 scalar (cases named f64thr_*).
  e = np.zeros((2, 1, 3, 3), np.float32)
  e[0, 0, 1, 1] = np.float32(1.1)
  add('gradient_thr_1p1_single', [e], 1.1, 0, 0)
  e = np.zeros((2, 1, 1, 3), np.float32)
  e[0, 0, 0] = (-1e-7, 3.0, 0)
  add('gradient_round_edge', [e], 3.0, 0, 0)
  e = np.zeros((2, 2, 4, 5), np.float32)
  e[1, 0, 1, 2] = np.float32(0.1)
  e[1, 1, 2, 3] = -np.float32(0.1)
  e[0, 1, 0, 0] = np.float32(0.1) + np.float32(1e-9)
  add('gradient_thr_0p1', [e], 0.1, 0, 0)
  s1 = smooth_flow(rng, 2, 2, 10, 11, scale=0.3)
  add('gradient_thr_1p1_smooth', [s1], 1.1, 0, 0)
  add('gradient_thr_0p3_smooth', [s1], 0.3, 0, 0)
  e = np.zeros((2, 1, 3, 4), np.float32)
  e[0, 0, 1, 1] = np.float32(1.1)
  e[1, 0, 1, 2] = np.float32(0.1)
  add('median_thr_1p1', [e], 0, 1.1, 0)
  add('median_thr_0p1', [e], 0, 0.1, 0)
  add('f64thr_median_1p1', [e], 0, np.float64(1.1), 0)
  add('f64thr_median_0p1', [e], 0, np.float64(0.1), 0)
  add('median_thr_0p3_smooth', [s1], 0, 0.3, 0)
  add('f64thr_median_0p3_smooth', [s1], 0, np.float64(0.3), 0)
  e1 = np.full((3, 1, 2, 3), NAN, np.float32)
  e2 = np.ones((3, 1, 2, 3), np.float32)
  e2[2] = np.float32(0.7)
  e2[2, 0, 1] = np.float32(0.7) * 2
  add('merge_3ch_dz0p7', [e1, e2], 0, 0, 0, 0.7)
  add('f64thr_merge_3ch_dz0p7', [e1, e2], 0, 0, 0, np.float64(0.7))

  arrs = {'names': np.array([n for n, *_ in cases])}
  for i, (name, flows, params, out) in enumerate(cases):
    arrs[f'flows_{i}'] = flows
    arrs[f'params_{i}'] = params
    arrs[f'out_{i}'] = out
  path = os.path.join(HERE, 'reconcile_flows.npz')
  np.savez_compressed(path, **arrs)
  print(f'reconcile_flows: {len(cases)} cases, {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
  main()
