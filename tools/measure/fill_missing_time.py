"""Device time of map_utils.fill_missing(extrapolate=True, interpolate_first=False)
and, as context, the reference function's time on the host for the same input.

Two inputs: a [3, 130, 74, 74] float64 volume of inverse-map size (a sheared
ellipsoid of valid nodes in a NaN shell, what the 3-D invert_map leaves) and a
[2, 64, 410, 410] float32 map (per slice a rotated rectangle with round holes).
Channel 0 of either holds the node's own flat index, so a filled node names its
source.

  python tools/measure/fill_missing_time.py [--reps 10] [--out FILE]
      device: the map resident (DeviceArray); torch events around `--reps`
      back-to-back calls after a warm-up of 3, so output and workspace allocation
      are included.  Checked: every filled node's source is valid and exactly as
      far as the nearest valid node that SciPy's k-d tree finds.
  python tools/measure/fill_missing_time.py --reference [--out FILE]
      host: the unmodified reference function (tests/golden/_refshim, needs the
      reference checkout), wall time of one call; the 2-channel map one slice at a
      time, which is the only way the reference takes it (map_utils.py:294).

Either run rewrites its own lines of FILE (default profiles/fill_missing_time.txt)
and keeps the other run's.  One JSON line per case.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def inputs():
  z, y, x = np.mgrid[:130, :74, :74]
  xs = x - 36.5 - 0.3 * (y - 36.5)
  valid = ((z - 64.5) / 60.0) ** 2 + ((y - 36.5) / 32.0) ** 2 + (xs / 28.0) ** 2 <= 1
  vol = np.stack([np.arange(valid.size, dtype=np.float64).reshape(valid.shape), 0.5 * y, -1.0 * x])
  vol[:, ~valid] = np.nan
  yield 'inverse-map volume', vol

  y, x = np.mgrid[:410, :410]
  flat = np.empty((2, 64, 410, 410), np.float32)
  flat[0] = np.arange(64 * 410 * 410, dtype=np.float32).reshape(64, 410, 410)   # < 2^24: exact
  flat[1] = 0.25 * x
  for k in range(64):
    a = 0.4 + 0.01 * k
    u = np.cos(a) * (x - 205) + np.sin(a) * (y - 205)
    v = -np.sin(a) * (x - 205) + np.cos(a) * (y - 205)
    ok = (np.abs(u) <= 190) & (np.abs(v) <= 150)
    ok &= (x - 150 - k) ** 2 + (y - 180) ** 2 > 30 ** 2
    ok &= (x - 280) ** 2 + (y - 240 + k) ** 2 > 12 ** 2
    flat[:, k][:, ~ok] = np.nan
  yield 'section maps', flat


def check_nearest(m, out):
  """Every node's source (channel 0 of `out`) is valid and at the k-d tree's distance."""
  from scipy import spatial
  dim = m.shape[0]
  # (of the 2-channel map every 21st slice: the tree takes the host a while)
  problems = [np.s_[k] for k in range(0, m.shape[1], 21)] if dim == 2 else [np.s_[:]]
  for sel in problems:
    valid = np.isfinite(m[(slice(None), sel)]).all(axis=0)
    coords = np.stack(np.nonzero(np.ones_like(valid)), axis=1)
    src = out[0][sel].ravel().astype(np.int64) - (sel * valid.size if dim == 2 else 0)
    assert src.min() >= 0 and src.max() < valid.size and valid.ravel()[src].all()
    d2 = ((coords - coords[src]) ** 2).sum(axis=1)
    want, _ = spatial.cKDTree(coords[valid.ravel()]).query(coords)
    assert np.array_equal(d2, np.rint(want ** 2).astype(np.int64))


def device(reps):
  import torch
  from sofima_amd import map_utils
  from sofima_amd._dev import DeviceArray
  kw = dict(extrapolate=True, interpolate_first=False)
  for name, m in inputs():
    dm = DeviceArray(torch.from_numpy(m).cuda())
    check_nearest(m, np.asarray(map_utils.fill_missing(dm, **kw)))
    for _ in range(3):
      map_utils.fill_missing(dm, **kw)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
      map_utils.fill_missing(dm, **kw)
    t1.record()
    torch.cuda.synchronize()
    yield {'where': 'device', 'case': name, 'shape': list(m.shape), 'dtype': str(m.dtype),
           'invalid_share': round(float(np.isnan(m[0]).mean()), 3),
           'ms': round(t0.elapsed_time(t1) / reps, 4)}


def reference():
  sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden', '_refshim'))
  import refshim
  refshim.install()
  from sofima import map_utils as rmu
  kw = dict(extrapolate=True, interpolate_first=False)
  for name, m in inputs():
    t = time.perf_counter()
    if m.shape[0] == 3:
      rmu.fill_missing(m, **kw)
    else:
      for k in range(m.shape[1]):
        rmu.fill_missing(m[:, k:k + 1], **kw)
    yield {'where': 'host, reference function', 'case': name, 'shape': list(m.shape),
           'dtype': str(m.dtype), 'ms': round((time.perf_counter() - t) * 1e3, 1)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--reference', action='store_true')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fill_missing_time.txt'))
  args = ap.parse_args()
  mine = list(reference() if args.reference else device(args.reps))
  kept = []
  if os.path.exists(args.out):
    with open(args.out) as f:
      kept = [json.loads(line) for line in f if line.strip()]
    kept = [r for r in kept if (r['where'] == 'device') == args.reference]
  rows = sorted(kept + mine, key=lambda r: (r['case'] != 'inverse-map volume', r['where'] != 'device'))
  with open(args.out, 'w') as f:
    for r in rows:
      f.write(json.dumps(r) + '\n')
      print(json.dumps(r), flush=True)


if __name__ == '__main__':
  main()
