"""Device time of map_utils.resample_map against the SciPy route of the reference.

A 2 x upsampling of a flow lattice, 101^2 -> 201^2 (what ReconcileAndFilterFlows
does with a coarse flow of an 8192^2 section): [2, 1, 101, 101] and
[2, 64, 101, 101] in one call, the latter once without holes and once with 5 %
blob holes.  float32 input already on the device; the device call is timed
with torch events around back-to-back calls (the time includes the workspace /
output allocations and the one host sync of the status read), the host route
(tests/resample_map_scipy.py: Qhull Delaunay + LinearNDInterpolator per slice,
as the reference calls them) with perf_counter on the same host, on at most
`--host-slices` slices and scaled to the whole stack.  Each device output is
compared with the host one where both have the same answer (nodes and edges of
full cells).  Prints one JSON line per case.

  python tools/measure/resample_map_time.py [--reps 20] [--host-slices 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sofima_amd import map_utils  # noqa: E402
from sofima_amd._dev import DeviceArray  # noqa: E402
from tests import resample_map_scipy as rms  # noqa: E402


def make_flow(rng, z, n, holes):
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, n, n)), (0, 5, 5))
                for _ in range(2)])
  f = (f / np.abs(f).max() * 10).astype(np.float32)
  if holes:
    noise = ndimage.gaussian_filter(rng.standard_normal((z, n, n)), (0, 1.5, 1.5))
    f[:, noise > np.quantile(noise, 1 - holes)] = np.nan
  return f


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--host-slices', type=int, default=4)
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  n = 101
  for z, holes in ((1, 0.0), (64, 0.0), (64, 0.05)):
    cm = make_flow(rng, z, n, holes)
    src = rms.box((0, 0, 0), (n, n, z))
    dst = rms.box((0, 0, 0), (2 * n - 1, 2 * n - 1, z))
    x = DeviceArray(torch.from_numpy(cm).cuda())
    got = map_utils.resample_map(x, src, dst, 2, 1)   # warm-up (allocator)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.reps):
      got = map_utils.resample_map(x, src, dst, 2, 1)
    t1.record()
    torch.cuda.synchronize()
    rec = {'shape': [2, z, n, n], 'dst': [2 * n - 1, 2 * n - 1], 'holes': holes,
           'device_ms': round(t0.elapsed_time(t1) / args.reps, 4)}
    k = min(z, args.host_slices)
    if k > 0:
      h0 = time.perf_counter()
      want = rms.resample_restated(cm[:, :k], rms.box(src.start, (n, n, k)),
                                   rms.box(dst.start, dst.size[:2] + (k,)), 2, 1)
      rec['host_ms'] = round((time.perf_counter() - h0) * 1e3 * z / k, 1)
      rec['host_slices_timed'] = k
      got_h = np.asarray(got)[:, :k]
      valid = np.isfinite(cm[0, :k])
      full = valid[:, :-1, :-1] & valid[:, :-1, 1:] & valid[:, 1:, :-1] & valid[:, 1:, 1:]
      shared = np.zeros(got_h.shape[1:], bool)
      for a in range(3):
        for b in range(3):
          if a != 1 or b != 1:
            shared[:, a:a + 2 * n - 2:2, b:b + 2 * n - 2:2] |= full
      assert np.array_equal(np.isnan(got_h), np.isnan(want))
      rec['max_abs_diff_shared'] = float(np.max(np.abs(got_h[:, shared] - want[:, shared])))
      rec['nan_nodes'] = int(np.isnan(got_h[0]).sum())
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
  main()
