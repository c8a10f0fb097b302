"""Device time of map_utils.invert_map against the SciPy statement.

Shapes: [2, 1, 205, 205] and [2, 16, 205, 205] (an 8192^2 section at stride
40) and [2, 1, 1024, 1024], smooth deformations of 0.5 x stride, dst box one
node larger on each side (as warp.render_tiles uses it).  The device call is
timed with torch events around back-to-back calls (input already on the
device as float64; the time includes the workspace / output allocations and
the one host sync of the status read), the host statement
(tests/invert_map_scipy.py: Qhull Delaunay + LinearNDInterpolator) with
perf_counter.  Each device output is checked against the host one under the
parity contract.  Prints one JSON line per case.

  python tools/measure/invert_map_time.py [--reps 20]
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
from tests import invert_map_scipy as ims  # noqa: E402


def make_map(rng, z, h, w, amp):
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, h, w)), (0, 6, 6))
                for _ in range(2)])
  return f / np.abs(f).max() * amp


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--no-host', action='store_true')
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  stride = 40
  for z, n in ((1, 205), (16, 205), (1, 1024)):
    cm = make_map(rng, z, n, n, 0.5 * stride)
    src = ims.box((0, 0, 0), (n, n, z))
    dst = ims.box((-1, -1, 0), (n + 2, n + 2, z))
    x = DeviceArray(torch.from_numpy(cm).cuda())
    got = map_utils.invert_map(x, src, dst, stride)   # warm-up (build, allocator)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.reps):
      got = map_utils.invert_map(x, src, dst, stride)
    t1.record()
    torch.cuda.synchronize()
    dev_ms = t0.elapsed_time(t1) / args.reps
    rec = {'shape': [2, z, n, n], 'device_ms': round(dev_ms, 4)}
    if not args.no_host:
      h0 = time.perf_counter()
      want = ims.invert_restated(cm, src, dst, stride)
      rec['host_ms'] = round((time.perf_counter() - h0) * 1e3, 1)
      rec['diag_exceptions'] = ims.check_contract(cm, src, dst, stride, np.asarray(got), want)
      rec['nan_nodes'] = int(np.isnan(np.asarray(got)[0]).sum())
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
  main()
