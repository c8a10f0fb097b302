"""Device time of flow_utils.reconcile_flows against the host restatement.

Shapes: [2, Z, 205, 205] (an 8192^2 section at stride 40; Z = 1, 16, 100) and
[2, 1, 2048, 2048], two flows each, em_alignment.ipynb's parameters
(max_gradient=0, max_deviation=20, min_patch_size=400) and all three filters.
The device call is timed with torch events around back-to-back calls (inputs
already on the device; the time includes the workspace / output allocation and
the packing of the two flows), the host restatement (tests/test_reconcile.py,
NumPy / SciPy) with perf_counter.  Each device output is checked against the
host one.  Prints one JSON line per case.

  python tools/measure/reconcile_time.py [--reps 20]
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
from sofima_amd import _dev, flow_utils  # noqa: E402
from tests.test_reconcile import reconcile_restated  # noqa: E402


def make_flow(rng, z, y, x, hole_frac):
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, y, x)), (0, 2, 2)) * 20
                for _ in range(2)]).astype(np.float32)
  hit = rng.random((z, y, x)) < 0.03
  f[:, hit] += rng.uniform(-30, 30, (2, int(hit.sum()))).astype(np.float32)
  noise = ndimage.gaussian_filter(rng.standard_normal((z, y, x)), (0, 1.5, 1.5))
  f[:, noise < np.quantile(noise, hole_frac)] = np.nan
  return f


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  args = ap.parse_args()
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  rng = np.random.default_rng(0)
  for shape in ((1, 205, 205), (16, 205, 205), (100, 205, 205), (1, 2048, 2048)):
    host = [make_flow(rng, *shape, 0.3), make_flow(rng, *shape, 0.15)]
    flows = [_dev.DeviceArray(torch.from_numpy(f).to(dev)) for f in host]
    for params in ((0, 20, 400, 0), (3.0, 4.0, 400, 0)):
      got = np.asarray(flow_utils.reconcile_flows(flows, *params))   # warm-up + check
      t0 = time.perf_counter()
      want = reconcile_restated(host, *params)
      host_ms = (time.perf_counter() - t0) * 1e3
      ok = bool(np.array_equal(got, want, equal_nan=True))
      torch.cuda.synchronize()
      start = torch.cuda.Event(enable_timing=True)
      stop = torch.cuda.Event(enable_timing=True)
      start.record()
      for _ in range(args.reps):
        flow_utils.reconcile_flows(flows, *params)
      stop.record()
      stop.synchronize()
      dev_ms = start.elapsed_time(stop) / args.reps
      print(json.dumps({'shape': [2, *shape], 'flows': 2, 'params': params,
                        'device_ms': round(dev_ms, 4), 'host_ms': round(host_ms, 1),
                        'speedup': round(host_ms / dev_ms, 1), 'bit_exact': ok}),
            flush=True)


if __name__ == '__main__':
  main()
