"""Device time of the map geometry helpers against their bytes-moved model.

Maps already on the device (DeviceArray), as a driver holds them after
invert_map / compose_maps_fast.  Every call is timed with torch events around
`--reps` back-to-back calls after a warm-up of 3, so the time includes the
output / workspace allocation and, for the boxes, the one host read of the 8
result doubles.  The model is the bytes the algorithm has to move (DESIGN.md
§1.10); GB/s = model bytes / time.  Each result is checked once against the
NumPy statement of tests/mapgeom_ref.py on a [.., 2, 64, 96] corner of the
problem (the statement of the whole map would take minutes on the host).
warp_points is timed as the whole call: host-side section check, upload of
the points, kernel, download.  Prints one JSON line per case.

  python tools/measure/mapgeom_time.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sofima_amd import map_utils, warp  # noqa: E402
from sofima_amd._dev import DeviceArray  # noqa: E402
from tests import mapgeom_ref as ref  # noqa: E402


def timed(fn, reps):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0.record()
  for _ in range(reps):
    fn()
  t1.record()
  torch.cuda.synchronize()
  return t0.elapsed_time(t1) / reps


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  args = ap.parse_args()
  gen = torch.Generator(device='cuda').manual_seed(0)

  def report(case, shape, dtype, ms, model_bytes):
    print(json.dumps({'case': case, 'shape': list(shape), 'dtype': str(dtype).replace('torch.', ''),
                      'ms': round(ms, 4), 'model_MB': round(model_bytes / 1e6, 1),
                      'GB_per_s': round(model_bytes / ms / 1e6, 1)}), flush=True)

  for shape, dtype in (((2, 25, 2048, 2048), torch.float32), ((2, 1, 8192, 8192), torch.float32),
                       ((3, 256, 512, 512), torch.float32), ((2, 1, 205, 205), torch.float32),
                       ((2, 12, 2048, 2048), torch.float64)):
    dim = shape[0]
    stride = (30, 20, 40)[-dim:]
    m = (torch.rand(shape, generator=gen, device='cuda', dtype=torch.float32) * 18 - 9).to(dtype)
    box = ref.Box((-400, 11, -3), shape[1:][::-1])
    dm = DeviceArray(m)
    e = m.element_size()
    # correctness on a corner, with its own box
    corner = m[:, :2, :64, :96].contiguous()
    cbox = ref.Box((-400, 11, -3), corner.shape[1:][::-1])
    ch = corner.cpu().numpy()
    assert np.array_equal(np.asarray(map_utils.to_absolute(DeviceArray(corner), stride, cbox)),
                          ref.to_absolute(ch, stride, cbox))
    for name in ('outer_box', 'inner_box'):
      got = getattr(map_utils, name)(DeviceArray(corner), cbox, stride)
      want = getattr(ref, name)(ch, cbox, stride)
      assert np.array_equal(got.start, want.start) and np.array_equal(got.size, want.size), name
    report('to_absolute', shape, dtype, timed(lambda: map_utils.to_absolute(dm, stride, box),
                                              args.reps), 2 * m.numel() * e)
    report('outer_box', shape, dtype, timed(lambda: map_utils.outer_box(dm, box, stride),
                                            args.reps), m.numel() * e)
    report('inner_box', shape, dtype, timed(lambda: map_utils.inner_box(dm, box, stride),
                                            args.reps), m.numel() * e)
    del m, dm

  mat = np.random.default_rng(0).uniform(-1.5, 1.5, (3, 4))
  for size in ((512, 512, 256), (205, 205, 1)):
    box = ref.Box((-13, 21, 5), size)
    small = ref.Box((-13, 21, 5), (96, 64, 2))
    assert np.array_equal(np.asarray(map_utils.make_affine_map(mat, small, (2.5, 20, 40))),
                          ref.make_affine_map(mat, small, (2.5, 20, 40)))
    report('make_affine_map', (3,) + size[::-1], torch.float64,
           timed(lambda: map_utils.make_affine_map(mat, box, (2.5, 20, 40)), args.reps),
           3 * int(np.prod(size)) * 8)

  rng = np.random.default_rng(1)
  shape = (2, 16, 205, 205)
  m = rng.uniform(-15, 15, shape).astype(np.float32)
  box = ref.Box((5, -3, 10), shape[1:][::-1])
  dm = DeviceArray(torch.from_numpy(m).cuda())
  for n in (10**4, 10**6):
    pts = np.concatenate([rng.uniform([150, -150], [8300, 8000], (n, 2)),
                          rng.integers(10, 26, (n, 1))], axis=1).astype(np.float32)
    ref.check_points_float(warp.warp_points(pts[:5000], dm, box, 40),
                           ref.warp_points(pts[:5000], m, box, 40))
    # per point: 12 bytes up, 4 section bytes up, 12 in / 8 out in the kernel, 8 node reads, 12 down
    report(f'warp_points n={n} (whole call)', shape, torch.float32,
           timed(lambda: warp.warp_points(pts, dm, box, 40), max(args.reps // 4, 3)),
           n * (12 + 4 + 8 + 8 * 4))


if __name__ == '__main__':
  main()
