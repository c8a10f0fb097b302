"""Time of the montage fine-flow stage: one batched launch against one call set
per tile pair.

Workload: a 30 x 30 montage, 870 + 870 tile pairs of [4, 150, 14] and
[4, 14, 150] (3000^2 tiles, stride 20, 280 px overlaps), smoothed-noise flows
with 30 % holes, generated on the device from a seed.

  (a) filter_flow_maps (x and y pairs) + aggregate_arrays(device_output=True)
  (b) what the calls before the batched filter give: clean_flow +
      reconcile_flows per pair on DeviceArrays, the host aggregate_arrays, and
      the upload of fx / fy that TargetMeshFn does

Both forms run in one process, alternated as b, a, b: three warm-up rounds, then
the median of `--reps` rounds, a host clock around a device synchronise.  (b) is
timed twice per round, so the distance of its two medians is the spread.  (a) is
also timed on a 2 x 2 montage, where batching cannot help much.  Before timing,
the outputs of (a) and (b) are compared bit for bit.

  python tools/measure/tile_flows_time.py [--reps 20] [--out profiles/tile_flows_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sofima_amd import _build, _dev, flow_utils, stitch_elastic  # noqa: E402

CLEAN = dict(min_peak_ratio=1.4, min_peak_sharpness=1.4, max_magnitude=40, max_deviation=10)
RECONCILE = dict(max_gradient=0, max_deviation=10, min_patch_size=10)
STRIDE, TILE = (20, 20), (3000, 3000)


def smooth(t, passes=2):
  for _ in range(passes):
    t = torch.nn.functional.avg_pool2d(t, 5, stride=1, padding=2, count_include_pad=False)
  return t


def make_flows(gen, n, h, w, dev):
  """n tile-pair flows [4, h, w] as DeviceArrays: smooth vectors, peak
  statistics, 30 % of the vectors in NaN blobs."""
  vec = smooth(torch.randn((n, 2, h, w), generator=gen, device=dev)) * 40
  stats = torch.rand((n, 2, h, w), generator=gen, device=dev) * 4 + 0.5
  noise = smooth(torch.randn((n, 1, h, w), generator=gen, device=dev))
  holes = noise > torch.quantile(noise.reshape(n, -1), 0.7, dim=1).reshape(n, 1, 1, 1)
  f = torch.cat([vec, stats], dim=1)
  f = torch.where(holes, torch.full_like(f, float('nan')), f)
  return [_dev.DeviceArray(f[i].contiguous()) for i in range(n)]


def montage(gx, gy, seed, dev):
  gen = torch.Generator(device=dev)
  gen.manual_seed(seed)
  kx = [(x, y) for y in range(gy) for x in range(gx - 1)]
  ky = [(x, y) for y in range(gy - 1) for x in range(gx)]
  fx = dict(zip(kx, make_flows(gen, len(kx), 150, 14, dev)))
  fy = dict(zip(ky, make_flows(gen, len(ky), 14, 150, dev)))
  m = {'fx': fx, 'fy': fy, 'ox': {k: (-280, 0) for k in kx}, 'oy': {k: (0, -280) for k in ky},
       'cx': np.zeros((2, gy, gx)), 'cy': np.zeros((2, gy, gx)),
       'coords': [(x, y) for y in range(gy) for x in range(gx)],
       'coarse': np.zeros((2, gy, gx))}
  return m


def aggregate(m, fine_x, fine_y, device_output):
  return stitch_elastic.aggregate_arrays(
      (m['cx'], fine_x, m['ox']), (m['cy'], fine_y, m['oy']), m['coords'], m['coarse'],
      STRIDE, TILE, device_output=device_output)


def form_a(m):
  fine_x = stitch_elastic.filter_flow_maps(m['fx'], CLEAN, RECONCILE)
  fine_y = stitch_elastic.filter_flow_maps(m['fy'], CLEAN, RECONCILE)
  return aggregate(m, fine_x, fine_y, True)


def form_b(m, dev):
  fine = []
  for flows in (m['fx'], m['fy']):
    fine.append({k: np.asarray(flow_utils.reconcile_flows(
        [flow_utils.clean_flow(v.tensor[:, None], **CLEAN)], **RECONCILE))[:, 0]
                 for k, v in flows.items()})
  fx, fy, x, nbors, idx = aggregate(m, fine[0], fine[1], False)
  return (_dev.DeviceArray(_dev.as_device_f32(fx, dev, copy=False)),
          _dev.DeviceArray(_dev.as_device_f32(fy, dev, copy=False)), x, nbors, idx)


def timed(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) * 1e3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tile_flows_time.txt'))
  args = ap.parse_args()
  torch.cuda.set_device(0)
  dev = torch.device('cuda', 0)
  lines = [f'tile_flows_time: build {_build.source_hash()}, {torch.cuda.get_device_name(0)}, '
           f'warm-up 3, median of {args.reps}, clean {CLEAN}, reconcile {RECONCILE}',
           '| montage | pairs | (a) batched ms | (b) per pair ms, two medians | (b) / (a) |',
           '|---|---:|---:|---:|---:|']
  for gx, gy in ((30, 30), (2, 2)):
    m = montage(gx, gy, 1234, dev)
    a, b = form_a(m), form_b(m, dev)
    for i, name in enumerate(('fx', 'fy', 'x')):
      ga, gb = np.asarray(a[i]), np.asarray(b[i])
      assert ga.dtype == gb.dtype == np.float32 and ga.shape == gb.shape, name
      assert np.array_equal(ga.view(np.int32), gb.view(np.int32)), f'{name}: (a) != (b)'
    assert np.array_equal(a[3], b[3]) and a[4] == b[4]
    kept = float(np.isfinite(np.asarray(a[0])).mean())
    del a, b
    ta, tb1, tb2 = [], [], []
    for r in range(3 + args.reps):
      t = (timed(lambda: form_b(m, dev)), timed(lambda: form_a(m)),
           timed(lambda: form_b(m, dev)))
      if r >= 3:
        tb1.append(t[0])
        ta.append(t[1])
        tb2.append(t[2])
    ma, mb1, mb2 = (statistics.median(v) for v in (ta, tb1, tb2))
    lines.append(f'| {gx} x {gy} | {len(m["fx"]) + len(m["fy"])} | {ma:.2f} | '
                 f'{mb1:.1f} / {mb2:.1f} | {min(mb1, mb2) / ma:.1f} |')
    lines.append(f'  ({gx} x {gy}: outputs of (a) and (b) equal bit for bit; '
                 f'{kept:.2f} of the fx nodes keep a vector; (a) min {min(ta):.2f} max '
                 f'{max(ta):.2f} ms)')
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as f:
    f.write(text)


if __name__ == '__main__':
  main()
