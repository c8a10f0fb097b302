"""Device time of map_utils.compose_maps and of the cross-block reconcile built on
it, with the SciPy route of the reference on the same host for scale.

  compose    whole public calls on resident float32 maps, 101^2 against 101^2
             at stride 40 (a mesh of a 4000^2 section): map1 smooth within
             +-30 px, map2 smooth, once without holes and once with 5 % blob
             holes.  For the holes case the size of the leftover list (queries
             that no triangle of the lattice part contains, inside the box of
             the valid nodes) and the number of triangles outside the lattice
             part, both derived on the host from the same maps.
  reconcile  a block of 8 sections (7 interior, z_map {0: 0, 8: 1}, box z 0 .. 8)
             through processor_maps.reconcile_cross_block_maps (two launches for
             the interior) next to the same block as a loop of single public
             calls in the reference's statement order.

The device calls are timed with torch events around back-to-back calls (the
time includes the workspace / output allocations and the host sync of each
status read); the host route (tests/compose_maps_scipy.py: Qhull Delaunay +
LinearNDInterpolator, as the reference calls them) with perf_counter.  The
parent commit has no device path, so no threshold is set: the numbers are
written down.  Prints one JSON line per case and writes them to --out.

  python tools/measure/compose_maps_time.py [--reps 20] [--out profiles/compose_maps_time.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sofima_amd import map_utils, processor_maps  # noqa: E402
from sofima_amd._dev import DeviceArray  # noqa: E402
from tests import compose_maps_scipy as cms  # noqa: E402

N, STRIDE = 101, 40


def smooth(rng, z, amp):
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, N, N)), (0, 5, 5))
                for _ in range(2)])
  return (f / np.abs(f).max() * amp).astype(np.float32)


def blobs(rng, z, frac):
  noise = ndimage.gaussian_filter(rng.standard_normal((z, N, N)), (0, 1.5, 1.5))
  return noise > np.quantile(noise, 1 - frac)


def device_ms(fn, reps):
  fn()   # warm-up (allocator)
  torch.cuda.synchronize()
  t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  t0.record()
  for _ in range(reps):
    out = fn()
  t1.record()
  torch.cuda.synchronize()
  return round(t0.elapsed_time(t1) / reps, 4), out


def leftover_and_triangles(m1, m2, b):
  """(leftover queries, triangles outside the lattice part) of one slice, on
  the host: the finite queries inside the box of the valid nodes less those in
  a full cell; 2 n - 2 - h triangles of n valid nodes with h on the hull, less
  two per full quad."""
  from scipy import spatial
  abs1 = cms.to_absolute(m1, STRIDE, b).astype(np.float64)
  valid = np.isfinite(m2).all(axis=0)[0]
  pos = cms.lattice((N, N), b, STRIDE)[valid.ravel()]
  _, full = cms.bd_cells(m1, b, STRIDE, m2, b, STRIDE)
  qx, qy = abs1[0, 0], abs1[1, 0]
  inbox = ((qx >= pos[:, 0].min()) & (qx <= pos[:, 0].max()) & (qy >= pos[:, 1].min()) &
           (qy <= pos[:, 1].max()))
  quads = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, :-1] & valid[1:, 1:]
  eq = spatial.ConvexHull(pos).equations
  on_hull = int((np.max(pos @ eq[:, :2].T + eq[:, 2], axis=1) > -1e-9).sum())
  return int((inbox & ~full[0]).sum()), int(2 * len(pos) - 2 - on_hull - 2 * quads.sum())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'compose_maps_time.txt'))
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  lines = []

  def emit(rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)

  b = cms.box((0, 0, 0), (N, N, 1))
  for holes in (0.0, 0.05):
    m1, m2 = smooth(rng, 1, 30.0), smooth(rng, 1, 10.0)
    if holes:
      m2[:, blobs(rng, 1, holes)] = np.nan
    d1, d2 = DeviceArray(torch.from_numpy(m1).cuda()), DeviceArray(torch.from_numpy(m2).cuda())
    ms, got = device_ms(lambda: map_utils.compose_maps(d1, b, STRIDE, d2, b, STRIDE), args.reps)
    h0 = time.perf_counter()
    want = cms.compose_restated(m1, b, STRIDE, m2, b, STRIDE)
    host = round((time.perf_counter() - h0) * 1e3, 1)
    got = np.asarray(got)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ref, full = cms.bd_cells(m1, b, STRIDE, m2, b, STRIDE)
    rec = {'case': 'compose', 'shape': [2, 1, N, N], 'stride': STRIDE, 'holes': holes,
           'device_ms': ms, 'host_ms': host, 'nan_nodes': int(np.isnan(got[0]).sum()),
           'max_abs_diff_full_cells': float(np.max(np.abs(got.astype(np.float64) - ref)[:, full]))}
    if holes:
      rec['leftover_queries'], rec['triangles_outside_lattice'] = leftover_and_triangles(m1, m2, b)
    emit(rec)

  # -- an 8-section block ----------------------------------------------------------
  z_map = {0: 0, 8: 1}
  box = cms.box((0, 0, 0), (N, N, 9))
  flat = cms.box((0, 0, 0), (N, N, 1))
  vols = {'cross_block': smooth(rng, 2, 10.0), 'cross_block_inv': smooth(rng, 2, 10.0),
          'last_inv': smooth(rng, 9, 10.0), 'main_inv': smooth(rng, 9, 10.0)}
  vols['cross_block'][:, blobs(rng, 2, 0.05)] = np.nan
  dev = {k: torch.from_numpy(v).cuda() for k, v in vols.items()}
  load = {k: (lambda z, t=t: DeviceArray(t[:, z:z + 1].contiguous())) for k, t in dev.items()}
  data = DeviceArray(torch.from_numpy(smooth(rng, 9, 30.0)).cuda())

  def batched():
    return processor_maps.reconcile_cross_block_maps(data, box, z_map=z_map, stride=STRIDE, **load)

  def looped():
    # forward, one block (0, 8) after the degenerate (0, 0): the reference's statements
    post = load['cross_block'](1)
    pre = DeviceArray(torch.zeros_like(post.tensor))
    end_inv = load['main_inv'](8)
    c = lambda m1, m2: map_utils.compose_maps(m1, flat, STRIDE, m2, flat, STRIDE)
    offset = c(c(pre, end_inv), post)
    out = data.tensor.clone()
    out[:, 0:1] = load['cross_block'](0).tensor
    out[:, 8:9] = post.tensor
    for i in range(1, 8):
      aligned = c(DeviceArray(out[:, i:i + 1].contiguous()), pre)
      out[:, i:i + 1] = c(aligned, DeviceArray(offset.tensor * (i / 8))).tensor
    return DeviceArray(out)

  ms_b, got_b = device_ms(batched, args.reps)
  ms_l, got_l = device_ms(looped, args.reps)
  same = bool(torch.equal(torch.nan_to_num(got_b.tensor[:, 1:8]),
                          torch.nan_to_num(got_l.tensor[:, 1:8])))
  host_data = np.asarray(data)
  h0 = time.perf_counter()
  pre = np.zeros_like(vols['cross_block'][:, :1])
  hc = lambda m1, m2: cms.compose_restated(m1, flat, STRIDE, m2, flat, STRIDE)
  offset = hc(hc(pre, vols['main_inv'][:, 8:9]), vols['cross_block'][:, 1:2])
  for i in range(1, 8):
    hc(hc(host_data[:, i:i + 1], pre), offset * (i / 8))
  host = round((time.perf_counter() - h0) * 1e3, 1)
  emit({'case': 'reconcile_block', 'sections': 9, 'interior': 7, 'shape': [2, 9, N, N],
        'stride': STRIDE, 'batched_ms': ms_b, 'loop_of_public_calls_ms': ms_l,
        'interior_bit_identical': same, 'host_ms': host,
        'finite_interior': float(torch.isfinite(got_b.tensor[:, 1:8]).float().mean())})
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
