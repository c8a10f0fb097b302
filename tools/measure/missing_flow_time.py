"""Device time of processor_flow.estimate_missing_flow against the same loop
assembled from the public calls that existed before it, and of its planning
step against device_plan().

A stack of four 8192^2 uint8 sections resident on the device, patch 160, stride
40, search radius 40 and 80, delta_z 1, max_delta_z 4; the flow is the one
section on top of the stack (look-backs 2 and 3 reach sections 1 and 0, 4
leaves the stack), with 5 % and 0.5 % of its nodes NaN in 5 x 5 blobs.  The
sections are unrelated noise and the magnitude limit is half the search
radius, so about a quarter of a round's nodes is accepted and the second round
still has work.  The forms are alternated in one process, torch events around
every call, 3 warm-up calls and `--reps` timed calls each:

  driver     estimate_missing_flow(device_output=True): sfm_flow_select +
             sfm_flow_starts, the correlation, sfm_flow_scatter,
             sfm_missing_flow_update; one integer read per round
  assembled  per round flow_field(selection_mask=<host mask>,
             device_output=True), flow_utils.clean_flow, torch element-wise
             updates, and the mask brought to the host for the next round.
             Timed twice in the alternation: the distance between the two
             medians is the spread the comparison has to beat
  plan       one round's planning alone: sfm_flow_select + sfm_flow_starts
             (with the read of n) against device_plan() fed the host mask

`one_round` is a call with max_delta_z 2 (a single look-back), `call` the whole
call (two look-backs).  The assembled result is checked against the driver's
before timing, bit for bit.  Prints one JSON line per case and writes them to
`--out`.

  python tools/measure/missing_flow_time.py [--reps 20] [--out profiles/missing_flow_time.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sofima_amd import flow_field as ff, flow_utils, processor_flow  # noqa: E402

SIZE, PATCH, STRIDE, BATCH = 8192, 160, 40, 1024
DELTA_Z, MAX_DELTA_Z, MAX_ATTEMPTS = 1, 4, 1
Z0 = 3      # the flow's section is the last of the four


def alternate(fns, reps):
  """Median ms of every fn, the fns called in turn."""
  for _ in range(3):
    for fn in fns:
      fn()
  torch.cuda.synchronize()
  times = [[] for _ in fns]
  for _ in range(reps):
    for i, fn in enumerate(fns):
      t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      t0.record()
      fn()
      t1.record()
      t1.synchronize()
      times[i].append(t0.elapsed_time(t1))
  return [float(np.median(t)) for t in times]


def blobs(rng, n, fraction):
  """[n, n] bool, about `fraction` of it True in 5 x 5 blobs."""
  holes = np.zeros((n, n), bool)
  while holes.mean() < fraction:
    y, x = rng.integers(0, n - 5, 2)
    holes[y:y + 5, x:x + 5] = True
  return holes


def assembled(flow, images, calc, radius, max_delta_z, thresholds):
  """processor/flow.py:666-828 through flow_field(), clean_flow and torch ops."""
  ratio, sharpness, magnitude = thresholds
  nz, ny, nx = flow.shape[1:]
  out = torch.empty((3, nz, ny, nx), dtype=torch.float32, device=flow.device)
  out[:2] = flow
  out[2] = float(DELTA_Z)
  size = (ny - 1) * STRIDE + PATCH
  for z in range(nz):
    ci = Z0 + z
    mask = ~torch.isfinite(out[0, z])
    attempts = torch.zeros((ny, nx), dtype=torch.int32, device=flow.device)
    curr = images[ci, radius:radius + size, radius:radius + size]
    for dz in processor_flow.search_deltas(DELTA_Z, max_delta_z):
      if ci - dz < 0:
        break
      mask &= attempts <= MAX_ATTEMPTS
      mask_h = mask.cpu().numpy()                  # the host round trip of a look-back
      if not mask_h.any():
        break
      field = calc.flow_field(images[ci - dz], curr, PATCH + 2 * radius, STRIDE,
                              selection_mask=mask_h, batch_size=BATCH, post_patch_size=PATCH,
                              device_output=True).tensor
      attempts += torch.isfinite(field[0]).int()
      clean = flow_utils.clean_flow(field[:, None], ratio, sharpness, magnitude, 0.0).tensor
      update = mask & torch.isfinite(clean[0, 0])
      out[0, z] = torch.where(update, clean[0, 0], out[0, z])
      out[1, z] = torch.where(update, clean[1, 0], out[1, z])
      out[2, z] = torch.where(update, float(dz), out[2, z])
      mask &= ~update
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'missing_flow_time.txt'))
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  dev = torch.device('cuda', torch.cuda.current_device())
  gen = torch.Generator(device=dev).manual_seed(0)
  images = torch.randint(0, 256, (4, SIZE, SIZE), generator=gen, device=dev, dtype=torch.uint8)
  calc = ff.JAXMaskedXCorrWithStatsCalculator()
  lines = []
  for radius in (40, 80):
    n = (SIZE - 2 * radius - PATCH) // STRIDE + 1
    thresholds = (0.0, 0.0, radius / 2)
    kw = dict(patch_size=PATCH, stride=STRIDE, delta_z=DELTA_Z, max_attempts=MAX_ATTEMPTS,
              search_radius=radius, min_peak_ratio=thresholds[0],
              min_peak_sharpness=thresholds[1], max_magnitude=thresholds[2], z0=Z0,
              batch_size=BATCH, calculator=calc, device_output=True)
    for fraction in (0.05, 0.005):
      holes = blobs(rng, n, fraction)
      flow_h = rng.uniform(-2, 2, (2, 1, n, n)).astype(np.float32)
      flow_h[:, 0, holes] = np.nan
      flow = torch.from_numpy(flow_h).to(dev)

      def driver(max_delta_z=MAX_DELTA_Z):
        return processor_flow.estimate_missing_flow(flow, images, max_delta_z=max_delta_z, **kw)

      got, filled = driver()
      want = assembled(flow, images, calc, radius, MAX_DELTA_Z, thresholds)
      assert torch.equal(got.tensor.view(torch.int32), want.view(torch.int32)), 'forms differ'
      assert filled[0, 0] > 0 and filled[0, 1] > 0 and filled[0, 2] == 0

      # planning alone, for the first round's selection
      sel_h = holes.copy()
      sel_d = torch.from_numpy(sel_h.astype(np.uint8)).to(dev)
      size = (n - 1) * STRIDE + PATCH
      curr = images[Z0, radius:radius + size, radius:radius + size].contiguous()
      res = ff._Resident.of_device(images[1], curr, None, None, ff._abi.DTYPE_U8, dev)
      capacity = -(-n * n // BATCH) * BATCH
      positions = torch.empty((capacity, 2), dtype=torch.int32, device=dev)
      counts = torch.empty((2,), dtype=torch.int32, device=dev)
      search = (PATCH + 2 * radius,) * 2

      def plan_select():
        processor_flow.select_patches(sel_d, BATCH, positions, counts)
        total = -(-int(counts[0].item()) // BATCH) * BATCH
        return processor_flow.patch_starts(positions, total, search, (PATCH,) * 2, (STRIDE,) * 2,
                                           (SIZE, SIZE), (size, size))

      def plan_device():
        return calc.device_plan(res, search, (STRIDE,) * 2, sel_h, 0.75, BATCH, (PATCH,) * 2)

      assert torch.equal(plan_select(), plan_device()['starts'])

      t = alternate([lambda: driver(2), lambda: assembled(flow, images, calc, radius, 2, thresholds),
                     driver, lambda: assembled(flow, images, calc, radius, MAX_DELTA_Z, thresholds),
                     lambda: assembled(flow, images, calc, radius, 2, thresholds),
                     lambda: assembled(flow, images, calc, radius, MAX_DELTA_Z, thresholds),
                     plan_select, plan_device], args.reps)
      lines.append(json.dumps({
          'search_radius': radius, 'grid': [n, n], 'nan_fraction': round(float(holes.mean()), 4),
          'nan_nodes': int(holes.sum()), 'filled_per_lookback': filled[0].tolist(),
          'reps': args.reps,
          'one_round_driver_ms': round(t[0], 4),
          'one_round_assembled_ms': [round(t[1], 4), round(t[4], 4)],
          'call_driver_ms': round(t[2], 4),
          'call_assembled_ms': [round(t[3], 4), round(t[5], 4)],
          'call_assembled_over_driver': round(min(t[3], t[5]) / t[2], 2),
          'plan_select_ms': round(t[6], 4), 'plan_device_plan_ms': round(t[7], 4)}))
      print(lines[-1], flush=True)
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
