"""Device time of the fused reference-position call against the same result
assembled from the existing public ops.

One section of [205, 205] and of [2048, 2048] nodes, K = 3 flows: two 2-channel
flows and one 3-channel flow whose third channel names one of four look-backs
(or none).  Flows and solved meshes are section planes of [c, nz, y, x] device
volumes with nz = 4, as the section driver holds them.  The forms are
alternated in one process, torch events around every call, 3 warm-up calls
and `--reps` timed calls each:

  fused      processor_mesh.compose_average (sfm_prev_state, one launch) +
             map_utils.mask_irregular_f64 (two launches), timed without and
             with the host read of the valid-node count that the driver does
  assembled  one map_utils.compose_maps_fast launch per (flow, look-back) over
             the whole plane, torch element-wise ops for the per-node choice,
             nan_to_num, counts and the float64 mean, and
             map_utils.mask_irregular, which narrows the mean to float32 and
             brings its mask to the host

The assembled form is checked against the fused one before timing: the means
value for value, NaN where NaN.  The model is the bytes the fused call has to
move: K flows x c channel planes x 4 bytes read, 2 planes x
8 bytes written, the bilinear taps served from cache; GB/s = model bytes /
median time of the compose-and-average call.  Prints one JSON line per case.

  python tools/measure/prev_state_time.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from sofima_amd import map_utils, processor_mesh  # noqa: E402

STRIDE = (40.0, 40.0)
OFFSETS = (1, 2, 3, 4)


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


def assembled_mean(flows, tables):
  """processor/mesh.py:331-371 with the existing ops; float64 [2, y, x]."""
  prev = torch.zeros((2,) + tuple(flows[0].shape[1:]), dtype=torch.float64, device='cuda')
  count = torch.zeros(tuple(flows[0].shape[1:]), dtype=torch.int32, device='cuda')
  for flow, table in zip(flows, tables):
    if flow.shape[0] == 2:
      ref = map_utils.compose_maps_fast(flow[:, None], (0, 0), STRIDE, table[0][1][:, None],
                                        (0, 0), STRIDE).tensor[:, 0]
    else:
      ref = torch.full_like(prev, float('nan'))
      for dz, mesh in table:
        m = flow[2] == dz
        curr = torch.where(m, flow[:2], float('nan'))
        curr = map_utils.compose_maps_fast(curr[:, None], (0, 0), STRIDE, mesh[:, None], (0, 0),
                                           STRIDE).tensor[:, 0]
        ref = torch.where(m, curr.double(), ref)
    count += torch.isfinite(ref[0]).int()
    prev += torch.nan_to_num(ref).double()
  count = count.float()
  count[count == 0] = float('nan')
  return prev / count


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  args = ap.parse_args()
  gen = torch.Generator(device='cuda').manual_seed(0)

  def rand(shape, amp):
    return (torch.rand(shape, generator=gen, device='cuda') * 2 - 1) * amp

  for shape in ((205, 205), (2048, 2048)):
    n = shape[0] * shape[1]
    nz = 4

    def plane(c, amp):      # section 1 of a [c, nz, y, x] volume: not contiguous
      return rand((c, nz) + shape, amp)[:, 1]

    flows = [plane(2, 30.0), plane(2, 30.0), plane(3, 30.0)]
    for f in flows:
      f[:2][:, torch.rand(shape, generator=gen, device='cuda') < 0.05] = float('nan')
    dz = torch.randint(0, 6, shape, generator=gen, device='cuda').float()   # 0, 5: no section
    flows[2][2] = dz
    meshes = [plane(2, 20.0) for _ in range(2 + len(OFFSETS))]
    tables = [[(1, meshes[0])], [(2, meshes[1])],
              [(o, meshes[2 + i]) for i, o in enumerate(OFFSETS)]]

    want = processor_mesh.compose_average(flows, tables, STRIDE)
    got = assembled_mean(flows, tables)
    nan = torch.isnan(want)
    assert torch.equal(nan, torch.isnan(got)) and torch.equal(want[~nan], got[~nan]), \
        'forms differ'
    assert nan.any() and not nan.all()

    def fused_average():
      return processor_mesh.compose_average(flows, tables, STRIDE)

    def fused():
      map_utils.mask_irregular_f64(fused_average(), STRIDE, 0.5, 1.5, dilation_iters=1)

    def fused_read():
      _, n_valid = map_utils.mask_irregular_f64(fused_average(), STRIDE, 0.5, 1.5,
                                                dilation_iters=1)
      return n_valid.item()

    def assembled():
      map_utils.mask_irregular(assembled_mean(flows, tables), STRIDE, 0.5, 1.5, dilation_iters=1)

    t_avg, t_fused, t_read, t_asm = alternate([fused_average, fused, fused_read, assembled],
                                              args.reps)
    channels = sum(f.shape[0] for f in flows)
    model = channels * n * 4 + 2 * n * 8
    print(json.dumps({
        'shape': list(shape), 'flows': len(flows), 'channel_planes': channels,
        'lookbacks': len(OFFSETS), 'reps': args.reps,
        'fused_average_ms': round(t_avg, 4), 'fused_with_mask_ms': round(t_fused, 4),
        'fused_with_mask_and_read_ms': round(t_read, 4),
        'assembled_with_mask_ms': round(t_asm, 4),
        'assembled_over_fused_with_read': round(t_asm / t_read, 2),
        'model_MB': round(model / 1e6, 3),
        'fused_average_GB_per_s': round(model / t_avg / 1e6, 1)}), flush=True)


if __name__ == '__main__':
  main()
