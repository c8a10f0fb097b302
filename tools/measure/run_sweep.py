"""Patch-queue run length x single-patch tail of the correlation kernel on the bench
pairs: per setting the production launch time, the flow wall time
and the bench line's pruning counters, settings interleaved within every round.

  SOFIMA_AMD_LIB=$PWD/sofima_amd/lib/libsofima_amd_measure.so \
      python tools/measure/run_sweep.py [--rounds 3] [--steps 6] [--out FILE]

SFM_MFMA_RUN_TAIL is a measurement switch: with the production library only the
run length varies (the script says so).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--steps', type=int, default=6)
  ap.add_argument('--runs', default='4,8,16')
  ap.add_argument('--tails', default='2,4,8')
  ap.add_argument('--pairs', default='warped,exact')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  import torch
  import bench
  from sofima_amd import _abi, flow_field
  lib = _abi.load()
  has_tail = _abi.get_option('SFM_BUILD_MEASUREMENT_SWITCHES') == '1'
  tails = [int(v) for v in args.tails.split(',')] if has_tail else [None]
  if not has_tail:
    print('production library: SFM_MFMA_RUN_TAIL is ignored, the built-in tail is used')
  settings = [(1, None)] + [(int(c), t) for c in args.runs.split(',') for t in tails]
  calc = flow_field.JAXMaskedXCorrWithStatsCalculator()
  n_patches = ((8192 - (bench.PATCH - bench.STEP)) // bench.STEP) ** 2
  rows = []
  for pair in args.pairs.split(','):
    pre, post = bench.synth_pair(8192, 1002, warp=bench.WARP if pair == 'warped' else None)
    a, b = torch.from_numpy(pre).cuda(), torch.from_numpy(post).cuda()
    ref = None
    for rnd in range(args.rounds):
      for run, tail in settings:
        with _abi.option('SFM_MFMA_RUN', run), _abi.option('SFM_MFMA_RUN_TAIL', tail):
          flow = calc.flow_field(a, b, bench.PATCH, bench.STEP, batch_size=bench.BATCH)
          if ref is None:
            ref = flow
          assert np.array_equal(flow, ref, equal_nan=True), (pair, run, tail)
          torch.cuda.synchronize()
          pf = _abi.SfmProfile()
          lib.sfm_profile_read(C.byref(pf))
          lib.sfm_profile_enable(1)
          t0 = time.perf_counter()
          for _ in range(args.steps):
            calc.flow_field(a, b, bench.PATCH, bench.STEP, batch_size=bench.BATCH)
          torch.cuda.synchronize()
          wall = (time.perf_counter() - t0) / args.steps * 1e3
          lib.sfm_profile_enable(0)
          _abi.check(lib.sfm_profile_read(C.byref(pf)))
        drawn, skipped = int(pf.tiles_drawn[0]), int(pf.tiles_skipped[0])
        row = {
            'pair': pair, 'round': rnd, 'run': run, 'tail': tail,
            'launch_ms': round(pf.kernel_ms[0] / int(pf.launches[0]), 4),
            'flow_ms': round(wall, 4),
            'issued_over_algorithmic': round(
                int(pf.mfma_issued[0]) * 32768.0 /
                (2.0 * bench.PATCH ** 4 * n_patches * args.steps), 4),
            'row_tiles_skipped_frac': round(skipped / drawn, 4),
            'row_tiles_abandoned_frac': round(int(pf.tiles_abandoned[0]) / drawn, 4),
            'col_tiles_skipped_per_row_tile': round(
                int(pf.col_tiles_skipped[0]) / (drawn - skipped), 3),
        }
        rows.append(row)
        print(json.dumps(row), flush=True)
  # per setting: mean and spread over the rounds
  lines = ['pair run tail | launch ms mean (min .. max) | flow ms mean | issued/alg | '
           'skipped | abandoned | cols/tile']
  for pair in args.pairs.split(','):
    for run, tail in settings:
      sel = [r for r in rows if (r['pair'], r['run'], r['tail']) == (pair, run, tail)]
      lm = [r['launch_ms'] for r in sel]
      mean = lambda k: sum(r[k] for r in sel) / len(sel)
      lines.append('%-6s %3d %4s | %.3f (%.3f .. %.3f) | %.3f | %.4f | %.4f | %.4f | %.3f' % (
          pair, run, '-' if tail is None else tail, sum(lm) / len(lm), min(lm), max(lm),
          mean('flow_ms'), mean('issued_over_algorithmic'), mean('row_tiles_skipped_frac'),
          mean('row_tiles_abandoned_frac'), mean('col_tiles_skipped_per_row_tile')))
  text = '\n'.join(lines)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')
      for r in rows:
        f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
  main()
