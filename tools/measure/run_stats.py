"""Run statistics of the correlation launch on the bench pairs, from the timing build
(tools/measure/build_timing_lib.sh): redone tiles and seed-block hits, split into the
first patch of a run and the patches inside one (the kernel's RUNS line).

  SOFIMA_AMD_LIB=$PWD/sofima_amd/lib/libsofima_amd_timing.so \
      python tools/measure/run_stats.py [runs ...] | grep -a '^RUNS\|^=='
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))


def main():
  import torch
  import bench
  from sofima_amd import _abi, flow_field
  runs = [int(v) for v in sys.argv[1:]] or [1, 8]
  calc = flow_field.JAXMaskedXCorrWithStatsCalculator()
  for pair in ('warped', 'exact'):
    pre, post = bench.synth_pair(8192, 1002, warp=bench.WARP if pair == 'warped' else None)
    a, b = torch.from_numpy(pre).cuda(), torch.from_numpy(post).cuda()
    for run in runs:
      with _abi.option('SFM_MFMA_RUN', run):
        for rep in range(2):
          print(f'== pair {pair} SFM_MFMA_RUN={run} pass {rep}', flush=True)
          calc.flow_field(a, b, bench.PATCH, bench.STEP, batch_size=bench.BATCH)
          torch.cuda.synchronize()


if __name__ == '__main__':
  main()
