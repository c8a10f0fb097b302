"""Device time of the B-spline prefilter and of the order-3 warp under every boundary
mode, next to 'mirror' on the same build.

`warp.affine_transform(order=3, mode=...)` of a resident uint8 image, one 2-D shape
(4096 x 4096) and one 3-D shape (z, y, x = 128, 512, 512), a small turn with shear about
the centre.  Per mode two figures, by HIP events (torch.cuda.Event) recorded around the
calls inside `affine_transform`: `prefilter_ms`, the launches of `_spline.prefilter` (one
per axis), and `warp_ms`, the launch of sfm_affine_warp.  2 warm-up rounds, `--reps`
timed ones, the modes alternating inside a round in one process; the median and the
spread (max - min) are reported, with the ratio to 'mirror' and, for the modes that
filter a padded image, the volume ratio prod (n + 24) / n that the padding adds.

What to expect is derived, not a threshold: 'reflect' is the mirror recursion with one
more term; 'grid-wrap' adds one sweep of the line to the x pass (and re-reads the line in
the z and y passes); 'nearest' and 'grid-constant' filter and sample the padded volume.

  python tools/measure/spline_modes_time.py [--reps 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sofima_amd import _abi, _spline, warp  # noqa: E402

SHAPES = ((4096, 4096), (128, 512, 512))
MODES = ('mirror', 'reflect', 'grid-wrap', 'nearest', 'grid-constant')
ORDER = 3


class Events:
  """HIP events around sfm_affine_warp and _spline.prefilter."""

  def __init__(self):
    self._lib = _abi.load()
    self._pending = []

  def _wrap(self, name, fn):
    def wrapped(*args, **kwargs):
      t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      t0.record()
      out = fn(*args, **kwargs)
      t1.record()
      self._pending.append((name, t0, t1))
      return out
    return wrapped

  def __enter__(self):
    self._warp = self._lib.sfm_affine_warp
    self._prefilter = _spline.prefilter
    self._lib.sfm_affine_warp = self._wrap('warp', self._warp)
    _spline.prefilter = self._wrap('prefilter', self._prefilter)
    return self

  def __exit__(self, *exc):
    self._lib.sfm_affine_warp = self._warp
    _spline.prefilter = self._prefilter
    return False

  def take(self):
    torch.cuda.synchronize()
    out = {name: t0.elapsed_time(t1) for name, t0, t1 in self._pending}
    self._pending = []
    return out


def matrix(shape):
  dim = len(shape)
  a = 0.05
  m = np.eye(dim)
  m[-2:, -2:] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
  m[-1, -2] += 0.02
  centre = (np.array(shape) - 1) / 2.0
  return m, centre - m @ centre


def stats(ts):
  return round(float(np.median(ts)), 3), round(float(max(ts) - min(ts)), 3)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spline_modes_time.txt'))
  args = ap.parse_args()
  _abi.set_option(_spline.OPTION, 1)
  _abi.set_option(_spline.MODES_OPTION, 1)
  rng = np.random.default_rng(0)
  lines = []
  for shape in SHAPES:
    img_t = torch.from_numpy(rng.integers(0, 256, shape).astype(np.uint8)).to('cuda')
    m, off = matrix(shape)
    times = {mode: {'prefilter': [], 'warp': []} for mode in MODES}
    with Events() as ev:
      for rep in range(2 + args.reps):
        for mode in MODES:
          out = warp.affine_transform(img_t, m, off, order=ORDER, mode=mode, cval=7.0,
                                      device_output=True)
          parts = ev.take()
          if rep >= 2:
            for key in ('prefilter', 'warp'):
              times[mode][key].append(parts[key])
          del out
    for mode in MODES:
      line = {'shape': list(shape), 'dtype': 'uint8', 'order': ORDER, 'mode': mode,
              'reps': args.reps}
      for key in ('prefilter', 'warp'):
        line[f'{key}_ms'], line[f'{key}_spread_ms'] = stats(times[mode][key])
        line[f'{key}_over_mirror'] = round(
            line[f'{key}_ms'] / stats(times['mirror'][key])[0], 2)
      pad = _spline.mode_pad(mode)
      line['padded_volume_ratio'] = round(float(np.prod([(n + 2 * pad) / n for n in shape])), 3)
      lines.append(json.dumps(line))
      print(lines[-1], flush=True)
    del img_t
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
