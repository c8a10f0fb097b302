"""Device time of spline order 3 against order 1: `warp.ndimage_warp`, the fused 3-D
tile render, and the B-spline prefilter alone.

  warp    one warp.ndimage_warp of a [128, 288, 288] uint8 volume (a smooth map of a
          few voxels, mesh stride (8, 16, 16)): the whole call as a caller sees it
          (upload, kernels, the result back on the host; wall clock) at order 1 and
          order 3, the same call in SciPy on this machine's CPU
          (oracle.warp_oracle.ndimage_warp, one run per order), and the two device
          parts of order 3 on their own
  render  the output box of tools/measure/render3d_time.py (512 x 512 x 128 over a
          2 x 2 grid of [128, 288, 288] uint8 tiles, everything resident, the plan
          given): TileRenderer.render at order 1 and order 3, and the two device
          parts of order 3
  plane   the prefilter of one 8192 x 8192 uint8 image, order 3: 8192 lines per
          pass, one thread each -- the known limit of the line-parallel scheme

The device parts are taken with HIP events (torch.cuda.Event) recorded around the
two steps inside the call: `prefilter` is _spline.prefilter (the table upload and one
launch per axis), `sample` the one launch of sfm_ndimage_warp_rel at order 3 (the entry
every float32 / float64 map takes, at either order) / sfm_render_tiles3d_spline.  2 warm-up calls, `--reps` timed ones; the median and the
spread (max - min) are reported.  Orders 1 and 3 alternate in one process.  One JSON
line per section goes to profiles/ndwarp_spline_time.txt.

  python tools/measure/ndwarp_spline_time.py [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import warp_oracle  # noqa: E402
from sofima_amd import _abi, _dev, _spline, processor_warp, warp  # noqa: E402
import render3d_time  # noqa: E402

VOLUME = (128, 288, 288)
STRIDE = (8, 16, 16)
PLANE = 8192


class Parts:
  """HIP events around _spline.prefilter and the sampling launch of a call."""

  def __init__(self):
    self.times = {'prefilter': [], 'sample': []}
    self._pending = []
    self._lib = _abi.load()

  def _wrap(self, name, fn, spline_only=False):
    def wrapped(*args, **kwargs):
      if spline_only and args[0]._obj.order < 2:     # byref(desc): the order-1 calls
        return fn(*args, **kwargs)
      t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      t0.record()
      out = fn(*args, **kwargs)
      t1.record()
      self._pending.append((name, t0, t1))
      return out
    return wrapped

  def __enter__(self):
    self._saved = (_spline.prefilter, self._lib.sfm_ndimage_warp_rel,
                   self._lib.sfm_render_tiles3d_spline)
    _spline.prefilter = self._wrap('prefilter', self._saved[0])
    self._lib.sfm_ndimage_warp_rel = self._wrap('sample', self._saved[1], spline_only=True)
    self._lib.sfm_render_tiles3d_spline = self._wrap('sample', self._saved[2])
    return self

  def __exit__(self, *exc):
    (_spline.prefilter, self._lib.sfm_ndimage_warp_rel,
     self._lib.sfm_render_tiles3d_spline) = self._saved
    return False

  def collect(self):
    torch.cuda.synchronize()
    for name, t0, t1 in self._pending:
      self.times[name].append(t0.elapsed_time(t1))
    self._pending = []


def stats(ts):
  return round(float(np.median(ts)), 3), round(float(max(ts) - min(ts)), 3)


def wall(fn):
  torch.cuda.synchronize()
  t = time.perf_counter()
  fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) * 1e3


def section_warp(reps):
  rng = np.random.default_rng(0)
  img = rng.integers(0, 256, VOLUME).astype(np.uint8)
  nodes = tuple(n // s + 1 for n, s in zip(VOLUME, STRIDE))
  z, y, x = np.mgrid[:nodes[0], :nodes[1], :nodes[2]].astype(np.float64)
  cmap = np.stack([2.5 * np.sin(y / 3.0) + np.cos(z / 2.0), 2.0 * np.cos(x / 4.0) - np.sin(z / 3.0),
                   1.2 * np.sin(x / 5.0 + y / 4.0)]).astype(np.float32)
  args = (img, cmap, STRIDE, (128,) * 3, (0,) * 3)
  t = time.perf_counter()
  want1 = warp_oracle.ndimage_warp(img, cmap, STRIDE, order=1)
  scipy1 = (time.perf_counter() - t) * 1e3
  t = time.perf_counter()
  want3 = warp_oracle.ndimage_warp(img, cmap, STRIDE, order=3)
  scipy3 = (time.perf_counter() - t) * 1e3
  assert np.array_equal(warp.ndimage_warp(*args, order=1), want1)
  assert np.array_equal(warp.ndimage_warp(*args, order=3), want3)
  assert np.mean(want3 != want1) > 0.25
  for _ in range(2):
    warp.ndimage_warp(*args, order=1)
    warp.ndimage_warp(*args, order=3)
  calls = {1: [], 3: []}
  with Parts() as parts:
    for _ in range(reps):
      for order in (1, 3):
        calls[order].append(wall(lambda: warp.ndimage_warp(*args, order=order)))
      parts.collect()
  (c1, c1s), (c3, c3s) = stats(calls[1]), stats(calls[3])
  (pf, pfs), (sm, sms) = stats(parts.times['prefilter']), stats(parts.times['sample'])
  voxels = int(np.prod(VOLUME))
  return {'section': 'warp', 'volume': list(VOLUME), 'dtype': 'uint8', 'reps': reps,
          'order1_call_ms': c1, 'order1_call_spread_ms': c1s,
          'order3_call_ms': c3, 'order3_call_spread_ms': c3s,
          'order3_prefilter_ms': pf, 'order3_prefilter_spread_ms': pfs,
          'order3_sample_ms': sm, 'order3_sample_spread_ms': sms,
          'prefilter_Gvoxel_s': round(voxels / pf / 1e6, 2),
          'coefficient_bytes': 8 * voxels,
          'scipy_cpu_order1_ms': round(scipy1, 1), 'scipy_cpu_order3_ms': round(scipy3, 1),
          'scipy_over_call_order3': round(scipy3 / c3, 1)}


def section_render(reps):
  tiles, meshes, inverted, xy = render3d_time.montage()
  b = render3d_time.box(*render3d_time.BOX)
  r = {order: processor_warp.TileRenderer(tiles, meshes, xy, inverted, render3d_time.STRIDE,
                                          order=order) for order in (1, 3)}
  plan = r[1].plan(b)
  assert [item[0] for item in plan] == [0, 1, 2, 3]
  got = {order: np.asarray(r[order].render(b, plan=plan)) for order in (1, 3)}
  assert np.mean(got[3] != 0) > 0.9 and np.mean(got[3] != got[1]) > 0.25
  for _ in range(2):
    for order in (1, 3):
      r[order].render(b, device_output=True, plan=plan)
  calls = {1: [], 3: []}
  with Parts() as parts:
    for _ in range(reps):
      for order in (1, 3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        r[order].render(b, device_output=True, plan=plan)
        t1.record()
        t1.synchronize()
        calls[order].append(t0.elapsed_time(t1))
      parts.collect()
  (c1, c1s), (c3, c3s) = stats(calls[1]), stats(calls[3])
  (pf, pfs), (sm, sms) = stats(parts.times['prefilter']), stats(parts.times['sample'])
  crop_voxels = int(sum(np.prod(item[1].size) for item in plan))
  return {'section': 'render', 'box': [int(v) for v in b.size], 'tiles': 4,
          'tile_shape': list(render3d_time.TILE), 'dtype': 'uint8', 'reps': reps,
          'order1_render_ms': c1, 'order1_render_spread_ms': c1s,
          'order3_render_ms': c3, 'order3_render_spread_ms': c3s,
          'order3_prefilter_ms': pf, 'order3_prefilter_spread_ms': pfs,
          'order3_sample_ms': sm, 'order3_sample_spread_ms': sms,
          'crop_voxels': crop_voxels, 'coefficient_bytes': 8 * crop_voxels,
          'order3_over_order1': round(c3 / c1, 1)}


def section_plane(reps):
  dev = _dev.device()
  rng = np.random.default_rng(1)
  img = torch.from_numpy(rng.integers(0, 256, (PLANE, PLANE)).astype(np.uint8)).to(dev)
  region = [(img.data_ptr(), (1, PLANE, PLANE), (PLANE * PLANE, PLANE, 1))]
  times = []
  for k in range(2 + reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    ws, _ = _spline.prefilter(region, _abi.DTYPE_U8, 3, dev)
    t1.record()
    t1.synchronize()
    if k >= 2:
      times.append(t0.elapsed_time(t1))
    del ws
  t, sp = stats(times)
  return {'section': 'plane', 'shape': [PLANE, PLANE], 'dtype': 'uint8', 'order': 3,
          'reps': reps, 'lines_per_pass': PLANE, 'prefilter_ms': t, 'prefilter_spread_ms': sp,
          'prefilter_Gvoxel_s': round(PLANE * PLANE / t / 1e6, 2),
          'coefficient_bytes': 8 * PLANE * PLANE}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=10)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ndwarp_spline_time.txt'))
  args = ap.parse_args()
  _abi.set_option(_spline.OPTION, 1)     # orders above 1 are opt-in
  lines = []
  for section in (section_warp, section_render, section_plane):
    lines.append(json.dumps(section(args.reps)))
    print(lines[-1], flush=True)
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
