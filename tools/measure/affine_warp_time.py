"""Device time of an affine resample by three routes: the fused `warp.affine_transform`,
the coordinate-map route that existed before it, and that route on resident data.

One 512 x 512 x 128 uint8 volume (z, y, x = 128, 512, 512), a rotation with shear and
anisotropic scale about a point near the centre, at order 1 and order 3:

  fused   warp.affine_transform: one launch of sfm_affine_warp, which forms the source
          coordinates from the matrix and reads no map
  map     map_utils.make_affine_map at stride 1 (a [3, z, y, x] float64 map, 24 bytes per
          voxel) and warp.ndimage_warp of it, which is `implementation='sofima'` of
          decorators_warp.warp_affine with NumPy in and out: the launches of
          sfm_affine_map and of sfm_ndimage_warp_rel (the map is downloaded and
          uploaded again, relative and in its own dtype)
  map_device  the same two functions on resident data: the DeviceArray of
          make_affine_map goes straight to ndimage_warp, with the image a CUDA tensor
          and device_output=True; nothing crosses to the host

Per route two figures.  `kernels_ms`: the launches named above, by HIP events
(torch.cuda.Event) recorded around them inside the call; for `map` the sum of its two
launches.  The order-3 prefilter is the same work on both routes and is reported on its
own.  `call_ms`: the whole call as a caller sees it, wall clock with a synchronisation at
the end: NumPy in and NumPy out for `fused` and `map` (the map route moves the map to the
host and back), resident in and out for `map_device`.  2 warm-up calls, `--reps` timed
ones, the routes and orders alternating in one process; the median and the spread
(max - min) are reported.  The routes must agree: make_affine_map is a few ulp off the
fused coordinates (map_utils), so the share of differing voxels is reported and asserted
to be below 1e-3; `map_device` must equal `map` voxel for voxel.
profiles/affine_warp_time.txt is rewritten: its first two lines, the record from before
ndimage_warp read relative maps (when `map` prepared a float64 absolute map on the host,
and there was no `map_device`), are kept as a fixed header, and one JSON line per order
of this run follows them, so the file always has four lines.

  python tools/measure/affine_warp_time.py [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sofima_amd import _abi, _spline, map_utils, warp  # noqa: E402

VOLUME = (128, 512, 512)      # z, y, x


class Events:
  """HIP events around the named library calls (and _spline.prefilter) of a call."""

  NAMES = ('sfm_affine_warp', 'sfm_affine_map', 'sfm_ndimage_warp_rel')

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
    self._saved = {name: getattr(self._lib, name) for name in self.NAMES}
    self._prefilter = _spline.prefilter
    for name, fn in self._saved.items():
      setattr(self._lib, name, self._wrap(name, fn))
    _spline.prefilter = self._wrap('prefilter', self._prefilter)
    return self

  def __exit__(self, *exc):
    for name, fn in self._saved.items():
      setattr(self._lib, name, fn)
    _spline.prefilter = self._prefilter
    return False

  def take(self):
    """{name: ms} of the calls since the last take."""
    torch.cuda.synchronize()
    out = {}
    for name, t0, t1 in self._pending:
      out[name] = out.get(name, 0.0) + t0.elapsed_time(t1)
    self._pending = []
    return out


def stats(ts):
  return round(float(np.median(ts)), 3), round(float(max(ts) - min(ts)), 3)


def inverse_matrix():
  """[3, 4] zyx matrix of scipy.ndimage.affine_transform: a turn of 0.05 rad in the yx
  plane, a little shear and scale, about the volume's centre."""
  a = 0.05
  m = np.eye(3)
  m[1:, 1:] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
  m = m @ np.diag([1.02, 0.98, 1.01])
  m[0, 2] += 0.01
  centre = (np.array(VOLUME) - 1) / 2.0
  return np.concatenate([m, (centre - m @ centre)[:, None]], axis=1)


def fused(img, m_zyx, order):
  return warp.affine_transform(img, m_zyx, order=order)


def affine_map(shape, m_zyx):
  # make_affine_map takes xyz rows and columns; the map's channels are x, y, z
  m_xyz = np.concatenate([m_zyx[::-1, :3][:, ::-1], m_zyx[::-1, 3:]], axis=1)
  box = types.SimpleNamespace(start=np.zeros(3, np.int64), size=np.array(shape[::-1]))
  return map_utils.make_affine_map(m_xyz, box, [1, 1, 1])


def by_map(img, m_zyx, order):
  cmap = affine_map(img.shape, m_zyx)
  return warp.ndimage_warp(img, np.asarray(cmap), [1, 1, 1], img.shape[::-1], [0, 0, 0],
                           order=order)


def by_map_device(img_t, m_zyx, order):
  shape = tuple(img_t.shape)
  return warp.ndimage_warp(img_t, affine_map(shape, m_zyx), [1, 1, 1], shape[::-1], [0, 0, 0],
                           order=order, device_output=True)


def wall(fn):
  torch.cuda.synchronize()
  t = time.perf_counter()
  out = fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t) * 1e3, out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'affine_warp_time.txt'))
  args = ap.parse_args()
  _abi.set_option(_spline.OPTION, 1)     # orders above 1 are opt-in
  rng = np.random.default_rng(0)
  img = rng.integers(0, 256, VOLUME).astype(np.uint8)
  m = inverse_matrix()
  img_t = torch.from_numpy(img).to('cuda')      # the resident image of map_device
  routes = {'fused': fused, 'map': by_map, 'map_device': by_map_device}
  kernels = {'fused': ('sfm_affine_warp',),
             'map': ('sfm_affine_map', 'sfm_ndimage_warp_rel'),
             'map_device': ('sfm_affine_map', 'sfm_ndimage_warp_rel')}

  differ = {}
  for order in (1, 3, 1, 3):             # (two warm-up calls of either route and order)
    a, b = fused(img, m, order), by_map(img, m, order)
    differ[order] = float(np.mean(a != b))
    assert np.mean(a != 0) > 0.9 and differ[order] < 1e-3, differ
    assert np.array_equal(np.asarray(by_map_device(img_t, m, order)), b)
  del a, b

  times = {(r, o): {'call': [], 'kernels': [], 'prefilter': []} for r in routes for o in (1, 3)}
  with Events() as ev:
    for _ in range(args.reps):
      for order in (1, 3):
        for name, fn in routes.items():
          ms, _ = wall(lambda: fn(img_t if name == 'map_device' else img, m, order))
          parts = ev.take()
          rec = times[name, order]
          rec['call'].append(ms)
          rec['kernels'].append(sum(parts.get(k, 0.0) for k in kernels[name]))
          rec['prefilter'].append(parts.get('prefilter', 0.0))
  voxels = int(np.prod(VOLUME))
  lines = []
  for order in (1, 3):
    line = {'volume': list(VOLUME), 'dtype': 'uint8', 'order': order, 'reps': args.reps,
            'map_bytes': 24 * voxels, 'voxels_differing': differ[order]}
    for name in routes:
      rec = times[name, order]
      for key in ('kernels', 'prefilter', 'call'):
        if key == 'prefilter' and order == 1:
          continue
        line[f'{name}_{key}_ms'], line[f'{name}_{key}_spread_ms'] = stats(rec[key])
    line['map_over_fused_kernels'] = round(line['map_kernels_ms'] / line['fused_kernels_ms'], 2)
    line['map_over_map_device_call'] = round(line['map_call_ms'] / line['map_device_call_ms'], 1)
    line['fused_Gvoxel_s'] = round(voxels / line['fused_kernels_ms'] / 1e6, 2)
    lines.append(json.dumps(line))
    print(lines[-1], flush=True)
  header = []      # the two lines of the earlier record: those without a map_device route
  if os.path.exists(args.out):
    with open(args.out) as f:
      header = [ln.strip() for ln in f if ln.strip() and 'map_device_call_ms' not in ln][:2]
  lines = header + lines
  with open(args.out, 'w') as f:
    f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
