"""Generates tests/golden/invert_map.npz from the UNMODIFIED reference
`map_utils.invert_map` (NumPy / SciPy Qhull; `_refshim` only makes
`import sofima` and `connectomics.common.bounding_box` resolve).

Build-container only.  Each case stores its coord_map (float32 or float64, as
given to the reference), the src / dst boxes (xyz start and size), the stride
(y, x) and the reference's float64 output.  Run:
  python tests/golden/make_golden_invert.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()
from connectomics.common import bounding_box  # noqa: E402
from sofima import map_utils as rmu  # noqa: E402

NAN = np.nan


def smooth_field(rng, z, h, w, amp, sigma=4.0):
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, h, w)), (0, sigma, sigma))
                for _ in range(2)])
  return f / np.abs(f).max() * amp


def rotation(h, w, stride, deg):
  t = np.deg2rad(deg)
  yy, xx = np.mgrid[:h, :w] * 1.0
  x, y = xx * stride, yy * stride
  cx, cy = x.mean(), y.mean()
  rx = cx + np.cos(t) * (x - cx) - np.sin(t) * (y - cy)
  ry = cy + np.sin(t) * (x - cx) + np.cos(t) * (y - cy)
  return np.stack([rx - x, ry - y])[:, None]


def main():
  rng = np.random.default_rng(11)
  cases = []

  def add(name, cm, src, dst, stride):
    src_b = bounding_box.BoundingBox(start=src[0], size=src[1])
    dst_b = bounding_box.BoundingBox(start=dst[0], size=dst[1])
    out = rmu.invert_map(cm.copy(), src_b, dst_b, stride)
    assert out.dtype == np.float64
    cases.append((name, cm, np.array(src, np.int64), np.array(dst, np.int64),
                  np.array(np.broadcast_to(stride, 2), np.float64), out))

  def same(h, w, z=1, start=(0, 0, 0)):
    b = (tuple(start), (w, h, z))
    return b, b

  # -- similarity maps: co-circular everywhere ---------------------------------
  cm = np.zeros((2, 1, 24, 28), np.float32)
  add('identity', cm, *same(24, 28), 40)
  cm = np.zeros((2, 1, 24, 28))
  cm[0] += 13.37
  cm[1] -= 7.25
  add('translation', cm, *same(24, 28, start=(3, 5, 0)), 40)
  add('rotation', rotation(26, 26, 40, 2.0), *same(26, 26), 40)
  cm = np.zeros((2, 1, 24, 24))
  cm[:, 0, 9, 9] = NAN
  cm[:, 0, 15:18, 4:6] = NAN
  cm[:, 0, :3, 18:] = NAN
  add('identity_holes_corner', cm, *same(24, 24), 40)
  cm = np.zeros((2, 1, 22, 22)) + 0.3
  cm[:, 0, 10:12, 10:13] = NAN
  add('translation_blob', cm, *same(22, 22), 40)

  # -- smooth deformations up to 0.6 x stride ---------------------------------
  s = 40
  add('smooth_f32', smooth_field(rng, 1, 32, 32, 0.6 * s).astype(np.float32),
      *same(32, 32), s)
  cm = smooth_field(rng, 1, 30, 30, 0.5 * s)
  for y, x in ((5, 5), (12, 20), (25, 8), (20, 21)):
    cm[:, 0, y, x] = NAN
  add('single_holes', cm, *same(30, 30), s)
  cm = smooth_field(rng, 1, 32, 32, 0.4 * s)
  noise = ndimage.gaussian_filter(rng.standard_normal((32, 32)), 1.5)
  cm[:, 0, noise > np.quantile(noise, 0.9)] = NAN
  add('blobs', cm, *same(32, 32), s)
  cm = smooth_field(rng, 1, 30, 30, 0.4 * s)
  band = ndimage.gaussian_filter(rng.standard_normal((2, 30)), (0, 3))
  yy, xx = np.mgrid[:30, :30]
  top = 3 + (band[0] / np.abs(band[0]).max() * 3).astype(int)
  left = 3 + (band[1] / np.abs(band[1]).max() * 3).astype(int)
  cm[:, 0, yy < top[None, :]] = NAN
  cm[:, 0, xx < left[:, None]] = NAN
  add('border_bands', cm, *same(30, 30), s)
  cm = smooth_field(rng, 1, 28, 28, 0.3 * s)
  yy, xx = np.mgrid[:28, :28]
  cm[:, 0, np.abs(yy - xx) <= 1] = NAN
  add('diagonal_split', cm, *same(28, 28), s)
  cm = smooth_field(rng, 1, 24, 24, 0.3 * s)
  keep = np.zeros((24, 24), bool)
  keep[:12, :12] = True
  keep[11:, 11:] = True                      # the two blocks share node (11, 11)
  cm[:, 0, ~keep] = NAN
  add('touching', cm, *same(24, 24), s)
  cm = smooth_field(rng, 1, 26, 26, 0.3 * s)
  cm[:, 0, 8:20, 8:20] = NAN
  for y, x in ((10, 12), (14, 16), (18, 9)):
    cm[:, 0, y, x] = rng.uniform(-5, 5, 2)
  add('isolated_nodes', cm, *same(26, 26), s)

  # -- boxes and strides -------------------------------------------------------
  cm = smooth_field(rng, 1, 24, 26, 0.5 * s)
  add('dst_larger', cm, ((10, 20, 0), (26, 24, 1)), ((9, 19, 0), (28, 26, 1)), s)
  add('dst_shifted', cm, ((10, 20, 0), (26, 24, 1)), ((14, 25, 0), (20, 12, 1)), s)
  cm = smooth_field(rng, 1, 24, 30, 1.0) * np.array([0.5 * 20, 0.5 * 40])[:, None, None, None]
  add('strides_40_20', cm, *same(24, 30), (40, 20))
  cm = smooth_field(rng, 1, 24, 24, 0.4 * 30)
  add('stride_non_integer', cm, *same(24, 24), (30.5, 29.25))

  # -- several slices of different validity ------------------------------------
  cm = smooth_field(rng, 5, 24, 24, 0.4 * s)
  cm[:, 1, :, :] = NAN                       # no valid node
  cm[:, 2, :, :] = NAN
  cm[:, 2, 3, 4:7] = 0.0                     # collinear: Qhull fails
  cm[:, 3, 5:9, 5:9] = NAN
  cm[:, 4, :, :6] = NAN
  add('multi_slice', cm, *same(24, 24, z=5), s)

  # the reference's 2-D KAT map
  hx = np.mgrid[:50, :50][1]
  cm = np.zeros([2, 1, 50, 50])
  cm[1, 0] = np.sin(hx / 25) * 20
  add('kat', cm, ((100, 200, 10), (50, 50, 1)), ((100, 200, 10), (50, 50, 1)), 40.0)

  arrays = {}
  for i, (name, cm, src, dst, stride, out) in enumerate(cases):
    arrays[f'{i:02d}_name'] = np.array(name)
    arrays[f'{i:02d}_map'] = cm
    arrays[f'{i:02d}_src'] = src
    arrays[f'{i:02d}_dst'] = dst
    arrays[f'{i:02d}_stride'] = stride
    arrays[f'{i:02d}_out'] = out
  path = os.path.join(HERE, 'invert_map.npz')
  np.savez_compressed(path, **arrays)
  print(f'{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
  main()
