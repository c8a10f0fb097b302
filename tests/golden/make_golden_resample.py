"""Generates tests/golden/resample_map.npz from the UNMODIFIED reference
`map_utils.resample_map` (NumPy / SciPy Qhull; `_refshim` only makes
`import sofima` and `connectomics.common.bounding_box` resolve).

Build-container only.  Each case stores its coord_map (float32 or float64, as
given to the reference), the src / dst boxes (xyz start and size), the two
strides and the reference's output (of the map's dtype).  The maps are tiny:
the tests state the contract by brute force over all triangles of valid nodes
(tests/resample_map_scipy.py).  Strides are exact in binary (1, 2, 0.5, 2.5,
3), so no query lies on the hull to rounding only.  Run:
  python tests/golden/make_golden_resample.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()
from connectomics.common import bounding_box  # noqa: E402
from sofima import map_utils as rmu  # noqa: E402

NAN = np.nan


def holes_8x10(cm):
  """A block hole, a notch in the border and single holes."""
  cm[:, :, 2:4, 3:6] = NAN
  cm[:, :, 6:, 7:9] = NAN
  cm[:, :, 5, 1] = NAN
  cm[:, :, 0, 0] = NAN
  cm[:, :, 4, 8] = NAN
  return cm


def main():
  rng = np.random.default_rng(17)
  cases = []

  def add(name, cm, src, dst, src_stride, dst_stride):
    src_b = bounding_box.BoundingBox(start=src[0], size=src[1])
    dst_b = bounding_box.BoundingBox(start=dst[0], size=dst[1])
    out = rmu.resample_map(cm.copy(), src_b, dst_b, src_stride, dst_stride)
    assert out.dtype == cm.dtype
    cases.append((name, cm, np.array(src, np.int64), np.array(dst, np.int64),
                  np.array([src_stride, dst_stride], np.float64), out))

  def field(z, h, w, dtype=np.float64):
    return rng.uniform(-3, 3, (2, z, h, w)).astype(dtype)

  # -- 2 x upsampling onto a larger dst box ------------------------------------
  src = ((3, 5, 0), (10, 8, 1))
  up2 = ((4, 8, 0), (23, 19, 1))             # src spans x 6 .. 24, y 10 .. 24 at stride 2
  add('up2_full', field(1, 8, 10), src, up2, 2, 1)
  add('up2_holes', holes_8x10(field(1, 8, 10)), src, up2, 2, 1)
  add('up2_holes_f32', holes_8x10(field(1, 8, 10, np.float32)), src, up2, 1, 0.5)
  yy, xx = np.mgrid[:8, :10]
  cm = np.stack([0.25 + 0.5 * xx - 0.125 * yy, -1.5 + 0.0625 * xx + 0.75 * yy])[:, None]
  add('affine_holes', holes_8x10(cm.copy()), ((-7, -4, 0), (10, 8, 1)),
      ((-16, -10, 0), (23, 19, 1)), 2, 1)

  # -- other directions --------------------------------------------------------
  add('down2', field(1, 9, 9), ((0, 0, 0), (9, 9, 1)), ((0, 0, 0), (5, 5, 1)), 1, 2)
  # src x 3 .. 21, y -3 .. 12; queries at odd multiples of 2 offsets: inside cells
  add('stride_3_to_2', holes_8x10(field(1, 8, 10))[:, :, :6, :7],
      ((1, -1, 0), (7, 6, 1)), ((1, -1, 0), (11, 8, 1)), 3, 2)
  add('stride_2p5_to_1', field(1, 5, 6), ((1, 3, 0), (6, 5, 1)), ((3, 7, 0), (12, 11, 1)),
      2.5, 1)
  add('dst_smaller', holes_8x10(field(1, 8, 10)), src, ((9, 13, 0), (7, 5, 1)), 2, 1)
  add('dst_disjoint', field(1, 4, 4), ((0, 0, 0), (4, 4, 1)), ((20, 20, 0), (3, 3, 1)), 2, 1)

  # -- smallest shapes ---------------------------------------------------------
  add('one_quad', field(1, 2, 2), ((0, 0, 0), (2, 2, 1)), ((0, 0, 0), (3, 3, 1)), 2, 1)
  cm = field(1, 2, 2)
  cm[:, 0, 1, 1] = NAN
  add('three_corners', cm, ((0, 0, 0), (2, 2, 1)), ((0, 0, 0), (5, 5, 1)), 2, 0.5)

  # -- several slices of different validity ------------------------------------
  cm = field(6, 6, 7)
  cm[:, 1] = NAN                              # no valid node
  cm[:, 2] = NAN
  cm[:, 2, 3, 2:5] = 1.0                      # collinear: Qhull fails
  cm[:, 3] = NAN
  cm[:, 3, 1, 1] = cm[:, 3, 4, 5] = 2.0       # two valid nodes
  cm[:, 4, 2:4, 2:5] = NAN
  cm[:, 5, :, :3] = NAN
  add('multi_slice', cm, ((2, 1, 0), (7, 6, 6)), ((3, 1, 0), (14, 12, 6)), 2, 1)

  arrays = {}
  for i, (name, cm, src, dst, strides, out) in enumerate(cases):
    arrays[f'{i:02d}_name'] = np.array(name)
    arrays[f'{i:02d}_map'] = cm
    arrays[f'{i:02d}_src'] = src
    arrays[f'{i:02d}_dst'] = dst
    arrays[f'{i:02d}_strides'] = strides
    arrays[f'{i:02d}_out'] = out
  path = os.path.join(HERE, 'resample_map.npz')
  np.savez_compressed(path, **arrays)
  print(f'{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
  main()
