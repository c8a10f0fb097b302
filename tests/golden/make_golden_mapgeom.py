"""Generates tests/golden/mapgeom.npz from the UNMODIFIED reference
`map_utils.to_absolute / to_relative / outer_box / inner_box / make_affine_map`
and `warp.warp_points` (NumPy / SciPy; `_refshim` only makes `import sofima` and
`connectomics.common.bounding_box` resolve).

Build-container only.  Inputs and outputs only:
  geoNN_*  a map, its box (xyz start and size; start all zero and `hasbox` 0 for
           the calls without a box), stride ([z]yx), target_len ([z]yx), and the
           reference's to_absolute, to_relative (of that absolute map),
           outer_box (start, size; `outer_err` 1 when it raised ValueError) and,
           for NaN-free maps, inner_box (start, size as the reference builds
           them, float arrays)
  affNN_*  matrix, box, stride (zyx) and the reference's map
  ptsNN_*  points, map, box, stride and the warped points
Run:
  python tests/golden/make_golden_mapgeom.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()
from connectomics.common import bounding_box  # noqa: E402
from sofima import map_utils as rmu  # noqa: E402
from sofima import warp as rwarp  # noqa: E402

NAN = np.nan


def bb(start, size):
  return bounding_box.BoundingBox(start=start, size=size)


def main():
  rng = np.random.default_rng(23)
  arrays = {}

  # -- to_absolute / to_relative / outer_box / inner_box -------------------------
  geo = []

  def add_geo(name, cm, stride, start=None, target_len=None):
    dim = cm.shape[0]
    size = cm.shape[1:][::-1]
    box = bb(start, size) if start is not None else None
    ab = rmu.to_absolute(cm.copy(), stride, box)
    rel = rmu.to_relative(ab.copy(), stride, box)
    assert ab.dtype == cm.dtype and rel.dtype == cm.dtype
    rec = dict(name=np.array(name), map=cm, hasbox=np.array(int(start is not None)),
               start=np.array(start if start is not None else (0, 0, 0), np.int64),
               size=np.array(size, np.int64),
               stride=np.array(np.broadcast_to(stride, dim), np.float64),
               target_len=np.array(np.broadcast_to(
                   target_len if target_len is not None else stride, dim), np.float64),
               abs=ab, rel=rel)
    if box is not None:
      # integer strides stay Python ints for the box arithmetic, like a caller's
      tl = target_len
      try:
        with warnings.catch_warnings():
          warnings.simplefilter('ignore')
          ob = rmu.outer_box(cm.copy(), box, stride, tl)
        rec.update(outer_err=np.array(0), outer_start=np.array(ob.start),
                   outer_size=np.array(ob.size))
      except ValueError:
        rec.update(outer_err=np.array(1))
      if not np.isnan(cm).any():
        ib = rmu.inner_box(cm.copy(), box, stride)
        rec.update(inner_start=np.array(ib.start, np.float64),
                   inner_size=np.array(ib.size, np.float64))
    geo.append(rec)

  def field(dim, z, y, x, amp, dtype):
    return (rng.uniform(-amp, amp, (dim, z, y, x))).astype(dtype)

  add_geo('c2_f32_scalar', field(2, 3, 5, 7, 25.0, np.float32), 40, (3, -5, 2))
  add_geo('c2_f32_nobox', field(2, 3, 5, 7, 25.0, np.float32), 40)
  add_geo('c2_f64_peraxis_neg', field(2, 2, 6, 9, 12.0, np.float64), (20.5, 40), (-11, -4, 7))
  add_geo('c2_f64_target_len', field(2, 2, 6, 9, 300.0, np.float64), (20, 40), (5, 6, 0),
          target_len=(16, 8))
  add_geo('c3_f32_peraxis', field(3, 4, 5, 6, 9.0, np.float32), (30, 20, 10), (-7, 11, 2))
  add_geo('c3_f64_scalar', field(3, 4, 5, 6, 6.0, np.float64), 12.5, (2, 3, -4))
  add_geo('c3_f32_nobox', field(3, 4, 5, 6, 9.0, np.float32), (30, 20, 10))
  add_geo('c3_f32_target_len', field(3, 3, 4, 5, 50.0, np.float32), (30, 20, 10), (1, 2, 3),
          target_len=7)
  add_geo('c2_single_node', field(2, 1, 1, 1, 5.0, np.float32), 40, (9, -9, 1))
  add_geo('c2_f32_large_coords', field(2, 1, 4, 5, 0.4, np.float32), 40,
          (400001, -300007, 0))      # float32 rounding of the sum is visible
  cm = field(2, 2, 8, 9, 30.0, np.float32)
  cm[:, 0, 2:4, 3:6] = NAN
  cm[:, 1, 0, :] = NAN
  cm[0, 1, 5, 5] = NAN               # one channel only
  add_geo('c2_f32_holes', cm, 40, (-3, 4, 0))
  cm = field(3, 3, 4, 5, 8.0, np.float64)
  cm[:, 1, 1:3, 2:4] = NAN
  add_geo('c3_f64_holes', cm, (10, 20, 30), (1, -2, 3))
  cm = field(2, 2, 4, 5, 8.0, np.float32)
  cm[1] = NAN
  add_geo('c2_f32_all_nan_channel', cm, 40, (0, 0, 0))
  for i, rec in enumerate(geo):
    for k, v in rec.items():
      arrays[f'geo{i:02d}_{k}'] = v

  # -- make_affine_map -----------------------------------------------------------
  aff = []

  def add_aff(name, matrix, start, size, stride):
    out = rmu.make_affine_map(np.array(matrix, np.float64), bb(start, size), stride)
    assert out.dtype == np.float64
    aff.append(dict(name=np.array(name), matrix=np.array(matrix, np.float64),
                    start=np.array(start, np.int64), size=np.array(size, np.int64),
                    stride=np.array(np.broadcast_to(stride, 3), np.float64), out=out))

  eye = np.hstack([np.eye(3), np.zeros((3, 1))])
  add_aff('identity', eye, (0, 0, 0), (6, 5, 4), 10)
  tr = eye.copy()
  tr[:, 3] = (3.25, -7.5, 11.0)
  add_aff('translation', tr, (4, -3, 2), (7, 3, 2), (4, 8, 16))
  gen = rng.uniform(-1.5, 1.5, (3, 4))
  gen[:, 3] *= 40
  add_aff('general', gen, (-13, 21, 5), (5, 6, 3), (2.5, 20, 40))
  add_aff('general_single_node', gen, (3, 2, 1), (1, 1, 1), 7)
  for i, rec in enumerate(aff):
    for k, v in rec.items():
      arrays[f'aff{i:02d}_{k}'] = v

  # -- warp_points -----------------------------------------------------------------
  pts = []

  def add_pts(name, points, cm, start, stride):
    box = bb(start, cm.shape[1:][::-1])
    with warnings.catch_warnings():
      warnings.simplefilter('ignore')
      out = rwarp.warp_points(points.copy(), cm.copy(), box, stride)
    assert out.dtype == points.dtype
    pts.append(dict(name=np.array(name), points=points, map=cm,
                    start=np.array(start, np.int64), stride=np.array(float(stride)), out=out))

  def cloud(n, cm, start, stride, dtype, zs):
    """Points inside the grid, outside on every side, on nodes and on the last node."""
    nz, ny, nx = cm.shape[1:]
    x0, y0 = start[0] * stride, start[1] * stride
    w, h = (nx - 1) * stride, (ny - 1) * stride
    xy = rng.uniform([x0 - 0.7 * stride, y0 - 0.7 * stride],
                     [x0 + w + 0.7 * stride, y0 + h + 0.7 * stride], (n, 2))
    on = rng.integers(0, [nx, ny], (n // 4, 2)) * stride + [x0, y0]
    xy[:n // 4] = on
    xy[n // 4] = (x0 + w, y0 + h)                       # the last node
    xy[n // 4 + 1] = (x0 - 2.5 * stride, y0 + h + 3.25 * stride)
    z = rng.choice(zs, n)
    p = np.concatenate([xy, z[:, None]], axis=1)
    return (np.round(p) if np.issubdtype(dtype, np.integer) else p).astype(dtype)

  m32 = field(2, 3, 6, 7, 15.0, np.float32)
  m64 = field(2, 3, 6, 7, 15.0, np.float64)
  start = (5, -3, 10)
  zs = (10, 11, 12, 9, 8)            # 9, 8: sections -1, -2 wrap
  for dt in (np.float32, np.float64, np.int32, np.int64):
    add_pts(f'm32_{np.dtype(dt).name}', cloud(160, m32, start, 40, dt, zs), m32, start, 40)
    add_pts(f'm64_{np.dtype(dt).name}', cloud(160, m64, start, 40, dt, zs), m64, start, 40)
  m = field(2, 1, 2, 2, 4.0, np.float32)
  add_pts('map_2x2', cloud(64, m, (0, 0, 0), 20.5, np.float64, (0,)), m, (0, 0, 0), 20.5)
  m = field(2, 2, 2, 9, 4.0, np.float64)
  add_pts('map_2x9', cloud(65, m, (-4, 2, -1), 32, np.float32, (-1, 0, -2)), m, (-4, 2, -1), 32)
  m = m32.copy()
  m[:, 0, 2:4, 2:5] = NAN
  m[0, 1, 0, 0] = NAN
  add_pts('nan_nodes_f32', cloud(120, m, start, 40, np.float32, zs), m, start, 40)
  add_pts('nan_nodes_f64', cloud(120, m.astype(np.float64), start, 40, np.float64, zs),
          m.astype(np.float64), start, 40)
  add_pts('far_f32_points', (cloud(100, m32, (40001, 70003, 10), 40, np.float64, zs)
                             ).astype(np.float32), m32, (40001, 70003, 10), 40)
  for i, rec in enumerate(pts):
    for k, v in rec.items():
      arrays[f'pts{i:02d}_{k}'] = v

  path = os.path.join(HERE, 'mapgeom.npz')
  np.savez_compressed(path, **arrays)
  print(f'{len(geo)} + {len(aff)} + {len(pts)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
  main()
