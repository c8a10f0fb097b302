"""Generates tests/golden/compose_maps_tri.npz from the UNMODIFIED reference
`map_utils.compose_maps` (NumPy / SciPy Qhull; `_refshim` only makes
`import sofima` and `connectomics.common.bounding_box` resolve).

Build-container only.  Each case stores both maps (float32 or float64, as
given to the reference), both boxes (xyz start and size), the two strides and
the reference's output (of map1's dtype).  The maps are tiny: the tests state
the contract by brute force over all triangles of valid nodes
(tests/compose_maps_scipy.py).  Strides are exact in binary.  Generic map2
data pins the contract (the value of SOME admissible triangle); an exactly
affine map2 (coefficients multiples of 1/64) has one admissible value per
query, holes included, and pins plain parity.  Asserted here for every case
but 'map1_zero' (its queries lie on nodes and on the hull on purpose): no
query lies within 1e-7 * stride of the hull, and in the affine cases every
query in the hull has a single admissible value.  Run:
  python tests/golden/make_golden_compose.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
sys.path.insert(0, ROOT)
import refshim  # noqa: E402

refshim.install()
from connectomics.common import bounding_box  # noqa: E402
from sofima import map_utils as rmu  # noqa: E402

from tests import compose_maps_scipy as cms  # noqa: E402
from tests import resample_map_scipy as rms  # noqa: E402

NAN = np.nan


def holes_8x10(cm):
  """A block hole, a notch in the border and single holes
  (make_golden_resample.py)."""
  cm[:, :, 2:4, 3:6] = NAN
  cm[:, :, 6:, 7:9] = NAN
  cm[:, :, 5, 1] = NAN
  cm[:, :, 0, 0] = NAN
  cm[:, :, 4, 8] = NAN
  return cm


def affine_rel(shape_yx, start_xy, stride, coeffs, dtype=np.float64):
  """A relative [2, 1, y, x] map whose absolute form is exactly affine in the
  lattice position: abs = p + c0 + c1 * x + c2 * y per channel, the
  coefficients multiples of 1/64."""
  yy, xx = np.mgrid[:shape_yx[0], :shape_yx[1]]
  x = (xx + start_xy[0]) * stride
  y = (yy + start_xy[1]) * stride
  cm = np.stack([c[0] + c[1] * x + c[2] * y for c in coeffs])[:, None]
  out = cm.astype(dtype)
  assert np.array_equal(out.astype(np.float64), cm)
  return out


def check_case(name, m1, b1, s1, m2, b2, s2, out, affine):
  abs1 = cms.to_absolute(m1, s1, b1).astype(np.float64)
  abs2 = cms.to_absolute(m2, s2, b2).astype(np.float64)
  pos = cms.lattice(m2.shape[2:], b2, s2)
  for z in range(m1.shape[1]):
    valid = np.all(np.isfinite(abs2[:, z]), axis=0).ravel()
    qry = np.stack([abs1[0, z].ravel(), abs1[1, z].ravel()], 1)
    qry = qry[np.all(np.isfinite(qry), axis=1)]
    if valid.sum() < 3 or not len(qry):
      continue
    try:
      dist = np.abs(rms._hull_distance(pos[valid], qry))
    except Exception:   # collinear nodes: no hull
      continue
    assert dist.min() > 1e-7 * s2, (name, z, dist.min())
  counts = cms.check_contract(m1, b1, s1, m2, b2, s2, out, out)
  if affine:
    assert counts['in_hull'] > 0 and counts['single'] == counts['in_hull'], (name, counts)
  return counts


def main():
  rng = np.random.default_rng(23)
  cases = []

  def add(name, m1, box1, s1, m2, box2, s2, affine=False, check=True):
    b1 = bounding_box.BoundingBox(start=box1[0], size=box1[1])
    b2 = bounding_box.BoundingBox(start=box2[0], size=box2[1])
    keep1, keep2 = m1.copy(), m2.copy()
    out = rmu.compose_maps(m1, b1, s1, m2, b2, s2)
    assert out.dtype == m1.dtype and out.shape == m1.shape
    assert np.array_equal(m1, keep1, equal_nan=True) and np.array_equal(m2, keep2, equal_nan=True)
    counts = None
    if check:
      counts = check_case(name, m1, cms.box(*box1), s1, m2, cms.box(*box2), s2, out, affine)
    print(f'{name}: finite {np.isfinite(out[0]).sum()} of {out[0].size}, {dict(counts or {})}')
    cases.append((name, m1, np.array(box1, np.int64), m2, np.array(box2, np.int64),
                  np.array([s1, s2], np.float64), out))
    return out

  def field(z, h, w, dtype=np.float64, amp=3.0):
    return rng.uniform(-amp, amp, (2, z, h, w)).astype(dtype)

  same = ((3, 5, 0), (10, 8, 1))              # x 12 .. 48, y 20 .. 48 at stride 4
  co = ((0.25, 1 / 64, -3 / 64), (-1.5, 5 / 64, 2 / 64))

  # -- generic and affine map2, equal boxes --------------------------------------
  add('generic', field(1, 8, 10), same, 4, field(1, 8, 10), same, 4)
  add('generic_holes', field(1, 8, 10), same, 4, holes_8x10(field(1, 8, 10)), same, 4)
  add('affine', field(1, 8, 10), same, 4, affine_rel((8, 10), same[0], 4, co), same, 4,
      affine=True)
  add('affine_holes', field(1, 8, 10), same, 4,
      holes_8x10(affine_rel((8, 10), same[0], 4, co)), same, 4, affine=True)

  # -- dtypes ------------------------------------------------------------------
  add('generic_holes_f32', field(1, 8, 10, np.float32), same, 4,
      holes_8x10(field(1, 8, 10, np.float32)), same, 4)
  add('affine_holes_f32', field(1, 8, 10, np.float32), same, 4,
      holes_8x10(affine_rel((8, 10), same[0], 4, co, np.float32)), same, 4, affine=True)
  add('affine_holes_f32_f64', field(1, 8, 10, np.float32), same, 4,
      holes_8x10(affine_rel((8, 10), same[0], 4, co)), same, 4, affine=True)
  add('generic_holes_f64_f32', field(1, 8, 10), same, 4,
      holes_8x10(field(1, 8, 10, np.float32)), same, 4)
  # float32 at coordinates near 2000
  far = ((500, 490, 0), (10, 8, 1))
  add('affine_holes_f32_far', field(1, 8, 10, np.float32), far, 4,
      holes_8x10(affine_rel((8, 10), far[0], 4, ((0.25, 1 / 64, 0), (-1.5, 0, 1 / 64)),
                            np.float32)), far, 4, affine=True)

  # -- different boxes and strides ---------------------------------------------
  other = ((3, 5, 0), (6, 5, 1))              # stride 5: x 15 .. 40, y 25 .. 45
  add('boxes_strides', field(1, 5, 6), other, 5, holes_8x10(field(1, 8, 10)), same, 4)
  add('boxes_strides_affine', field(1, 5, 6), other, 5,
      holes_8x10(affine_rel((8, 10), same[0], 4, co)), same, 4, affine=True)
  fine = ((26, 42, 0), (12, 9, 1))            # stride 0.5: x 13 .. 18.5, y 21 .. 25
  add('fine_queries', field(1, 9, 12, amp=0.2), fine, 0.5, holes_8x10(field(1, 8, 10)), same, 4)

  # -- invalid entries -----------------------------------------------------------
  m1 = field(1, 8, 10)
  m1[0, 0, 3, 4] = NAN
  m1[1, 0, 5, 6] = np.inf
  m1[0, 0, 1, 2] = -np.inf
  m1[:, 0, 6, 3] = NAN
  add('map1_nan_inf', m1, same, 4, holes_8x10(field(1, 8, 10)), same, 4)
  m2 = field(1, 8, 10)
  m2[1, 0, 3, 3:5] = NAN                      # channel 1 only
  m2[1, 0, 6, 8] = NAN
  m2[0, 0, 1, 1] = np.inf                     # channel 0 only
  add('map2_nan_channel1', field(1, 8, 10), same, 4, m2, same, 4)

  # -- queries on nodes and on the hull; a query inside an interior hole --------
  add('map1_zero', np.zeros((2, 1, 8, 10)), same, 4, holes_8x10(field(1, 8, 10)), same, 4,
      check=False)
  m1 = np.zeros((2, 1, 8, 10))
  m1[0] = 0.5
  m1[1] = 0.25
  out = add('hole_query', m1, same, 4, holes_8x10(field(1, 8, 10)), same, 4)
  assert np.isfinite(out[:, 0, 2:4, 3:5]).all()   # nodes of the block hole, shifted into it

  # -- smallest shapes -----------------------------------------------------------
  quad = ((0, 0, 0), (2, 2, 1))               # stride 4: the square 0 .. 4
  inner = ((1, 1, 0), (3, 3, 1))              # stride 1: 1 .. 3
  add('one_quad', field(1, 3, 3, amp=0.4), inner, 1, field(1, 2, 2), quad, 4)
  m2 = field(1, 2, 2)
  m2[:, 0, 1, 1] = NAN
  add('three_corners', field(1, 3, 3, amp=0.4), inner, 1, m2, quad, 4)
  m2 = field(1, 3, 4)
  m2[:] = NAN
  m2[:, 0, 0, 1] = m2[:, 0, 2, 3] = 1.0
  add('two_valid', field(1, 3, 3), ((0, 0, 0), (3, 3, 1)), 4, m2, ((0, 0, 0), (4, 3, 1)), 4)
  m2 = field(1, 3, 4)
  m2[:] = NAN
  m2[:, 0, 1, :] = 0.5
  add('collinear', field(1, 3, 3), ((0, 0, 0), (3, 3, 1)), 4, m2, ((0, 0, 0), (4, 3, 1)), 4)

  # -- several slices of different validity -------------------------------------
  m2 = field(6, 6, 7)
  m2[:, 1] = NAN                              # no valid node
  m2[:, 2] = NAN
  m2[:, 2, 3, 2:5] = 1.0                      # collinear: Qhull fails
  m2[:, 3] = NAN
  m2[:, 3, 1, 1] = m2[:, 3, 4, 5] = 2.0       # two valid nodes
  m2[:, 4, 2:4, 2:5] = NAN
  m2[:, 5, :, :3] = NAN
  m1 = field(6, 6, 7)
  m1[:, 0, 2, 2] = NAN
  multi = ((2, 1, 0), (7, 6, 6))
  add('multi_slice', m1, multi, 4, m2, multi, 4)

  arrays = {}
  for i, (name, m1, b1, m2, b2, strides, out) in enumerate(cases):
    arrays[f'{i:02d}_name'] = np.array(name)
    arrays[f'{i:02d}_map1'] = m1
    arrays[f'{i:02d}_box1'] = b1
    arrays[f'{i:02d}_map2'] = m2
    arrays[f'{i:02d}_box2'] = b2
    arrays[f'{i:02d}_strides'] = strides
    arrays[f'{i:02d}_out'] = out
  path = os.path.join(HERE, 'compose_maps_tri.npz')
  np.savez_compressed(path, **arrays)
  print(f'{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
  main()
