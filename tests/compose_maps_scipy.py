"""SciPy statement of map_utils.compose_maps and its contract.

`compose_restated` is SciPy exactly as the reference calls it: both maps are
made absolute in their own dtype, per z slice the nodes of map2 where both
channels are finite, at `(index + start) * stride2`, go through Qhull
(`spatial.Delaunay`) and `LinearNDInterpolator` over the absolute map2, asked
at the finite nodes of the absolute map1; the result is assigned into an array
of map1's dtype and made relative in it.

The points are a lattice, so the contract is that of `resample_map`
(tests/resample_map_scipy.py): `check_contract` asserts, by brute force over
all triangles of valid nodes, that a result is the interpolant of an admissible
triangle at every query, equals the reference wherever all of them agree, and
is NaN exactly where the reference is.  `bd_cells` states the device's own
triangulation where it is documented: a full cell is split from (i, j + 1) to
(i + 1, j).
"""
import collections

import numpy as np

from tests import resample_map_scipy as rms

Box = rms.Box
box = rms.box


def _offsets(shape_yx, stride, b):
  """(x offsets, y offsets) [y, x] float64 as to_absolute / to_relative form
  them: index * stride + start * stride."""
  yy, xx = np.mgrid[:shape_yx[0], :shape_yx[1]]
  return xx * stride + b.start[0] * stride, yy * stride + b.start[1] * stride


def to_absolute(m, stride, b):
  out = np.array(m, copy=True)
  ox, oy = _offsets(m.shape[2:], stride, b)
  out[0] += ox
  out[1] += oy
  return out


def to_relative(m, stride, b):
  out = np.array(m, copy=True)
  ox, oy = _offsets(m.shape[2:], stride, b)
  out[0] -= ox
  out[1] -= oy
  return out


def lattice(shape_yx, b, stride):
  """Positions [h * w, 2] (x, y) float64: the integer sum, then one product."""
  yy, xx = np.mgrid[b.start[1]:b.start[1] + shape_yx[0], b.start[0]:b.start[0] + shape_yx[1]]
  return np.stack([(xx * stride).ravel(), (yy * stride).ravel()], 1).astype(np.float64)


def compose_restated(map1, box1, stride1, map2, box2, stride2):
  from scipy import interpolate, spatial
  map1, map2 = np.asarray(map1), np.asarray(map2)
  assert map1.shape[0] == 2 and map2.shape[0] == 2
  abs1 = to_absolute(map1, stride1, box1)
  abs2 = to_absolute(map2, stride2, box2)
  pos = lattice(map2.shape[2:], box2, stride2)
  ret = np.full_like(map1, np.nan)
  for z in range(map1.shape[1]):
    valid = np.all(np.isfinite(abs1[:, z]), axis=0)
    if not valid.any():
      continue
    valid_src = np.all(np.isfinite(abs2[:, z]), axis=0).ravel()
    if not valid_src.any():
      continue
    try:
      tri = spatial.Delaunay(np.ascontiguousarray(pos[valid_src], dtype=np.double))
    except spatial.QhullError:
      continue
    values = np.array([abs2[0, z].ravel()[valid_src], abs2[1, z].ravel()[valid_src]]).T
    ip = interpolate.LinearNDInterpolator(tri, values, fill_value=np.nan)
    r = ip((abs1[0, z][valid], abs1[1, z][valid])).T
    ret[0, z][valid] = r[0]
    ret[1, z][valid] = r[1]
  return to_relative(ret, stride1, box1)


def tolerance(map1, box1, stride1, map2, box2, stride2):
  """1e-6 for float64 maps; for a float32 map1 plus two float32 spacings at the
  largest absolute coordinate of the case: the interpolant is rounded once to
  float32 at that magnitude, where the two sides may land on neighbouring
  values, and once more after the subtraction."""
  map1, map2 = np.asarray(map1), np.asarray(map2)
  if map1.dtype == np.float64:
    return 1e-6
  big = 0.0
  for m, s, b in ((map1, stride1, box1), (map2, stride2, box2)):
    a = to_absolute(m.astype(np.float64), s, b)
    a = a[np.isfinite(a)]
    if a.size:
      big = max(big, float(np.abs(a).max()))
  return 1e-6 + 2 * float(np.spacing(np.float32(big)))


def check_contract(map1, box1, stride1, map2, box2, stride2, got, want, tol=None,
                   same_mask=True):
  """Asserts the contract of `got` against the reference's `want` (both
  relative, of map1's shape) for tiny maps; returns a Counter of 'queries'
  (finite nodes of abs_map1), 'in_hull' of them and 'single' with one
  admissible value.  With `same_mask` the NaN masks must be equal."""
  map1, map2 = np.asarray(map1), np.asarray(map2)
  got, want = np.asarray(got), np.asarray(want)
  assert got.shape == want.shape == map1.shape, (got.shape, want.shape, map1.shape)
  if tol is None:
    tol = tolerance(map1, box1, stride1, map2, box2, stride2)
  abs1 = to_absolute(map1, stride1, box1).astype(np.float64)
  abs2 = to_absolute(map2, stride2, box2).astype(np.float64)
  pos = lattice(map2.shape[2:], box2, stride2)
  ox, oy = _offsets(map1.shape[2:], stride1, box1)
  off = np.stack([ox.ravel(), oy.ravel()], 1).astype(np.float64)
  counts = collections.Counter()
  gn, wn = np.isnan(got), np.isnan(want)
  if same_mask:
    assert np.array_equal(gn, wn), f'NaN masks differ at {int((gn != wn).sum())} entries'
  for z in range(map1.shape[1]):
    if not same_mask and (gn[:, z] != wn[:, z]).any():
      # queries on the hull itself: closed on the device, Qhull's eps in SciPy
      z2 = z if map2.shape[1] > 1 else 0
      valid = np.all(np.isfinite(abs2[:, z2]), axis=0).ravel()
      k = np.flatnonzero((gn[:, z] != wn[:, z]).any(axis=0).ravel())
      q = np.stack([abs1[0, z].ravel()[k], abs1[1, z].ravel()[k]], 1)
      dist = np.abs(rms._hull_distance(pos[valid], q))
      assert dist.max() <= 1e-7 * stride2, (
          f'slice {z}: NaN masks differ at {k.size} queries, up to {dist.max()} from the hull')
      counts['hull_exception'] += int(k.size)
    z2 = z if map2.shape[1] > 1 else 0
    valid = np.all(np.isfinite(abs2[:, z2]), axis=0).ravel()
    values = np.stack([abs2[0, z2].ravel(), abs2[1, z2].ravel()], 1)
    qry = np.stack([abs1[0, z].ravel(), abs1[1, z].ravel()], 1)
    ok = np.all(np.isfinite(qry), axis=1)
    idx = np.flatnonzero(ok)
    adm = rms.admissible_values(valid, values, pos, qry[idx])
    g = got[:, z].reshape(2, -1).T.astype(np.float64)
    w = want[:, z].reshape(2, -1).T.astype(np.float64)
    bad = np.flatnonzero(~ok)
    assert np.isnan(g[bad]).all(), f'slice {z}: a value at a query that is not finite'
    for a, k in zip(adm, idx):
      counts['queries'] += 1
      if np.isnan(g[k]).any() or np.isnan(w[k]).any():
        assert len(a) == 0 or np.isnan(g[k]).all() != np.isnan(w[k]).all(), (
            f'slice {z}, query {k} at {qry[k]}: NaN inside the hull')
        continue
      counts['in_hull'] += 1
      assert len(a), f'slice {z}, query {k} at {qry[k]}: a value outside the hull'
      rel = a - off[k]
      for name, val in (('result', g[k]), ('reference', w[k])):
        err = np.max(np.abs(rel - val), axis=1)
        assert err.min() <= tol, (
            f'slice {z}, query {k} at {qry[k]}: {name} {val} is no admissible value, '
            f'nearest misses by {err.min()} (tol {tol})')
      if np.max(np.ptp(a, axis=0)) <= rms.AGREE:
        counts['single'] += 1
        assert np.max(np.abs(g[k] - w[k])) <= tol, (
            f'slice {z}, query {k}: {g[k]} against the reference {w[k]} where all '
            f'Delaunay triangulations agree')
  return counts


def bd_cells(map1, box1, stride1, map2, box2, stride2):
  """The documented triangulation where it is stated: (values, mask), values
  [2, z, y, x] float64 relative, mask [z, y, x] the queries whose cell of map2
  (floor(q / stride2) - start) has four valid corners.  The cell (a b / d c:
  a = (i, j), b = (i, j + 1), c = (i + 1, j + 1), d = (i + 1, j)) is split
  from b to d; on the shared edges both halves give one value."""
  map1, map2 = np.asarray(map1), np.asarray(map2)
  abs1 = to_absolute(map1, stride1, box1).astype(np.float64)
  abs2 = to_absolute(map2, stride2, box2).astype(np.float64)
  h, w = map2.shape[2:]
  ox, oy = _offsets(map1.shape[2:], stride1, box1)
  out = np.full(map1.shape, np.nan)
  mask = np.zeros(map1.shape[1:], bool)
  for z in range(map1.shape[1]):
    z2 = z if map2.shape[1] > 1 else 0
    valid = np.all(np.isfinite(abs2[:, z2]), axis=0)
    qx, qy = abs1[0, z], abs1[1, z]
    ok = np.isfinite(qx) & np.isfinite(qy)
    with np.errstate(invalid='ignore'):
      cj = np.where(ok, np.floor(qx / stride2) - box2.start[0], -1)
      ci = np.where(ok, np.floor(qy / stride2) - box2.start[1], -1)
    ok &= (cj >= 0) & (cj < w - 1) & (ci >= 0) & (ci < h - 1)
    cj = np.where(ok, cj, 0).astype(int)
    ci = np.where(ok, ci, 0).astype(int)
    ok &= valid[ci, cj] & valid[ci, cj + 1] & valid[ci + 1, cj] & valid[ci + 1, cj + 1]
    fx = qx / stride2 - (cj + box2.start[0])
    fy = qy / stride2 - (ci + box2.start[1])
    for c in range(2):
      v = abs2[c, z2]
      a, b, cc, d = v[ci, cj], v[ci, cj + 1], v[ci + 1, cj + 1], v[ci + 1, cj]
      lower = a + fx * (b - a) + fy * (d - a)
      upper = cc + (1 - fx) * (d - cc) + (1 - fy) * (b - cc)
      val = np.where(fx + fy <= 1, lower, upper)
      out[c, z] = np.where(ok, val - (ox, oy)[c], np.nan)
    mask[z] = ok
  return out, mask
