"""SciPy statement of map_utils.invert_map (2-D) and its parity contract.

`invert_restated` is written from the contract (absolute positions in
to_absolute's float64 order, source coordinates and queries in integer
arrays, Delaunay + LinearNDInterpolator per z slice, made relative).
`check_contract` compares a device result with a host result: equal NaN masks
except within 1e-7 * stride of the hull of the valid points, finite values
within 1e-6 px, and nodes in a full quad that the two sides split along
different diagonals when the quad is co-circular to 1e-9 and the device value
is the other diagonal's interpolant.
"""
import collections

import numpy as np

Box = collections.namedtuple('Box', 'start size')


def box(start, size):
  return Box(tuple(int(v) for v in start), tuple(int(v) for v in size))


def _strides(stride):
  if np.ndim(stride) == 0:
    return stride, stride
  sy, sx = stride
  return sy, sx


def slice_geometry(coord_map, src_box, dst_box, stride):
  """(positions [2, z, y, x] float64, values [2, y, x] int64 source coordinates,
  queries [2, yd, xd] int64, (sy, sx))."""
  sy, sx = _strides(stride)
  cm = np.asarray(coord_map, np.float64)
  h, w = cm.shape[2:]
  x0 = src_box.start[0] - dst_box.start[0]
  y0 = src_box.start[1] - dst_box.start[1]
  yy, xx = np.mgrid[:h, :w]
  pos = cm.copy()
  pos[0] += xx * sx + x0 * sx
  pos[1] += yy * sy + y0 * sy
  vals = np.mgrid[:h, :w]
  vals[0] = (vals[0] + y0) * sy
  vals[1] = (vals[1] + x0) * sx
  qry = np.mgrid[:dst_box.size[1], :dst_box.size[0]]
  qry[0] = qry[0] * sy
  qry[1] = qry[1] * sx
  return pos, vals, qry, (sy, sx)


def invert_restated(coord_map, src_box, dst_box, stride):
  from scipy import interpolate, spatial
  pos, vals, qry, (sy, sx) = slice_geometry(coord_map, src_box, dst_box, stride)
  z = pos.shape[1]
  hd, wd = dst_box.size[1], dst_box.size[0]
  out = np.full((2, z, hd, wd), np.nan)
  qpts = (qry[1].ravel(), qry[0].ravel())
  for k in range(z):
    valid = np.all(np.isfinite(pos[:, k]), axis=0)
    if not valid.any():
      continue
    pts = np.stack([pos[0, k][valid], pos[1, k][valid]], axis=1)
    try:
      tri = spatial.Delaunay(np.ascontiguousarray(pts))
    except spatial.QhullError:
      continue
    v = np.stack([vals[1][valid], vals[0][valid]], axis=1)
    ip = interpolate.LinearNDInterpolator(tri, v, fill_value=np.nan)
    r = ip(qpts)
    out[0, k] = r[:, 0].reshape(hd, wd)
    out[1, k] = r[:, 1].reshape(hd, wd)
  yy, xx = np.mgrid[:hd, :wd]
  out[0] -= xx * sx
  out[1] -= yy * sy
  return out


def _hull_distance(pts, q):
  """Signed distance of the points q [n, 2] from the convex hull of pts."""
  from scipy import spatial
  hull = spatial.ConvexHull(pts)
  eq = hull.equations  # n . x + d <= 0 inside, |n| = 1
  return np.max(q @ eq[:, :2].T + eq[:, 2], axis=1)


def _interp(tri_pts, tri_vals, q):
  p0, p1, p2 = tri_pts
  e1, e2, d = p1 - p0, p2 - p0, q - p0
  det = e1[0] * e2[1] - e1[1] * e2[0]
  l1 = (d[0] * e2[1] - d[1] * e2[0]) / det
  l2 = (e1[0] * d[1] - e1[1] * d[0]) / det
  lam = np.array([1 - l1 - l2, l1, l2])
  inside = lam.min() >= -1e-12
  return inside, lam @ tri_vals


def _incircle_norm(a, b, c, d):
  m = np.array([[a[0] - d[0], a[1] - d[1], (a[0] - d[0])**2 + (a[1] - d[1])**2],
                [b[0] - d[0], b[1] - d[1], (b[0] - d[0])**2 + (b[1] - d[1])**2],
                [c[0] - d[0], c[1] - d[1], (c[0] - d[0])**2 + (c[1] - d[1])**2]])
  scale = max(np.linalg.norm(p - q) for p in (a, b, c, d) for q in (a, b, c, d))
  return abs(np.linalg.det(m)) / scale**4


def check_contract(coord_map, src_box, dst_box, stride, got, want, tol=1e-6):
  """Asserts the parity contract; returns the number of nodes accepted by the
  diagonal exception."""
  return check_contract_counts(coord_map, src_box, dst_box, stride, got, want, tol)[0]


def check_contract_counts(coord_map, src_box, dst_box, stride, got, want, tol=1e-6):
  """Asserts the parity contract; returns (nodes accepted by the diagonal
  exception, nodes whose NaN masks differ on the hull)."""
  got = np.asarray(got, np.float64)
  want = np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  pos, vals, qry, (sy, sx) = slice_geometry(coord_map, src_box, dst_box, stride)
  h, w = pos.shape[2:]
  diag = 0
  mismatches = 0
  yy, xx = np.mgrid[:got.shape[2], :got.shape[3]]
  for k in range(got.shape[1]):
    gn = np.isnan(got[0, k]) | np.isnan(got[1, k])
    wn = np.isnan(want[0, k]) | np.isnan(want[1, k])
    assert np.array_equal(np.isnan(got[0, k]), np.isnan(got[1, k]))
    mism = gn != wn
    mismatches += int(mism.sum())
    valid = np.all(np.isfinite(pos[:, k]), axis=0)
    if mism.any():
      pts = np.stack([pos[0, k][valid], pos[1, k][valid]], axis=1)
      q = np.stack([qry[1][mism], qry[0][mism]], axis=1).astype(np.float64)
      dist = np.abs(_hull_distance(pts, q))
      assert dist.max() <= 1e-7 * min(sx, sy), (
          f'slice {k}: NaN masks differ at {int(mism.sum())} nodes, up to '
          f'{dist.max()} px from the hull')
    both = ~gn & ~wn
    err = np.maximum(np.abs(got[0, k] - want[0, k]), np.abs(got[1, k] - want[1, k]))
    bad = both & (err > tol)
    for v, u in zip(*np.nonzero(bad)):
      q = np.array([qry[1][v, u], qry[0][v, u]], np.float64)
      gv = np.array([got[0, k, v, u] + u * sx, got[1, k, v, u] + v * sy])
      ok = False
      for i in range(h - 1):
        for j in range(w - 1):
          c = [(i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j)]
          if not all(valid[p] for p in c):
            continue
          P = [pos[:, k][:, p[0], p[1]] for p in c]
          V = [np.array([vals[1][p], vals[0][p]], np.float64) for p in c]
          lo, hi = np.min(P, axis=0), np.max(P, axis=0)
          if np.any(q < lo - 1e-9) or np.any(q > hi + 1e-9):
            continue
          if _incircle_norm(*P) > 1e-9:
            continue
          for tris in (((0, 1, 2), (0, 2, 3)), ((0, 1, 3), (1, 2, 3))):
            for t in tris:
              inside, val = _interp([P[m] for m in t], np.array([V[m] for m in t]), q)
              if inside and np.max(np.abs(val - gv)) <= tol:
                ok = True
      assert ok, (f'slice {k}, node (y={v}, x={u}): device {got[:, k, v, u]}, '
                  f'host {want[:, k, v, u]}')
      diag += 1
  return diag, mismatches
