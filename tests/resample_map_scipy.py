"""SciPy statement of map_utils.resample_map (linear) and its contract.

`resample_restated` is SciPy exactly as the reference calls it: per z slice the
nodes whose channel 0 is finite, at `(index + start) * src_stride`, go through
Qhull (`spatial.Delaunay`) and `LinearNDInterpolator`, both channels at once.

The source points are a lattice, so the Delaunay triangulation is not unique
and Qhull's choice is arbitrary.  What every Delaunay triangulation shares is
stated by brute force for tiny maps: a triangle of valid nodes is *admissible*
at a query when it contains the query (closed) and its open circumdisk holds
no valid node; every such triangle belongs to some Delaunay triangulation, and
every Delaunay triangulation answers a query in the hull with one of them.
`admissible_values` lists the linear interpolants over all of them;
`check_contract` asserts that a result is one of them at every query, equals
the reference wherever they all agree, and is NaN exactly outside the hull.
"""
import collections
import itertools

import numpy as np

Box = collections.namedtuple('Box', 'start size')

# two interpolants count as one value below this spread
AGREE = 1e-9


def box(start, size):
  return Box(tuple(int(v) for v in start), tuple(int(v) for v in size))


def lattices(shape, src_box, dst_box, src_stride, dst_stride):
  """(src positions [h * w, 2], queries [hd * wd, 2]) as (x, y) float64 rows,
  formed as the reference forms them: the integer sum, then one product."""
  h, w = shape
  sy, sx = np.mgrid[:h, :w]
  sy = (sy + src_box.start[1]) * src_stride
  sx = (sx + src_box.start[0]) * src_stride
  ty, tx = np.mgrid[:dst_box.size[1], :dst_box.size[0]]
  ty = (ty + dst_box.start[1]) * dst_stride
  tx = (tx + dst_box.start[0]) * dst_stride
  return (np.stack([sx.ravel(), sy.ravel()], 1).astype(np.float64),
          np.stack([tx.ravel(), ty.ravel()], 1).astype(np.float64))


def resample_restated(coord_map, src_box, dst_box, src_stride, dst_stride):
  from scipy import interpolate, spatial
  cm = np.asarray(coord_map)
  assert cm.shape[0] == 2
  pos, qry = lattices(cm.shape[2:], src_box, dst_box, src_stride, dst_stride)
  hd, wd = dst_box.size[1], dst_box.size[0]
  out = np.full((2, cm.shape[1], hd, wd), np.nan, dtype=cm.dtype)
  for z in range(cm.shape[1]):
    valid = np.isfinite(cm[0, z]).ravel()
    if not valid.any():
      continue
    try:
      tri = spatial.Delaunay(np.ascontiguousarray(pos[valid], dtype=np.double))
    except spatial.QhullError:
      continue
    values = np.array([cm[0, z].ravel()[valid], cm[1, z].ravel()[valid]]).T
    ip = interpolate.LinearNDInterpolator(tri, values, fill_value=np.nan)
    r = ip((qry[:, 0], qry[:, 1])).T
    out[0, z] = r[0].reshape(hd, wd)
    out[1, z] = r[1].reshape(hd, wd)
  return out


def admissible_values(valid, values, pos, qry):
  """The interpolants of all admissible triangles, by brute force.

  valid [n] bool, values [n, 2], pos [n, 2], qry [m, 2] (float64).  Returns a
  list of m arrays [k, 2]: the values at query q of the k triangles of valid
  nodes that contain q and whose open circumdisk holds no valid node; k == 0
  outside the convex hull.  Cubic in the number of valid nodes: tiny maps only.
  """
  idx = np.flatnonzero(valid)
  out = [np.zeros((0, 2)) for _ in range(len(qry))]
  if idx.size < 3:
    return out
  p = pos[idx].astype(np.float64)
  v = values[idx].astype(np.float64)
  span = max(np.ptp(p[:, 0]), np.ptp(p[:, 1]), 1e-300)
  tri = np.array(list(itertools.combinations(range(idx.size), 3)))
  a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
  area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
  keep = np.abs(area) > 1e-12 * span**2
  tri, area = tri[keep], area[keep]
  flip = area < 0
  tri[flip] = tri[flip][:, [0, 2, 1]]
  a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
  # open circumdisk empty: the in-circle determinant of no node is positive
  empty = np.ones(len(tri), bool)
  for d in p:
    ad, bd, cd = a - d, b - d, c - d
    det = ((ad**2).sum(1) * (bd[:, 0] * cd[:, 1] - cd[:, 0] * bd[:, 1]) +
           (bd**2).sum(1) * (cd[:, 0] * ad[:, 1] - ad[:, 0] * cd[:, 1]) +
           (cd**2).sum(1) * (ad[:, 0] * bd[:, 1] - bd[:, 0] * ad[:, 1]))
    empty &= det <= 1e-9 * span**4
  tri = tri[empty]
  a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
  e1, e2 = b - a, c - a
  det = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
  for k, q in enumerate(qry):
    d = q - a
    l1 = (d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]) / det
    l2 = (e1[:, 0] * d[:, 1] - e1[:, 1] * d[:, 0]) / det
    l0 = 1 - l1 - l2
    inside = np.minimum(np.minimum(l0, l1), l2) >= -1e-12
    if inside.any():
      t = tri[inside]
      # a zero weight does not let a vertex's NaN in (SciPy's sum does: see the
      # NaN tests, which compare with the reference directly)
      with np.errstate(invalid='ignore'):
        out[k] = (l0[inside, None] * v[t[:, 0]] + l1[inside, None] * v[t[:, 1]] +
                  l2[inside, None] * v[t[:, 2]])
  return out


def _hull_distance(pts, q):
  from scipy import spatial
  eq = spatial.ConvexHull(pts).equations
  return np.max(q @ eq[:, :2].T + eq[:, 2], axis=1)


def check_contract(coord_map, src_box, dst_box, src_stride, dst_stride, got, want, tol=1e-6,
                   hull_exception=True):
  """Asserts the contract of `got` [2, z, yd, xd] against the reference's
  `want` for a tiny `coord_map`; returns (counts, single): a Counter of
  'in_hull' queries, 'single' of them with one admissible value and
  'hull_exception' queries whose NaN mask differs from the reference's within
  1e-7 * stride of the hull; single [z, yd, xd] bool marks the queries where
  all Delaunay triangulations agree.
  """
  cm = np.asarray(coord_map, np.float64)
  got = np.asarray(got, np.float64)
  want = np.asarray(want, np.float64)
  assert got.shape == want.shape, (got.shape, want.shape)
  pos, qry = lattices(cm.shape[2:], src_box, dst_box, src_stride, dst_stride)
  counts = collections.Counter()
  single = np.zeros(got.shape[1:], bool)
  for z in range(cm.shape[1]):
    valid = np.isfinite(cm[0, z]).ravel()
    values = np.stack([cm[0, z].ravel(), cm[1, z].ravel()], 1)
    adm = admissible_values(valid, values, pos, qry)
    g = got[:, z].reshape(2, -1).T
    w = want[:, z].reshape(2, -1).T
    gn, wn = np.isnan(g[:, 0]), np.isnan(w[:, 0])
    mism = np.flatnonzero(gn != wn)
    if mism.size:
      assert hull_exception, f'slice {z}: NaN masks differ at {mism.size} queries'
      dist = np.abs(_hull_distance(pos[valid], qry[mism]))
      assert dist.max() <= 1e-7 * min(src_stride, dst_stride), (
          f'slice {z}: NaN masks differ at {mism.size} queries, up to {dist.max()} from the hull')
      counts['hull_exception'] += int(mism.size)
    for k in range(len(qry)):
      if gn[k] or wn[k]:
        # outside the hull no triangle is admissible (on it, to rounding, some may be)
        assert len(adm[k]) == 0 or gn[k] != wn[k] or not np.isfinite(adm[k]).all(), (
            f'slice {z}, query {k}: NaN inside the hull')
        continue
      counts['in_hull'] += 1
      assert len(adm[k]), f'slice {z}, query {k}: a value outside the hull'
      for name, val in (('result', g[k]), ('reference', w[k])):
        err = np.max(np.abs(adm[k] - val), axis=1)
        assert np.nanmin(err) <= tol, (
            f'slice {z}, query {k} at {qry[k]}: {name} {val} is no admissible value, '
            f'nearest misses by {np.nanmin(err)}')
      if np.max(np.ptp(adm[k], axis=0)) <= AGREE:
        counts['single'] += 1
        single[z].flat[k] = True
        assert np.max(np.abs(g[k] - w[k])) <= tol, (
            f'slice {z}, query {k}: {g[k]} against the reference {w[k]} where all '
            f'Delaunay triangulations agree')
  return counts, single
