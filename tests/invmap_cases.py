"""Edge cases of map_utils.invert_map and their host-side references.

No GPU and nothing of the package is used here: the cases, a NumPy restatement
of the sets R and B of DESIGN.md 1.9, and the analytic inverse of an affine
map, which holds for any triangulation of any subset of the nodes and so
checks the cases that are too large for Qhull.

`edge_cases()` yields `(name, coord_map, src_box, dst_box, stride, expect)`;
`expect` is 'contract' (compare with `ims.invert_restated`), 'affine' (compare
with `affine_inverse`), ('refused', regex) or 'all_nan'.  `CLAIMS[name]` holds
what the case says about itself (boundary nodes, valid nodes per slice, empty
R, degenerate slices, the affine map); tests/test_invert_map_cases.py checks
every claim on the host.
"""
import numpy as np

from tests import invert_map_scipy as ims

STRIDE = 40
MAX_B = 7936  # the kernel's cap on |B|
NODE_BITS = 21

# Largest |invert_restated - affine_inverse| in px over the queries that
# `in_hull` calls inside, per small affine case.  Source:
# tests/test_invert_map_cases.py::test_affine_cases_match_the_restatement, which
# recomputes every figure and fails when one exceeds the value here (the values
# are the measured ones rounded up to two digits).
E_REF = {
    'affine_small_holes': 4.6e-13,
    'cap_strip_7936': 5.9e-11,
    'cap_band_7936': 1.9e-12,
    'cap_strip_two_holes_7936': 5.9e-11,
}
# cases checked against affine_inverse without a SciPy run: E_ref is the
# largest small-case figure scaled by the ratio of the largest coordinates
LARGE_AFFINE = ('nodeid_2p21',)


# ------------------------------------------------------------ sets R and B


def full_quads(valid):
  """[h-1, w-1] bool: quads whose four corners are valid (the lattice part R)."""
  valid = np.asarray(valid, bool)
  return valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, 1:] & valid[1:, :-1]


def boundary_count(valid):
  """|B|: valid nodes that are not the interior vertex of four full quads."""
  valid = np.asarray(valid, bool)
  h, w = valid.shape
  f = np.zeros((h + 1, w + 1), bool)
  f[1:h, 1:w] = full_quads(valid)
  interior = f[:-1, :-1] & f[:-1, 1:] & f[1:, :-1] & f[1:, 1:]
  return int(valid.sum() - (valid & interior).sum())


def valid_nodes(coord_map, src_box, dst_box, stride):
  """[z, h, w] bool: nodes whose absolute position is finite."""
  pos = ims.slice_geometry(coord_map, src_box, dst_box, stride)[0]
  return np.all(np.isfinite(pos), axis=0)


def has_fold(pos):
  """True when a full quad of the slice `pos` [2, h, w] has a non-positive
  triangle under either diagonal (float64 orientation test)."""
  valid = np.all(np.isfinite(pos), axis=0)
  x, y = pos

  def orient(a, b, c):
    return ((x[b] - x[a]) * (y[c] - y[a]) - (y[b] - y[a]) * (x[c] - x[a]))

  h, w = valid.shape
  for i in range(h - 1):
    for j in range(w - 1):
      a, b, c, d = (i, j), (i, j + 1), (i + 1, j + 1), (i + 1, j)
      if not (valid[a] and valid[b] and valid[c] and valid[d]):
        continue
      ac = min(orient(a, b, c), orient(a, c, d))
      bd = min(orient(a, b, d), orient(b, c, d))
      if ac <= 0 and bd <= 0:
        return True
  return False


# ------------------------------------------------------------ affine oracle


def affine_matrix(deg, shear, scale_x, scale_y):
  """Rotation x shear x anisotropic scale, det > 0."""
  t = np.deg2rad(deg)
  rot = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
  a = rot @ np.array([[1.0, shear], [0.0, 1.0]]) @ np.diag([scale_x, scale_y])
  assert np.linalg.det(a) > 0
  return a


def affine_map(A, t, h, w, src_box, stride):
  """Relative [2, 1, h, w] float64 map whose absolute positions are
  p = A @ (X, Y) + t, (X, Y) the absolute lattice coordinates of the src box."""
  sy, sx = ims._strides(stride)
  yy, xx = np.mgrid[:h, :w]
  X = (xx + src_box.start[0]) * float(sx)
  Y = (yy + src_box.start[1]) * float(sy)
  px = A[0, 0] * X + A[0, 1] * Y + t[0]
  py = A[1, 0] * X + A[1, 1] * Y + t[1]
  return np.stack([px - X, py - Y])[:, None]


def affine_points(A, t, valid, src_box, stride):
  """Absolute positions [n, 2] (x, y) in the dst-independent frame of the valid nodes."""
  sy, sx = ims._strides(stride)
  i, j = np.nonzero(valid)
  X = (j + src_box.start[0]) * float(sx)
  Y = (i + src_box.start[1]) * float(sy)
  return np.stack([A[0, 0] * X + A[0, 1] * Y + t[0], A[1, 0] * X + A[1, 1] * Y + t[1]], axis=1)


def dst_queries(dst_box, stride):
  """Absolute query positions [n, 2] (x, y), row-major over the dst lattice."""
  sy, sx = ims._strides(stride)
  yy, xx = np.mgrid[:dst_box.size[1], :dst_box.size[0]]
  return np.stack([((xx + dst_box.start[0]) * float(sx)).ravel(),
                   ((yy + dst_box.start[1]) * float(sy)).ravel()], axis=1)


def affine_inverse(A, t, src_box, dst_box, stride):
  """The inverse of the affine map in relative format, float64
  [2, 1, dst y, dst x]: A^-1 (q - t) - q at every dst node q (integer strides).
  Exact wherever the query lies in the convex hull of the valid nodes."""
  del src_box  # A and t are stated in absolute coordinates
  q = dst_queries(dst_box, stride)
  inv = np.linalg.inv(A)
  d = q - np.asarray(t, np.float64)
  sx_ = inv[0, 0] * d[:, 0] + inv[0, 1] * d[:, 1]
  sy_ = inv[1, 0] * d[:, 0] + inv[1, 1] * d[:, 1]
  hd, wd = dst_box.size[1], dst_box.size[0]
  return np.stack([(sx_ - q[:, 0]).reshape(hd, wd), (sy_ - q[:, 1]).reshape(hd, wd)])[:, None]


def in_hull(points, queries, eps):
  """+1 for queries [n, 2] more than eps inside the convex hull of points
  [m, 2], -1 for those more than eps outside, 0 for those within eps of it."""
  from scipy import spatial
  eq = spatial.ConvexHull(points).equations  # n . x + d <= 0 inside, |n| = 1
  queries = np.asarray(queries, np.float64)
  dist = np.full(len(queries), -np.inf)
  for nx, ny, d in eq:
    np.maximum(dist, queries[:, 0] * nx + queries[:, 1] * ny + d, out=dist)
  return np.where(dist < -eps, 1, np.where(dist > eps, -1, 0))


def affine_tolerance(name, max_coord):
  """max(16 E_ref, 64 ulp of the largest coordinate), never above the
  contract's 1e-6 px.  E_ref of a large case: the largest small-case figure
  scaled by the ratio of the largest coordinates."""
  if name in E_REF:
    e_ref = E_REF[name]
  else:
    big = max(E_REF, key=E_REF.get)
    e_ref = E_REF[big] * max_coord / CLAIMS[big]['max_coord']
  return min(max(16 * e_ref, 64 * np.spacing(max_coord)), 1e-6)


# ------------------------------------------------------------ builders

CLAIMS = {}
_BUILDERS = {}


def _case(name):
  def deco(fn):
    _BUILDERS[name] = fn
    return fn
  return deco


def smooth(rng, z, h, w, amp, sigma=1.5):
  """Two smooth random fields [2, z, h, w], peak `amp` ([y, x] pair or scalar)."""
  from scipy import ndimage
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, h, w)), (0, sigma, sigma),
                                        mode='nearest') for _ in range(2)])
  f /= np.abs(f).reshape(2, -1).max(axis=1)[:, None, None, None]
  amp = np.broadcast_to(np.asarray(amp, np.float64), (2,))
  return f * amp[:, None, None, None]


def _checker(h, w):
  yy, xx = np.mgrid[:h, :w]
  return (yy + xx) % 2 == 0


def degenerate_slice(kind, h, w, x0, y0, rng, stride=STRIDE):
  """A [2, h, w] slice of the named kind and (valid nodes, degenerate?)."""
  s = np.full((2, h, w), np.nan)
  if kind == 'empty':
    return s, 0, True
  if kind == 'one':
    s[:, h // 2, w // 2] = rng.uniform(-5, 5, 2)
    return s, 1, True
  if kind == 'two':
    s[:, 0, 0] = rng.uniform(-5, 5, 2)
    s[:, h - 1, w - 1] = rng.uniform(-5, 5, 2)
    return s, 2, True
  if kind == 'row':  # one valid row, moved along the row only: collinear
    r = h // 2
    s[0, r] = np.round(rng.uniform(-0.3 * stride, 0.3 * stride, w))
    s[1, r] = 3.0
    return s, w, True
  if kind == 'coincident':  # every other node, all at one absolute position
    yy, xx = np.nonzero(_checker(h, w))
    s[0, yy, xx] = 101.25 - (xx + x0) * stride
    s[1, yy, xx] = 57.75 - (yy + y0) * stride
    return s, len(yy), True
  if kind == 'three':
    for y, x in ((0, 0), (0, w - 1), (h - 1, w // 2)):
      s[:, y, x] = rng.uniform(-0.3 * stride, 0.3 * stride, 2)
    return s, 3, False
  if kind.startswith('four'):  # isolated nodes of the undeformed lattice: co-circular
    dy, dx = int(kind[4]), int(kind[5])
    for y in (0, dy):
      for x in (0, dx):
        s[:, y, x] = 0.0
    return s, 4, False
  raise ValueError(kind)


# slice index -> kind; every other slice is a good smooth slice
MIX_37 = {3: 'empty', 5: 'one', 8: 'two', 9: 'row', 13: 'coincident', 17: 'three', 20: 'four22',
          21: 'four25', 22: 'four42', 23: 'empty', 30: 'one', 36: 'three'}
MIX_300 = {1: 'empty', 6: 'one', 7: 'two', 13: 'row', 14: 'coincident', 63: 'three',
           64: 'four22', 65: 'good', 128: 'empty', 191: 'four22', 255: 'row', 256: 'three',
           257: 'coincident', 299: 'two'}


def _waves(name, seed, z, h, w, mix, axis_only=None):
  rng = np.random.default_rng(seed)
  s = STRIDE
  src = ims.box((7, 3, 0), (w, h, z))
  dst = ims.box((6, 2, 0), (w + 2, h + 2, z))
  amp = 0.3 * s
  cm = smooth(rng, z, h, w, amp, sigma=1.0)
  if axis_only == 'x':  # a single row, moved along itself
    cm[1] = 0.0
  if axis_only == 'y':
    cm[0] = 0.0
  nvalid = [h * w] * z
  degenerate = [axis_only is not None] * z
  on_hull = []
  for k, kind in mix.items():
    if kind == 'good':
      continue
    cm[:, k], nvalid[k], degenerate[k] = degenerate_slice(kind, h, w, 1, 1, rng)
    if kind.startswith('four'):
      on_hull.append(k)  # lattice nodes: the queries lie on the hull by construction
  CLAIMS[name] = dict(nvalid=nvalid, degenerate=degenerate, on_hull=on_hull,
                      r_empty=[not full_quads(v).any()
                               for v in valid_nodes(cm, src, dst, s)])
  return cm, src, dst, s


@_case('waves_37x5x7')
def _():
  return (*_waves('waves_37x5x7', 101, 37, 5, 7, MIX_37), 'contract')


@_case('waves_300x3x3')
def _():
  return (*_waves('waves_300x3x3', 103, 300, 3, 3, MIX_300), 'contract')


@_case('waves_5x2x40')
def _():
  return (*_waves('waves_5x2x40', 113, 5, 2, 40, {}), 'contract')


@_case('row_3x1x9')
def _():
  return (*_waves('row_3x1x9', 104, 3, 1, 9, {}, axis_only='x'), 'all_nan')


@_case('col_3x9x1')
def _():
  return (*_waves('col_3x9x1', 105, 3, 9, 1, {}, axis_only='y'), 'all_nan')


@_case('four_cocircular_5_5')
def _():
  """Four isolated nodes of the undeformed lattice five nodes apart: R is
  empty and the completion breaks the in-circle tie symbolically."""
  name = 'four_cocircular_5_5'
  cm = np.full((2, 1, 8, 8), np.nan)
  for y in (1, 6):
    for x in (1, 6):
      cm[:, 0, y, x] = 0.0
  b = ims.box((0, 0, 0), (8, 8, 1))
  CLAIMS[name] = dict(nvalid=[4], degenerate=[False], on_hull=[0], r_empty=[True], boundary=[4])
  return cm, b, b, STRIDE, 'contract'


def _affine_case(name, h, w, A, t0, holes, margin=2):
  """An affine map with NaN `holes` ([h, w] bool); the dst box covers the
  image of the map plus `margin` nodes per side."""
  s = STRIDE
  src = ims.box((0, 0, 0), (w, h, 1))
  cm = affine_map(A, t0, h, w, src, s)
  cm[:, 0, holes] = np.nan
  corners = np.array([[0, 0], [(w - 1) * s, 0], [0, (h - 1) * s], [(w - 1) * s, (h - 1) * s]],
                     np.float64)
  p = corners @ A.T + t0
  lo = np.floor(p.min(axis=0) / s).astype(int) - margin
  hi = np.ceil(p.max(axis=0) / s).astype(int) + margin
  dst = ims.box((lo[0], lo[1], 0), (hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, 1))
  valid = ~holes
  CLAIMS[name] = dict(A=A, t=np.asarray(t0, np.float64), boundary=[boundary_count(valid)],
                      nvalid=[int(valid.sum())], r_empty=[not full_quads(valid).any()],
                      max_coord=float(max(np.abs(p).max(), abs(lo).max() * s, abs(hi).max() * s)))
  return cm, src, dst, s, 'affine'


@_case('affine_small_holes')
def _():
  holes = np.zeros((24, 28), bool)
  holes[9, 9] = holes[15:18, 4:6] = holes[:3, 20:] = True
  holes[10:14, 14:22] = ~_checker(4, 8)
  return _affine_case('affine_small_holes', 24, 28, affine_matrix(7.0, 0.1, 1.05, 0.93),
                      (13.37, -7.25), holes)


_STRIP_A = affine_matrix(0.05, 0.02, 1.01, 0.97)


@_case('cap_strip_7936')
def _():
  """[2, 1, 2, 3968], all valid: every node is a boundary node."""
  out = _affine_case('cap_strip_7936', 2, 3968, _STRIP_A, (3.5, 11.25),
                     np.zeros((2, 3968), bool))
  assert CLAIMS['cap_strip_7936']['boundary'] == [MAX_B]
  return out


def _strip_3969(nholes):
  holes = np.zeros((2, 3969), bool)
  holes[0, 1000] = True
  if nholes == 2:
    holes[1, 2500] = True
  return holes


@_case('cap_strip_two_holes_7936')
def _():
  """[2, 1, 2, 3969] with two NaN nodes: |B| = 7936, accepted."""
  name = 'cap_strip_two_holes_7936'
  out = _affine_case(name, 2, 3969, _STRIP_A, (3.5, 11.25), _strip_3969(2))
  assert CLAIMS[name]['boundary'] == [MAX_B]
  return out


@_case('cap_strip_one_hole_7937')
def _():
  """The same map with one NaN node: |B| = 7937, refused."""
  name = 'cap_strip_one_hole_7937'
  cm, src, dst, s, _ = _affine_case(name, 2, 3969, _STRIP_A, (3.5, 11.25), _strip_3969(1))
  assert CLAIMS[name]['boundary'] == [MAX_B + 1]
  return cm, src, dst, s, ('refused', r'slice 0 refused: more than 7936 boundary nodes$')


def band_holes(n=130, target=MAX_B):
  """The checkerboard of NaN restricted to a band of rows of an n x n map,
  then single holes until |B| is exactly `target`.  R keeps the rows above and
  below the band, so the band's nodes sit in real pockets."""
  holes = np.zeros((n, n), bool)
  r0 = r1 = 4
  while r1 < n - 12:  # widen the band while the count stays at or below the target
    trial = holes.copy()
    trial[r0:r1 + 1] = ~_checker(r1 + 1 - r0, n)
    if boundary_count(~trial) > target:
      break
    holes = trial
    r1 += 1
  # single holes below the band, three nodes apart: 8 new boundary nodes each,
  # then fewer next to the border
  cands = [(y, x) for y in range(r1 + 4, n - 3, 3) for x in range(3, n - 3, 3)]
  cands += [(n - 2, x) for x in range(3, n - 3, 3)] + [(n - 1, x) for x in range(4, n - 3, 3)]
  for y, x in cands:
    if boundary_count(~holes) == target:
      break
    trial = holes.copy()
    trial[y, x] = True
    if boundary_count(~trial) <= target:
      holes = trial
  return holes


@_case('cap_band_7936')
def _():
  name = 'cap_band_7936'
  out = _affine_case(name, 130, 130, affine_matrix(4.0, 0.08, 1.04, 0.95), (21.5, -9.75),
                     band_holes())
  assert CLAIMS[name]['boundary'] == [MAX_B] and not CLAIMS[name]['r_empty'][0]
  return out


def _jagged(h, w, rows, cols, from_top):
  """A NaN blob with a jagged rim: column c loses 1 + (5 c mod rows) nodes."""
  holes = np.zeros((h, w), bool)
  for c in cols:
    d = 1 + (5 * c) % rows
    if from_top:
      holes[:d, c] = True
    else:
      holes[h - d:, c] = True
  return holes


@_case('nodeid_2p21')
def _():
  """H * W == 2^21: NaN blobs in the last 8 rows and at the top left, so
  completion triangles carry node ids just under 2^21 and near 0."""
  name = 'nodeid_2p21'
  h, w = 1024, 2048
  holes = _jagged(h, w, 8, range(w - 160, w), False) | _jagged(h, w, 8, range(0, 160), True)
  out = _affine_case(name, h, w, affine_matrix(0.05, 0.003, 1.002, 0.998), (17.25, -5.5), holes)
  assert h * w == 1 << NODE_BITS and CLAIMS[name]['boundary'][0] < MAX_B
  assert holes[0, 0] and holes[h - 1, w - 1]
  return out


@_case('nodeid_over_2p21')
def _():
  cm = np.zeros((2, 1, 1024, 2049), np.float32)
  b = ims.box((0, 0, 0), (2049, 1024, 1))
  d = ims.box((0, 0, 0), (4, 4, 1))
  return cm, b, d, STRIDE, ('refused', r'2098176 nodes per slice exceed 2\^21')


def _fold(cm, k, y, x):
  cm[0, k, y, x] = 55.0  # the node jumps past its right neighbour
  cm[1, k, y, x] = 0.0


@_case('status_fold_1_4')
def _():
  """good, fold, all-NaN, good, fold."""
  rng = np.random.default_rng(110)
  cm = smooth(rng, 5, 20, 20, 0.3 * STRIDE, sigma=2.0)
  cm[:, 1] = 0.0
  cm[:, 4] *= 0.25
  _fold(cm, 1, 10, 10)
  _fold(cm, 4, 6, 13)
  cm[:, 2] = np.nan
  b = ims.box((0, 0, 0), (20, 20, 5))
  CLAIMS['status_fold_1_4'] = dict(folds=[1, 4])
  return cm, b, b, STRIDE, ('refused', r'^invert_map: slice 1 refused: folded or degenerate quad'
                            r'[^()]* \(2 slices refused: \[1, 4\]\)$')


@_case('status_cap_1_fold_2')
def _():
  """7936 boundary nodes, 7937 boundary nodes, 7936 and a fold."""
  s = STRIDE
  cm = np.zeros((2, 3, 2, 3969))
  cm[:, :, 0, 1000] = np.nan
  cm[:, 0, 1, 2500] = np.nan
  cm[:, 2, 1, 2500] = np.nan
  _fold(cm, 2, 0, 2000)
  b = ims.box((0, 0, 0), (3969, 2, 3))
  d = ims.box((0, 0, 0), (8, 2, 3))
  CLAIMS['status_cap_1_fold_2'] = dict(folds=[2], boundary=[7936, 7937, 7936])
  return cm, b, d, s, ('refused', r'^invert_map: slice 1 refused: more than 7936 boundary nodes '
                       r'\(2 slices refused: \[1, 2\]; slice 2: folded or degenerate quad[^()]*\)$')


def _nonfinite(name, seed, value, channel):
  rng = np.random.default_rng(seed)
  cm = smooth(rng, 1, 12, 14, 0.3 * STRIDE)
  cm[channel, 0, 5, 6] = value
  src = ims.box((7, 3, 0), (14, 12, 1))
  dst = ims.box((6, 2, 0), (16, 14, 1))
  CLAIMS[name] = dict(nvalid=[12 * 14 - 1], degenerate=[False], on_hull=[], r_empty=[False],
                      boundary=[2 * (12 + 14) - 4 + 8])
  return cm, src, dst, STRIDE, 'contract'


@_case('hole_posinf_x')
def _():
  return _nonfinite('hole_posinf_x', 120, np.inf, 0)


@_case('hole_neginf_y')
def _():
  return _nonfinite('hole_neginf_y', 121, -np.inf, 1)


@_case('hole_nan_x')
def _():
  return _nonfinite('hole_nan_x', 122, np.nan, 0)


@_case('huge_1e300')
def _():
  """One node at 1e300: the slice's exponent sends every other node to one
  grid point, every quad degenerates and the slice is refused by name.  (Qhull
  fails on the same points, so the restatement has no answer to compare.)"""
  rng = np.random.default_rng(123)
  cm = smooth(rng, 2, 12, 14, 0.3 * STRIDE)
  cm[0, 1, 5, 6] = 1e300
  b = ims.box((0, 0, 0), (14, 12, 2))
  return cm, b, b, STRIDE, ('refused', r'^invert_map: slice 1 refused: folded or degenerate quad[^()]*$')


def _disjoint(name, dx, dy):
  rng = np.random.default_rng(130)
  cm = smooth(rng, 2, 16, 16, 0.3 * STRIDE)
  src = ims.box((500, 700, 0), (16, 16, 2))
  dst = ims.box((500 + dx, 700 + dy, 0), (64, 64, 2))
  return cm, src, dst, STRIDE, 'all_nan'


for _n, _dx, _dy in (('disjoint_x_plus', 100000, 0), ('disjoint_x_minus', -100000, 0),
                     ('disjoint_y_plus', 0, 100000), ('disjoint_y_minus', 0, -100000)):
  _BUILDERS[_n] = (lambda n=_n, dx=_dx, dy=_dy: _disjoint(n, dx, dy))


def _stride_case(name, seed, stride, rough=False):
  """The source starts 3 nodes left of and above the dst start, so source
  coordinates are negative and truncation differs from floor.

  The amplitude keeps the lattice Delaunay: with strides a <= b, the node two
  steps along the short axis clears the circumcircle of a lattice quad by about
  2 a^2 / b, and the field moves a node by at most 0.3 a^2 / b.  `rough` moves
  it by 0.3 x stride per axis, which a lattice of unequal strides does not
  survive."""
  rng = np.random.default_rng(seed)
  h, w = 20, 22
  sy, sx = stride
  amp = (0.3 * sx, 0.3 * sy) if rough else 0.3 * min(sy, sx)**2 / max(sy, sx)
  cm = smooth(rng, 1, h, w, amp)
  src = ims.box((10, 20, 0), (w, h, 1))
  dst = ims.box((13, 23, 0), (w, h, 1))
  CLAIMS[name] = dict(nvalid=[h * w], degenerate=[False], on_hull=[], r_empty=[False],
                      boundary=[2 * (h + w) - 4])
  return cm, src, dst, stride, 'contract'


@_case('stride_0.5_0.5')
def _():
  return _stride_case('stride_0.5_0.5', 140, (0.5, 0.5))


@_case('stride_0.3_2.5')
def _():
  return _stride_case('stride_0.3_2.5', 141, (0.3, 2.5))


@_case('stride_0.3_2.5_rough')
def _():
  cm, src, dst, stride, _ = _stride_case('stride_0.3_2.5_rough', 141, (0.3, 2.5), rough=True)
  return cm, src, dst, stride, ('refused', r'^invert_map: slice 0 refused: '
                                r'edge not locally Delaunay$')


@_case('stride_30.5_29.25')
def _():
  return _stride_case('stride_30.5_29.25', 142, (30.5, 29.25))


def _blobs(name, seed, z, n, quantile):
  from scipy import ndimage
  rng = np.random.default_rng(seed)
  cm = smooth(rng, z, n, n, 0.3 * STRIDE, sigma=3.0)
  noise = ndimage.gaussian_filter(rng.standard_normal((z, n, n)), (0, 1.5, 1.5))
  cm[:, noise > np.quantile(noise, quantile)] = np.nan
  src = ims.box((7, 3, 0), (n, n, z))
  dst = ims.box((6, 2, 0), (n + 2, n + 2, z))
  valid = valid_nodes(cm, src, dst, STRIDE)
  CLAIMS[name] = dict(nvalid=[int(v.sum()) for v in valid], degenerate=[False] * z, on_hull=[],
                      r_empty=[False] * z)
  return cm, src, dst, STRIDE, 'contract'


@_case('reuse_A_96')
def _():
  return _blobs('reuse_A_96', 150, 1, 96, 0.9)


@_case('reuse_B_20')
def _():
  return _blobs('reuse_B_20', 151, 1, 20, 0.8)


@_case('reuse_B_20x3')
def _():
  """reuse_B_20 three times over: every slice must equal the single one."""
  _, cm, src, dst, stride, _ = case('reuse_B_20')
  CLAIMS['reuse_B_20x3'] = {k: v * 3 for k, v in CLAIMS['reuse_B_20'].items()}
  return (np.concatenate([cm] * 3, axis=1), ims.box(src.start, src.size[:2] + (3,)),
          ims.box(dst.start, dst.size[:2] + (3,)), stride, 'contract')


NAMES = tuple(_BUILDERS)
_built = {}


def case(name):
  """(name, coord_map, src_box, dst_box, stride, expect); built once, read-only."""
  if name not in _built:
    cm, src, dst, stride, expect = _BUILDERS[name]()
    cm.setflags(write=False)
    _built[name] = (name, cm, src, dst, stride, expect)
  return _built[name]


def edge_cases(names=NAMES):
  for name in names:
    yield case(name)


def names_expecting(kind):
  """Case names by expectation, without building the large ones."""
  big = {'nodeid_2p21': 'affine', 'nodeid_over_2p21': 'refused'}
  out = []
  for name in NAMES:
    e = big[name] if name in big else case(name)[5]
    e = e[0] if isinstance(e, tuple) else e
    if e == kind:
      out.append(name)
  return out
