"""Float64 references and input helpers shared by the edge tests
(tests/test_gpu_postflow_edges.py, tests/test_gpu_montage_edges.py and their
CPU companions).  Plain helpers: no test lives here and nothing needs a GPU."""
import itertools

import numpy as np

f32 = np.float32


def around(v):
  """The float32 nearest to v and its two neighbours on either side."""
  c = f32(v)
  lo1 = np.nextafter(c, f32(-np.inf))
  hi1 = np.nextafter(c, f32(np.inf))
  return [np.nextafter(lo1, f32(-np.inf)), lo1, c, hi1, np.nextafter(hi1, f32(np.inf))]


def sample64(vol, q, mode):
  """Bi- / trilinear sample of `vol` at index coordinates q (one array per
  axis), in double.  Per corner: 'constant' -- any index out of range makes the
  corner NaN; 'nearest' -- indices are clamped.  A NaN corner poisons the sum
  whatever its weight."""
  nan_q = np.zeros(q[0].shape, bool)
  los, ws = [], []
  for c in q:
    nan_q |= np.isnan(c)
    c = np.where(np.isnan(c), 0.0, c)
    lo = np.floor(c)
    los.append(lo.astype(np.int64))
    ws.append(c - lo)
  total = np.zeros(q[0].shape, np.float64)
  for corner in itertools.product((0, 1), repeat=len(q)):
    w = np.ones(q[0].shape, np.float64)
    valid = np.ones(q[0].shape, bool)
    idx = []
    for ax, pick in enumerate(corner):
      i = los[ax] + pick
      valid &= (i >= 0) & (i < vol.shape[ax])
      idx.append(np.clip(i, 0, vol.shape[ax] - 1))
      w = w * (ws[ax] if pick else 1.0 - ws[ax])
    val = vol[tuple(idx)]
    if mode == 'constant':
      val = np.where(valid, val, np.nan)
    total = total + w * val
  return np.where(nan_q, np.nan, total)


def compose64(map1, start1, stride1, map2, start2, stride2, mode):
  """map2(map1(.)) over map1's lattice from the definition, all in double:
  absolute coordinates of map1's nodes relative to origin = min(start1,
  start2), divided by stride2 to index map2's absolute coordinates (the
  documented operation: map2's own start enters its coordinates only), sampled
  linearly, made relative to map1's lattice again.

  Returns (result, near, M): `near` marks queries within 4 float32 ulps of an
  integer index on some axis without being ON it, where a float32 evaluation
  may choose the neighbouring cell (the value is continuous there, the set of
  corners is not; a query exactly on a node is exact in float32 too: dyadic
  strides); M is the largest finite absolute coordinate |ref2 + map2|."""
  m1 = np.asarray(map1, f32).astype(np.float64)
  m2 = np.asarray(map2, f32).astype(np.float64)
  dim = m1.shape[0]
  vec = lambda v: tuple(float(a) for a in np.ravel(v)[-dim:]) if np.ndim(v) else (float(v),) * dim
  st1, st2 = vec(stride1), vec(stride2)
  s1 = np.asarray(start1, np.float64).ravel()[-dim:]
  s2 = np.asarray(start2, np.float64).ravel()[-dim:]
  origin = np.minimum(s1, s2)

  def lattice(shape, start, stride):
    axes = [(np.arange(n) + (start[i] - origin[i])) * stride[i] for i, n in enumerate(shape)]
    return np.meshgrid(*axes, indexing='ij')   # [z]yx

  ref1 = lattice(m1.shape[-dim:], s1, st1)
  ref2 = lattice(m2.shape[-dim:], s2, st2)
  out = np.zeros_like(m1)
  near = np.zeros(m1.shape[1:], bool)
  big = 0.0

  def note(q):
    with np.errstate(invalid='ignore'):
      hit = np.zeros(q[0].shape, bool)
      for c in q:
        off = np.abs(c - np.rint(c))
        hit |= (off > 0) & (off <= 4 * 2.0**-24 * np.maximum(np.abs(c), 1.0))
    return hit

  if dim == 2:
    for z in range(m1.shape[1]):
      q = [(ref1[0] + m1[1, z]) / st2[0], (ref1[1] + m1[0, z]) / st2[1]]
      near[z] = note(q)
      for c, ax in ((0, 1), (1, 0)):
        vol = m2[c, z] + ref2[ax]
        fin = vol[np.isfinite(vol)]
        big = max(big, float(np.abs(fin).max()) if fin.size else 0.0)
        out[c, z] = sample64(vol, q, mode) - ref1[ax]
  else:
    q = [(ref1[0] + m1[2]) / st2[0], (ref1[1] + m1[1]) / st2[1], (ref1[2] + m1[0]) / st2[2]]
    near[...] = note(q)
    for c, ax in ((0, 2), (1, 1), (2, 0)):
      vol = m2[c] + ref2[ax]
      fin = vol[np.isfinite(vol)]
      big = max(big, float(np.abs(fin).max()) if fin.size else 0.0)
      out[c] = sample64(vol, q, mode) - ref1[ax]
  return out, near, big


def compose_atol(dim, big):
  """The output is a difference of two absolute coordinates; the sampled one
  is a sum of T float32 products (T = 4 bilinear, 8 trilinear)."""
  return ((4 if dim == 2 else 8) + 3) * 2.0**-24 * big


def smooth(rng, shape, amp, waves=2.5):
  """Smooth field on a [z, y, x] lattice: a few sines, plus a little noise."""
  grids = np.meshgrid(*[np.linspace(0, 1, n) if n > 1 else np.zeros(1) for n in shape],
                      indexing='ij')
  out = np.zeros(shape)
  for _ in range(3):
    ph = rng.uniform(0, 2 * np.pi, len(shape))
    k = rng.uniform(0.5, waves, len(shape)) * 2 * np.pi
    term = np.ones(shape)
    for g, kk, pp in zip(grids, k, ph):
      term = term * np.sin(kk * g + pp)
    out += term
  out = out / 3 * amp + rng.standard_normal(shape) * 0.02 * amp
  return out


# ---------------------------------------------------------------------------
# Peak search (flow_field.py:178-275): reference and cases shared by
# tests/test_gpu_peaks_ndwarp_edges.py and tests/test_peaks_ndwarp_refs.py
# ---------------------------------------------------------------------------
def peak_mask64(img, min_distance, threshold_rel):
  """[b, ...] bool: the peaks of every surface.  An element is a peak when it
  exceeds threshold_rel x the surface maximum (one float32 product, strict) and
  equals the maximum of its (2 min_distance + 1)^dim window, the surface
  zero-padded.  A surface whose maximum is NaN (any NaN element) or whose
  threshold is not finite below its elements (+inf) has none."""
  img = np.asarray(img, f32)
  m = int(min_distance)
  sp = img.shape[1:]
  mask = np.zeros(img.shape, bool)
  for n in range(img.shape[0]):
    s = img[n]
    if np.isnan(s).any():
      continue
    with np.errstate(invalid='ignore'):
      thr = f32(threshold_rel) * s.max()
    padded = np.zeros(tuple(a + 2 * m for a in sp), f32)
    padded[tuple(slice(m, m + a) for a in sp)] = s
    wmax = np.full(sp, -np.inf, f32)
    for off in itertools.product(range(2 * m + 1), repeat=len(sp)):
      wmax = np.maximum(wmax, padded[tuple(slice(o, o + a) for o, a in zip(off, sp))])
    with np.errstate(invalid='ignore'):
      mask[n] = (s > thr) & (s == wmax)
  return mask


def peaks64(img, center, min_distance, threshold_rel, radius, group=None):
  """Top-two peak statistics of a batch of surfaces -> [b, dim + 2] float32:
  x, y[, z] of the first peak relative to `center`, sharpness, ratio.

  Per surface: the first peak is the largest peak, the lowest flat index among
  equals; no peak -> a NaN row whose first-peak index counts as 0.  The flat
  first-peak indices of ALL surfaces of the batch (of each run of `group`
  surfaces, when given) are struck from every surface's peak list; the second
  peak is the largest left.  With none left the reference's arg-max lands on
  flat index 0 and reads the UN-struck list there: the element's value when
  index 0 is a peak, else nothing (ratio 0).  sharpness = first / min over the
  window of 2 r + 1 elements per axis around it, shifted to stay inside the
  surface and CLIPPED to the surface where the surface is smaller (the
  reference has no answer there; this is the project's rule).  Both quotients
  are single float32 divisions."""
  img = np.asarray(img, f32)
  b, sp = img.shape[0], img.shape[1:]
  dim = len(sp)
  rad = [int(radius)] * dim if np.ndim(radius) == 0 else [int(r) for r in radius]
  group = b if group is None else int(group)
  mask = peak_mask64(img, min_distance, threshold_rel).reshape(b, -1)
  flat = img.reshape(b, -1)
  first = np.zeros(b, np.int64)
  for n in range(b):
    idx = np.flatnonzero(mask[n])
    if idx.size:
      first[n] = idx[flat[n, idx] == flat[n, idx].max()][0]
  out = np.full((b, dim + 2), np.nan, f32)
  for n in range(b):
    idx = np.flatnonzero(mask[n])
    if not idx.size:
      continue
    g0 = n // group * group
    left = np.setdiff1d(idx, first[g0:g0 + group])
    if left.size:
      second = flat[n, left].max()
    else:
      second = flat[n, 0] if mask[n, 0] else None
    pos = np.unravel_index(first[n], sp)
    win = []
    for a in range(dim):
      size = min(2 * rad[a] + 1, sp[a])
      start = min(max(pos[a] - size // 2, 0), sp[a] - size)
      win.append(slice(start, start + size))
    v1 = flat[n, first[n]]
    with np.errstate(divide='ignore', invalid='ignore'):
      out[n, :dim] = [f32(pos[a]) - f32(center[a]) for a in range(dim)][::-1]
      out[n, dim] = v1 / img[n][tuple(win)].min()
      out[n, dim + 1] = f32(0) if second is None else v1 / second
  return out


def _pcase(name, img, center, m, t, r, oracle=True):
  img = np.ascontiguousarray(img, f32)
  img.setflags(write=False)
  return dict(name=name, img=img, center=tuple(center), min_distance=m, threshold_rel=t,
              radius=r, oracle=oracle)


def _scatter(shape, flat_idx, values, fill=0.0):
  s = np.full(int(np.prod(shape)), fill, f32)
  s[np.asarray(flat_idx)] = values
  return s.reshape(shape)


def peaks_capacity_cases():
  """min_distance 0 on 64 x 70: every element above the threshold is a peak.
  Surface 1 (one of the first workgroup's four) and surface 4 (alone in the
  second) hold exactly n peaks, n on either side of the candidate capacity
  2048; the others a few hundred.  'distinct': all values differ; 'equal':
  all peaks are 1, so the lowest index wins twice."""
  cases = []
  for n in (2047, 2048, 2049):
    for kind in ('distinct', 'equal'):
      rng = np.random.default_rng(n)
      surfs = []
      for cnt in (300, n, 700, 1500, n):
        idx = rng.choice(64 * 70, cnt, replace=False)
        vals = (1 + rng.permutation(64 * 70)[:cnt] / 8192.0) if kind == 'distinct' else 1.0
        surfs.append(_scatter((64, 70), idx, vals))
      cases.append(_pcase(f'cap{n}_{kind}', np.stack(surfs), (32, 35), 0, 0.5, 5))
  return cases


def _edge_peaks(rng, shape):
  """Noise in [0, 1) with distinct larger values in every corner and on the
  first / last row and column of the last two axes."""
  s = rng.random(shape).astype(f32)
  h, w = shape[-2:]
  spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3),
           (h // 2, 0), (h // 3, w - 1)]
  vals = 1.5 + rng.permutation(len(spots)) / 16.0
  for (y, x), v in zip(spots, vals):
    for z in ([0, shape[0] - 1] if len(shape) == 3 else [Ellipsis]):
      s[z, y, x] = v + (0.01 if z == 0 else 0.0) if len(shape) == 3 else v
  return s


def peaks_sweep_cases():
  """Every row-sweep template (width <= 64 / 128 / 256 / above) at row counts
  that are no multiple of waves x piece, and the three sizes around the switch
  to the multi-workgroup first pass.  Batch 3; the radius shrinks with the
  surface so that the oracle is defined."""
  cases = []
  for w in (1, 63, 64, 65, 128, 129, 256, 257, 300):
    for h in (1, 3, 4, 5, 33):
      rng = np.random.default_rng(1000 * w + h)
      img = np.stack([_edge_peaks(rng, (h, w)) for _ in range(3)])
      r = (min(5, (h - 1) // 2), min(5, (w - 1) // 2))
      cases.append(_pcase(f'sweep_{h}x{w}', img, (h // 2, w // 2), 2, 0.5, r))
  for shape, c, r in (((511, 513), (255, 256), 5), ((512, 512), (256, 256), (5, 3)),
                      ((64, 64, 64), (32, 32, 32), (1, 2, 2))):
    rng = np.random.default_rng(shape[-1])
    img = np.stack([_edge_peaks(rng, shape) for _ in range(3)])
    cases.append(_pcase('sweep_' + 'x'.join(map(str, shape)), img, c, 2, 0.5, r))
  return cases


def peaks_window_cases():
  """Forms of the peak window: min_distance 0 ... 7 and larger than the
  surface, 2-D and 3-D; pairs of maxima, equal and unequal, at distance exactly
  min_distance (inside one another's window) and one more; a plateau; negative
  border elements next to the zero padding."""
  cases = []
  for shape, c, r, ms in (((17, 19), (8, 9), 5, (0, 1, 2, 3, 7, 20)),
                          ((6, 9, 10), (3, 4, 5), (1, 2, 2), (0, 1, 2, 3, 12))):
    for m in ms:
      rng = np.random.default_rng(m)
      img = np.stack([rng.random(shape).astype(f32) for _ in range(3)])
      cases.append(_pcase(f'win{len(shape)}d_m{m}', img, c, m, 0.5, r))
  for m in (1, 2, 3):
    surfs = []
    for d in (m, m + 1):
      for second in (5.0, 4.0):
        for axis in (0, 1):
          s = np.zeros((16, 18), f32)
          s[6, 7] = 5.0
          s[(6 + d, 7) if axis == 0 else (6, 7 + d)] = second
          s[14, 2] = 3.0
          surfs.append(s)
    cases.append(_pcase(f'pair_m{m}', np.stack(surfs), (8, 9), m, 0.5, 2))
    vol = np.zeros((4, 7, 12, 12), f32)
    vol[:, 3, 5, 5] = 5.0
    vol[0, 3 + m, 5, 5] = 5.0
    vol[1, 3, 5, 5 + m + 1] = 4.0
    vol[2, 3 - m, 5 - m, 5 - m] = 4.0
    vol[3, 3, 5 + m, 5] = 5.0
    vol[:, 6, 11, 11] = 3.0
    cases.append(_pcase(f'pair3d_m{m}', vol, (3, 6, 6), m, 0.5, 1))
  s = np.zeros((2, 16, 18), f32)
  s[0, 4:7, 5:9] = 2.0      # plateau: every element of it is a peak
  s[0, 12, 12] = 1.5
  s[1, 0:2, 0:3] = 2.0      # plateau in the corner: flat index 0 is a peak
  s[1, 9, 9] = 2.0
  cases.append(_pcase('plateau', s, (8, 9), 2, 0.5, 5))
  s = np.full((3, 12, 13), -1.0, f32)
  s[:, 1:-1, 1:-1] = 0.25
  s[0, 5, 6] = 1.0
  s[1, 0, 4] = -0.5         # largest of its in-surface window, below the padding's 0
  s[1, 6, 6] = 1.0
  s[2, 0, 0] = 1.0          # a positive corner is a peak
  s[2, 11, 12] = 0.75
  cases.append(_pcase('negative_border', s, (6, 6), 2, 0.5, 5))
  return cases


def peaks_threshold_cases():
  """Elements on the float32 product threshold_rel x max and an ulp or two
  either side ('>' is strict); threshold_rel 0 and 1; all-negative, all-zero
  and constant positive surfaces (the last overflows the candidate list at
  50 x 50)."""
  cases = []
  for t, top in ((0.3, 1.7), (0.5, 3.0), (0.7, 1.1)):
    vals = around(f32(t) * f32(top))
    s = np.zeros((len(vals), 14, 15), f32)
    s[:, 3, 4] = top
    for n, v in enumerate(vals):
      s[n, 10, 11] = v
    cases.append(_pcase(f'thr_{t}', s, (7, 7), 2, t, 2))
  rng = np.random.default_rng(7)
  img = rng.random((3, 14, 15)).astype(f32)
  img[2] -= 0.5
  for t in (0.0, 1.0):
    cases.append(_pcase(f'thr_rel_{t}', img, (7, 7), 2, t, 2))
  for shape in ((8, 9), (50, 50)):
    name = 'x'.join(map(str, shape))
    for t in (0.0, 0.5):
      cases.append(_pcase(f'negative_{name}_t{t}', -1 - rng.random((2,) + shape), (4, 4), 2, t, 3))
      cases.append(_pcase(f'zero_{name}_t{t}', np.zeros((2,) + shape), (4, 4), 2, t, 3))
      cases.append(_pcase(f'constant_{name}_t{t}', np.full((5,) + shape, 2.5), (4, 4), 2, t, 3))
  return cases


def peaks_special_cases():
  """NaN and infinities, each on a 40 x 37 surface (one workgroup per surface)
  and on 512 x 512 (multi-workgroup first pass)."""
  cases = []
  for shape in ((40, 37), (512, 512)):
    h, w = shape
    tag = f'{h}x{w}'
    p, q, far = (h // 2, w // 2), (h // 3, w // 4), (h - 3, w - 4)

    def base(n):
      s = np.full((n,) + shape, 0.125, f32)
      s[:, p[0], p[1]] = 4.0
      s[:, q[0], q[1]] = 2.5
      return s

    # a NaN row's first-peak index is 0: struck from surface 1, whose second peak
    # is at 0 (only candidate), and from surface 2 (a third, smaller one remains)
    s = base(4)
    s[0, far[0], far[1]] = np.nan
    s[1, q[0], q[1]] = 0.125
    s[1, 0, 0] = 3.0
    s[2, 0, 0] = 3.0
    cases.append(_pcase(f'nan_couples_{tag}', s, p, 2, 0.5, 5))
    # NaN next to the first peak, NaN far from every peak window, negative NaN
    s = base(4)
    s[0, p[0], p[1] + 1] = np.nan
    s[1, far[0], far[1]] = np.nan
    s[2, far[0], far[1]] = -np.nan
    s[2].flat[1] = np.nan
    cases.append(_pcase(f'nan_places_{tag}', s, p, 2, 0.5, 5))
    for t in (0.5, 0.0):
      s = base(3)
      s[1, far[0], far[1]] = np.inf
      s[2, p[0], p[1]] = np.inf
      cases.append(_pcase(f'posinf_{tag}_t{t}', s, p, 2, t, 5))
    # -inf: far away, inside the sharpness window (-0.0), next to the peak, all over
    s = base(4)
    s[0, far[0], far[1]] = -np.inf
    s[1, p[0] + 3, p[1] - 2] = -np.inf
    s[2, p[0], p[1] - 1] = -np.inf
    s[2, q[0] + 1, q[1]] = -np.inf
    s[3] = -np.inf
    cases.append(_pcase(f'neginf_{tag}', s, p, 2, 0.5, 5))
    # window minimum exactly 0 (+0 and -0: sharpness +inf, -inf) and negative
    s = base(3)
    s[0, p[0] + 1, p[1] + 1] = 0.0
    s[1, p[0] + 1, p[1] + 1] = -0.0
    s[2, p[0] - 2, p[1] + 4] = -0.75
    cases.append(_pcase(f'window_min_{tag}', s, p, 2, 0.5, 5))
  return cases


def peaks_coupling_cases():
  """Batch coupling: a first-peak index of one surface is the best remaining
  candidate of another; index 0 a peak and struck, on the one-workgroup path;
  batches of 1, 4, 5 and 9 (one, exactly one, two and three second-pass
  workgroups) whose peaks sit on a shared lattice, so indices collide."""
  cases = []
  s = np.zeros((3, 20, 23), f32)
  s[0, 5, 5] = 9.0          # A: first peak at (5, 5)
  s[0, 15, 15] = 3.0
  s[1, 12, 3] = 8.0         # B: first (12, 3), best remaining (5, 5) is struck
  s[1, 5, 5] = 7.0
  s[1, 17, 20] = 2.0
  s[2, 12, 3] = 1.0         # C: its own first peak (15, 15) is A's second
  s[2, 15, 15] = 6.0
  cases.append(_pcase('couple_first_second', s, (10, 11), 2, 0.1, 5))
  s = np.zeros((3, 20, 23), f32)
  s[0, 0, 0] = 5.0          # first peak at index 0: struck everywhere
  s[0, 9, 9] = 4.0
  s[1, 9, 9] = 6.0          # index 0 is the only other peak: read un-struck
  s[1, 0, 0] = 2.0
  s[2, 9, 9] = 6.0          # index 0 no peak: nothing left, ratio 0
  cases.append(_pcase('couple_index0', s, (10, 11), 2, 0.1, 5))
  for b in (1, 4, 5, 9):
    rng = np.random.default_rng(b)
    s = np.zeros((b, 20, 23), f32)
    for n in range(b):
      k = rng.integers(2, 6)
      ys, xs = rng.integers(0, 4, k) * 6, rng.integers(0, 4, k) * 7
      s[n, ys, xs] = rng.permutation(16)[:k] + 4.0
    cases.append(_pcase(f'couple_batch{b}', s, (10, 11), 2, 0.1, 5))
  return cases


def peaks_sharpness_cases():
  """The sharpness window: exactly the surface, anisotropic, radius 0, the
  peak in every corner (the window shifts inward), and surfaces smaller than
  the window on one axis (no oracle: peaks64's clipped window is the rule)."""
  cases = []
  rng = np.random.default_rng(11)

  def corners(shape):
    s = (rng.random((2 ** len(shape),) + shape) - 0.25).astype(f32)
    for n, c in enumerate(itertools.product(*[(0, a - 1) for a in shape])):
      s[(n,) + c] = 3.0 + n / 8.0
    return s

  cases.append(_pcase('sharp_exact', corners((11, 11)), (5, 5), 2, 0.5, 5))
  cases.append(_pcase('sharp_aniso', corners((13, 15)), (6, 7), 2, 0.5, (5, 3)))
  cases.append(_pcase('sharp_aniso3d', corners((6, 9, 10)), (3, 4, 5), 1, 0.5, (1, 2, 2)))
  cases.append(_pcase('sharp_r0', corners((13, 15)), (6, 7), 2, 0.5, 0))
  cases.append(_pcase('sharp_r0_3d', corners((6, 9, 10)), (3, 4, 5), 2, 0.5, (0, 0, 0)))
  cases.append(_pcase('sharp_small_y', corners((9, 11)), (4, 5), 2, 0.5, 5, oracle=False))
  cases.append(_pcase('sharp_small_x', corners((11, 9)), (5, 4), 2, 0.5, 5, oracle=False))
  cases.append(_pcase('sharp_small_z', corners((7, 20, 20)), (3, 10, 10), 2, 0.5, 5, oracle=False))
  return cases


PEAKS_CASE_GROUPS = dict(capacity=peaks_capacity_cases, sweep=peaks_sweep_cases,
                         window=peaks_window_cases, threshold=peaks_threshold_cases,
                         special=peaks_special_cases, coupling=peaks_coupling_cases,
                         sharpness=peaks_sharpness_cases)


# ---------------------------------------------------------------------------
# warp.ndimage_warp (warp.py:189-335): cases.  The reference of these is
# oracle.warp_oracle.ndimage_warp, i.e. scipy.ndimage.map_coordinates itself.
# ---------------------------------------------------------------------------
NDWARP_DTYPES = (np.uint8, np.uint16, f32)


def _wcase(name, image, cmap, stride, order, boxes=None, scale=None):
  image = np.ascontiguousarray(image)
  cmap = np.ascontiguousarray(cmap, f32)
  image.setflags(write=False)
  cmap.setflags(write=False)
  return dict(name=name, image=image, cmap=cmap, stride=tuple(stride), order=order,
              boxes=boxes, scale=scale)


def _image(rng, shape, dtype):
  """Random image without zeros (a voxel the warp blanks is then visible)."""
  if dtype == f32:
    return (rng.random(shape) * 100 + 1).astype(f32)
  return rng.integers(1, np.iinfo(dtype).max, shape, endpoint=True).astype(dtype)


def _all(name, rng, shape, cmap, stride, **kw):
  """One case per image type and order."""
  return [_wcase(f'{name}_{np.dtype(t).name}_o{order}', _image(rng, shape, t), cmap, stride,
                 order, **kw) for t in NDWARP_DTYPES for order in (0, 1)]


def ndwarp_nonfinite_map(dim, kind):
  """(clean map, map with non-finite nodes, image shape, stride): 5 x 6 (x 4 in
  3-D) nodes, stride 4, so that the image ends inside the last cell."""
  rng = np.random.default_rng(300 + dim)
  nodes = (5, 6) if dim == 2 else (4, 5, 6)
  shape = tuple(4 * (n - 1) for n in nodes)
  clean = smooth(rng, (dim,) + nodes, 1.5).astype(f32)
  bad = clean.copy()
  mid = tuple(n // 2 for n in nodes)
  if kind == 'nan_node':
    bad[(slice(None),) + mid] = np.nan
  elif kind == 'nan_one_channel':
    bad[(0,) + mid] = np.nan
  elif kind == 'nan_block':
    bad[(slice(None),) + tuple(slice(m - 1, m + 1) for m in mid)] = np.nan
  elif kind == 'nan_border':
    bad[(slice(None),) + (0,) + mid[1:]] = np.nan           # first row / plane, not a corner
    bad[(slice(None),) + tuple(n - 1 for n in nodes)] = np.nan  # the far corner
  elif kind == 'posinf':
    bad[(slice(None),) + mid] = np.inf
  elif kind == 'neginf':
    bad[(slice(None),) + mid] = -np.inf
  elif kind == 'mixed':
    bad[(0,) + mid] = np.inf
    bad[(1,) + mid] = -np.inf
    bad[(slice(None),) + tuple(m - 1 for m in mid)] = np.nan
  else:
    raise ValueError(kind)
  return clean, bad, shape, (4,) * dim


NDWARP_NONFINITE_KINDS = ('nan_node', 'nan_one_channel', 'nan_block', 'nan_border', 'posinf',
                          'neginf', 'mixed')


def ndwarp_nonfinite_cases():
  """NaN / +-inf map nodes: the output is 0 wherever the dense coordinate is not
  finite (a NaN tap poisons it whatever its weight)."""
  cases = []
  for dim in (2, 3):
    for kind in NDWARP_NONFINITE_KINDS:
      _, bad, shape, stride = ndwarp_nonfinite_map(dim, kind)
      cases += _all(f'{kind}_{dim}d', np.random.default_rng(dim), shape, bad, stride)
  return cases


def ndwarp_edge_tap_cases():
  """The tap beyond the last sample has weight 0 and is read mirrored, from
  len - 2: a non-finite value there makes the sum NaN.
  'map_hi': NaN along node index m - 2 of one axis, stride 4, the output's last
  row exactly on node m - 1 (dense coordinate NaN -> output 0).
  'img_hi': inf / NaN along image index len - 2 of one axis, zero relative map
  of stride 1 (dense coordinate = output index), order 1, float32.
  '*_lo': the mirror images at the lower edge (index 1, coordinate 0), where the
  in-range tap 1 is read."""
  cases = []
  for dim in (2, 3):
    nodes = (4, 5) if dim == 2 else (4, 4, 5)
    shape = tuple(4 * (n - 1) + 1 for n in nodes)
    for axis in range(dim):
      for side, at in (('hi', nodes[axis] - 2), ('lo', 1)):
        rng = np.random.default_rng(10 * dim + axis)
        cmap = smooth(rng, (dim,) + nodes, 1.0).astype(f32)
        cmap[(slice(None),) + (slice(None),) * axis + (at,)] = np.nan
        cases += _all(f'map_{side}_ax{axis}_{dim}d', rng, shape, cmap, (4,) * dim)
    shape = (6, 7) if dim == 2 else (4, 5, 6)
    for axis in range(dim):
      for side, at in (('hi', shape[axis] - 2), ('lo', 1)):
        for val in (np.inf, -np.inf, np.nan):
          img = _image(np.random.default_rng(axis), shape, f32)
          img[(slice(None),) * axis + (at,)] = val
          cases.append(_wcase(f'img_{side}_ax{axis}_{val}_{dim}d', img,
                              np.zeros((dim,) + shape, f32), (1,) * dim, 1))
  return cases


def ndwarp_boundary_targets(length):
  """Coordinates on and next to the limits of the range test and of order 0's
  rounding floor(c + 0.5), for an axis of `length` samples."""
  last = f32(length - 1)
  t = [f32(0.0), f32(-0.0), np.nextafter(f32(0), f32(-1)), -np.finfo(f32).tiny, f32(-1e-3),
       last, np.nextafter(last, f32(np.inf)), np.nextafter(last, f32(0))]
  for k in (0, 2, length - 2):
    t += around(k + 0.5)
  return np.array(t, f32)


def ndwarp_boundary_cases():
  """Stride-1 map the size of the image whose relative values put the absolute
  coordinate of one axis exactly on the targets above (in row 0 of that axis,
  where relative = absolute; the other rows get as close as float32 allows),
  the others on the voxel's own index."""
  cases = []
  length = 6
  targets = ndwarp_boundary_targets(length)
  for dim in (2, 3):
    for axis in range(dim):
      other = (axis + 1) % dim       # the targets vary along this axis
      shape = [3] * dim
      shape[axis], shape[other] = length, len(targets)
      cmap = np.zeros((dim,) + tuple(shape), f32)
      idx = np.arange(length, dtype=np.float64)
      rel = targets[np.newaxis, :].astype(np.float64) - idx[:, np.newaxis]   # [axis, other]
      rel = np.moveaxis(rel.reshape((length, len(targets)) + (1,) * (dim - 2)),
                        (0, 1), (axis, other)) if dim == 3 else (rel if axis == 0 else rel.T)
      cmap[dim - 1 - axis] = np.broadcast_to(rel, shape)   # channels are x, y[, z]
      cases += _all(f'boundary_ax{axis}_{dim}d', np.random.default_rng(axis), tuple(shape), cmap,
                    (1,) * dim)
  return cases


def ndwarp_rounding_cases():
  """Conversion to integer pixels: order 1 between the pixel pairs (0, 1),
  (254, 255) and (65534, 65535) at t = 0.5 (the value k + 0.5 goes up) and at
  the float32 below 0.5 (it stays)."""
  cases = []
  below = np.nextafter(f32(0.5), f32(0))
  for dtype, pairs in ((np.uint8, ((0, 1), (254, 255))), (np.uint16, ((0, 1), (254, 255), (65534, 65535))),
                       (f32, ((0, 1),))):
    for lo, hi in pairs:
      for dim in (2, 3):
        img = np.zeros((2,) * dim, dtype)
        img[..., 0], img[..., 1] = lo, hi
        cmap = np.zeros((dim,) + (2,) * dim, f32)
        cmap[0, ..., 0, 0] = 0.5      # x of the nodes (.., 0, 0) and (.., 1, 0)
        cmap[0, ..., 1, 0] = below
        for order in (0, 1):
          cases.append(_wcase(f'round_{np.dtype(dtype).name}_{lo}_{dim}d_o{order}', img, cmap,
                              (1,) * dim, order))
  return cases


def ndwarp_shape_cases():
  """Degenerate and awkward shapes, boxes, scales and strides."""
  cases = []
  rng = np.random.default_rng(77)
  field = lambda shape, amp: smooth(rng, shape, amp).astype(f32)
  # a single node on one axis: only output index 0 of that axis is inside the map
  cases += _all('one_node_y', rng, (9, 12), field((2, 1, 4), 1.0), (4, 4))
  cases += _all('one_node_x', rng, (9, 12), field((2, 3, 1), 1.0), (4, 4))
  cases += _all('one_node_z', rng, (3, 9, 8), field((3, 1, 3, 3), 1.0), (2, 4, 4))
  # (an axis of one sample is hit by the coordinate 0 alone: zero relative map there)
  cmap = field((3, 1, 3, 4), 1.0)
  cmap[2] = 0
  cases += _all('one_section', rng, (1, 9, 10), cmap, (1, 4, 3))
  cases += _all('image_1x1', rng, (1, 1), np.zeros((2, 1, 1)), (1, 1))
  cmap = field((2, 2, 2), 0.4)
  cmap[:, 0, 0] = 0
  cases += _all('image_1x1_map', rng, (1, 1), cmap, (4, 4))
  cases += _all('image_1x1x1', rng, (1, 1, 1), np.zeros((3, 2, 2, 2)), (2, 2, 2))
  # output voxel counts around the workgroup size and a few workgroups
  for shape in ((15, 17), (16, 16), (1, 257), (257, 1), (30, 41), (3, 9, 11)):
    nodes = tuple(max(2, (a + 3) // 4 + 1) for a in shape)
    cmap = field((len(shape),) + nodes, 2.0)
    for axis, a in enumerate(shape):
      if a == 1:
        cmap[len(shape) - 1 - axis] = 0
    cases += _all('count_' + 'x'.join(map(str, shape)), rng, shape, cmap, (4,) * len(shape))
  # output beyond the last node: the dense coordinate is 0 there and the image is
  # sampled at its origin (the reference's behaviour, kept)
  cases += _all('beyond_2d', rng, (20, 24), field((2, 3, 3), 2.0), (6, 6))
  cases += _all('beyond_3d', rng, (8, 14, 15), field((3, 2, 3, 3), 1.0), (3, 4, 4))
  # fractional strides, out_scale per axis
  cases += _all('frac_stride_2d', rng, (21, 26), field((2, 9, 9), 2.0), (2.5, 3.25))
  cases += _all('frac_stride_3d', rng, (7, 13, 14), field((3, 6, 6, 6), 1.0), (1.5, 2.75, 3.125))
  cases += _all('scale_2d', rng, (24, 28), field((2, 7, 8), 2.0), (4, 4), scale=(1.5, 0.75))
  # boxes (xyz start, size) with non-zero and negative starts; the map has context
  # around the output box, the output box lies inside the image box
  img_shape, cmap = (8, 22, 26), field((3, 4, 5, 6), 1.5)
  boxes = dict(image=((-12, 200, 10), (26, 22, 8)), map=((-3, 33, 3), (6, 5, 4)),
               out=((-10, 203, 11), (20, 18, 6)))
  cases += _all('boxes', rng, img_shape, cmap, (3, 6, 6), boxes=boxes, scale=(1.0, 1.0, 1.0))
  boxes = dict(image=((-24, 100, -4), (26, 22, 8)), map=((-3, 33, -1), (6, 5, 4)),
               out=((-10, 201, -1), (12, 16, 5)))
  cases += _all('boxes_scale', rng, img_shape, cmap, (3, 6, 6), boxes=boxes,
                scale=(2.0, 0.5, 1.0))
  return cases


NDWARP_CASE_GROUPS = dict(nonfinite=ndwarp_nonfinite_cases, edge_tap=ndwarp_edge_tap_cases,
                          boundary=ndwarp_boundary_cases, rounding=ndwarp_rounding_cases,
                          shapes=ndwarp_shape_cases)


def ndwarp_oracle_args(case):
  """Keyword arguments of oracle.warp_oracle.ndimage_warp for a case."""
  kw = dict(order=case['order'])
  if case['boxes'] is not None:
    b = case['boxes']
    kw.update(image_start=np.array(b['image'][0]), map_start=np.array(b['map'][0]),
              out_start=np.array(b['out'][0]), out_size=np.array(b['out'][1]))
  if case['scale'] is not None:
    kw['out_scale'] = case['scale']
  return kw
