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
