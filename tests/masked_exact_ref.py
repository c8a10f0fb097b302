"""Exact reference, element-wise checker and case list for the masked
(Padfield) correlation.  TEST INFRASTRUCTURE, CPU only.

The masked surface is a function of six sums over the overlap of a shift:
n, sum a, sum b, sum ab, sum a^2, sum b^2 (masked pixels left out).  For
integer-valued patches these are integers below 2^53, so a float64 FFT followed
by rint gives them exactly (`terms`); numerator, denominator and overlap follow
in float64 from differences of integers.  The quantity does not change when a
constant is subtracted from the valid pixels of a patch, so the device is called
with mean=None and no mean appears here.

The reference zeroes an element on two decisions that couple the patches of a
reference batch (group):  den <= tol, tol = 1e3 eps32 max(den), and
n_ov < float32(0.3) * float32(max n_ov).  The second has one answer (an integer
against an exact float32).  The first has one answer except within the rounding
of the implementation's den and tol: `classify` marks those elements `undecided`
(|den - tol| <= band tol) and `check` accepts either side there -- and ONLY there.
Every element is checked.
"""
from __future__ import annotations

import numpy as np
import scipy.fft
from scipy import ndimage

EPS32 = float(np.finfo(np.float32).eps)

# Matrix-core path (method 2).  Derived, not measured: the assembly documents a
# relative error below 2^-20 for its float denominator (padfield_terms).  The
# band is four times that (den and tol -- a maximum of such dens -- each carry
# it, with a factor 2 to spare); the atol is twice that (numerator / denominator
# of a value within [-1, 1]) plus the final float32 division, 2^-24, rounded up.
BAND_MFMA = 2.0 ** -18
ATOL_MFMA = 2.0 ** -19

# Float32 paths (direct kernel, FFT form).  Measured on the CPU against the
# reference's own float32 form, flow_oracle.xcorr_surface(dtype=np.float32) on the
# mean-subtracted patches, never against the kernels (tests/test_masked_exact_refs.py
# recomputes both and asserts that the constants still cover them):
#   largest |float32 form - want| on decided elements over the case list: see
#   MEASURED_DEV32; ATOL32 = max(4 x that, 5e-5), the factor 4 for the other
#   summation order (sequential fmaf against FFT);
#   largest |den - tol| / tol among elements where that form and `want` decide
#   differently (exact-zero den excluded): MEASURED_FLIP32; BAND32 = 4 x that.
#   measured: deviation 1.1e-6 (geo_33x3_20x2), so 4 x is 4.4e-6 and the 5e-5 floor
#   that tests/test_gpu_fft_own.py already uses holds; no element of any case is
#   decided differently by that form (one element of the whole list, in
#   faint_64x80_40x64, lies within 2^-18 of its tol at all), so 4 x is 0 and the
#   band keeps the matrix-core value as a floor.
MEASURED_DEV32 = 1.1e-6
MEASURED_FLIP32 = 0.0
ATOL32 = max(4 * MEASURED_DEV32, 5e-5)
BAND32 = max(4 * MEASURED_FLIP32, BAND_MFMA)


# ---------------------------------------------------------------------------
# the exact sums
# ---------------------------------------------------------------------------
def _corr(a, b, dim):
  """Full linear correlation over the last `dim` axes of integer-valued float64
  arrays, out[k] = sum_i a[i + k - (Q - 1)] b[i], as exact int64."""
  full = tuple(p + q - 1 for p, q in zip(a.shape[-dim:], b.shape[-dim:]))
  fast = tuple(scipy.fft.next_fast_len(n, real=True) for n in full)
  axes = tuple(range(-dim, 0))
  flip = (Ellipsis,) + (slice(None, None, -1),) * dim
  out = scipy.fft.irfftn(scipy.fft.rfftn(a, s=fast, axes=axes) *
                         scipy.fft.rfftn(b[flip], s=fast, axes=axes), s=fast, axes=axes)
  out = out[(Ellipsis,) + tuple(slice(0, n) for n in full)]
  r = np.rint(out)
  assert np.abs(out - r).max() < 0.25, 'FFT round-off too large for exact sums'
  return r.astype(np.int64)


def terms(prev, curr, pm, cm, dim=2):
  """The six exact sums per shift and, from them, num / den / n_ov in float64.

  prev, curr: integer-valued patches [b, *P], [b, *Q]; pm, cm: boolean masks of
  the same shapes (True = masked) or None.
  """
  a = np.asarray(prev).astype(np.float64)
  b = np.asarray(curr).astype(np.float64)
  assert (a == np.rint(a)).all() and (b == np.rint(b)).all()
  va = np.ones(a.shape) if pm is None else 1.0 - np.asarray(pm, np.float64)
  vb = np.ones(b.shape) if cm is None else 1.0 - np.asarray(cm, np.float64)
  a = a * va
  b = b * vb
  t = {
      'n': _corr(va, vb, dim), 'sa': _corr(a, vb, dim), 'sb': _corr(va, b, dim),
      'sab': _corr(a, b, dim), 'saa': _corr(a * a, vb, dim), 'sbb': _corr(va, b * b, dim),
  }
  n = t['n']
  # n * (the reference's terms): differences of int64 products, exact
  num_n = n * t['sab'] - t['sa'] * t['sb']
  pa_n = np.maximum(n * t['saa'] - t['sa'] ** 2, 0)
  pb_n = np.maximum(n * t['sbb'] - t['sb'] ** 2, 0)
  # the reference clamps the overlap with fmax(n, eps); where n == 0 every sum is 0
  nn = np.maximum(n.astype(np.float64), EPS32)
  t['n_ov'] = nn
  t['num'] = num_n.astype(np.float64) / nn
  t['den'] = np.sqrt(pa_n.astype(np.float64) * pb_n.astype(np.float64)) / nn
  return t


def classify(t, groups=None, band=BAND_MFMA):
  """want / uncut / undecided per element; maxima per reference batch of `groups`
  patches (None: the whole batch is one)."""
  num, den, n_ov = t['num'], t['den'], t['n_ov']
  b = num.shape[0]
  groups = b if not groups else int(groups)
  with np.errstate(divide='ignore', invalid='ignore'):
    uncut = np.where(den > 0, np.clip(num / np.where(den > 0, den, 1.0), -1.0, 1.0), 0.0)
  tol = np.empty_like(den)
  thr = np.empty_like(den)
  for lo in range(0, b, groups):
    sl = slice(lo, lo + groups)
    tol[sl] = 1e3 * EPS32 * den[sl].max()
    thr[sl] = float(np.float32(0.3) * np.float32(n_ov[sl].max()))
  cut_ov = n_ov < thr
  cut_tol = den <= tol
  want = np.where(cut_ov | cut_tol, 0.0, uncut)
  # (tol == 0: every den of the batch is exactly 0 and the cut is decided)
  undecided = (np.abs(den - tol) <= band * tol) & ~cut_ov & (tol > 0)
  return {'want': want, 'uncut': uncut, 'undecided': undecided, 'cut_ov': cut_ov,
          'cut_tol': cut_tol, 'den': den, 'tol': tol, 'thr': thr, 'n_ov': n_ov,
          'live': ~cut_ov}


def check(got, cls, atol, exact_zero_den=True):
  """Checks EVERY element of `got` against the classification; raises
  AssertionError naming the first offenders.

  exact_zero_den=False (float32 paths): live elements whose exact den is below
  2 tol only get the finite / range check -- there float32 round-off decides, in
  the reference as well.
  """
  got = np.asarray(got)
  want, uncut = cls['want'], cls['uncut']
  assert got.shape == want.shape, (got.shape, want.shape)
  g = got.astype(np.float64)
  fin = np.isfinite(g)
  ok_range = fin & (g >= -1.0) & (g <= 1.0)
  cut = cls['cut_ov'] | cls['cut_tol']
  und = cls['undecided']
  loose = np.zeros(want.shape, bool)
  if not exact_zero_den:
    loose = cls['live'] & (cls['den'] < 2 * cls['tol'])
  with np.errstate(invalid='ignore'):
    near_want = np.abs(g - want) <= atol
    near_uncut = np.abs(g - uncut) <= atol
  ok = np.where(loose, True,
                np.where(und, (g == 0.0) | near_uncut,
                         np.where(cut, g == 0.0, near_want)))
  bad = ~(ok & ok_range)
  if bad.any():
    idx = np.argwhere(bad)
    lines = []
    for i in idx[:6]:
      i = tuple(i)
      lines.append(f'{i}: got {got[i]!r} want {want[i]:.9g} uncut {uncut[i]:.9g} '
                   f'den/tol {cls["den"][i] / cls["tol"][i] if cls["tol"][i] else np.nan:.9g} '
                   f'n_ov {cls["n_ov"][i]:.9g} thr {cls["thr"][i]:.9g} '
                   f'cut_ov {bool(cls["cut_ov"][i])} undecided {bool(und[i])}')
    raise AssertionError(f'{int(bad.sum())} of {bad.size} elements wrong (atol {atol:.3g}):\n' +
                         '\n'.join(lines))


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
class Case:
  """One batch of patches.  group: patches per reference batch (None = all)."""

  def __init__(self, name, prev, curr, pm, cm, dim=2, group=None, kind='geometry',
               faint=(), tie=None, mfma=True):
    self.name, self.prev, self.curr, self.pm, self.cm = name, prev, curr, pm, cm
    self.dim, self.group, self.kind, self.faint, self.tie = dim, group, kind, tuple(faint), tie
    self.mfma = mfma
    self._terms = None
    self._cls = {}

  @property
  def P(self):
    return self.prev.shape[1:]

  @property
  def Q(self):
    return self.curr.shape[1:]

  def terms(self):
    if self._terms is None:
      self._terms = terms(self.prev, self.curr, self.pm, self.cm, self.dim)
    return self._terms

  def classify(self, band):
    if band not in self._cls:
      self._cls[band] = classify(self.terms(), self.group, band)
    return self._cls[band]

  def centred_f32(self):
    """The patches minus their own mean over the valid pixels, float32: the
    input of the reference's float32 form when the device runs with mean=None."""
    out = []
    for x, m in ((self.prev, self.pm), (self.curr, self.cm)):
      x64 = x.astype(np.float64)
      mu = np.zeros(len(x))
      for k in range(len(x)):
        v = x64[k][~m[k]]
        mu[k] = v.mean() if v.size else 0.0
      out.append((x64 - mu.reshape((-1,) + (1,) * self.dim)).astype(np.float32))
    return out


def _texture(rng, b, P, Q):
  """Smooth uint8 texture; the post patch is the pre patch moved by (1, -1)."""
  py, px = P
  qy, qx = Q
  base = ndimage.gaussian_filter(rng.standard_normal((b, py + 8, px + 8)), (0, 1.3, 1.3))
  base = ((base - base.min()) / (base.max() - base.min()) * 255).astype(np.uint8)
  oy, ox = (py - qy) // 2, (px - qx) // 2
  prev = np.ascontiguousarray(base[:, 4:4 + py, 4:4 + px])
  curr = np.ascontiguousarray(base[:, 5 + oy:5 + oy + qy, 3 + ox:3 + ox + qx])
  return prev, curr


def _class_masks(rng, b, P, Q, density):
  """Patch k is clean / pre masked / post masked / both masked for k % 4 =
  0 / 1 / 2 / 3: random pixels at `density` plus a fully masked corner block."""
  pm = np.zeros((b,) + tuple(P), bool)
  cm = np.zeros((b,) + tuple(Q), bool)
  for k in range(b):
    if k % 4 in (1, 3):
      pm[k] = rng.random(P) < density
      pm[k][tuple(slice(0, max(1, s // 3)) for s in P)] = True
    if k % 4 in (2, 3):
      cm[k] = rng.random(Q) < density
      cm[k][tuple(slice(s - max(1, s // 4), s) for s in Q)] = True
  return pm, cm


def _full_range(prev, curr, k):
  """Pixels 0 and 255 in patch k (a - centre = -128: the square split)."""
  # (away from the fully masked corner blocks of _class_masks)
  h, w = (prev.shape[2] + 1) // 2, (curr.shape[2] + 1) // 2
  prev[k, -1, -h:] = 0
  prev[k, -2, -h:] = 255
  curr[k, 0, :w] = 0
  curr[k, 1, :w] = 255


def _faint(rng, shape, amp):
  return (126 + rng.integers(0, amp, shape)).astype(np.uint8)


GEOMETRIES = [
    (20, 48, 20, 48),     # 3x4
    (18, 64, 18, 64),     # 4x5
    (17, 80, 12, 70),     # 5x6
    (20, 96, 20, 96),     # 6x7
    (16, 112, 16, 100),   # 7x8
    (19, 128, 19, 128),   # 8x9
    (20, 160, 20, 160),   # 10x11
    (50, 46, 37, 31),     # P != Q
    (33, 3, 20, 2),       # P != Q
    (96, 48, 96, 48),     # 191 rows: six 32-row assembly blocks, the last one ragged
    (160, 160, 160, 160),  # production shape, batch of 4
]
FAINT_SHAPES = [(48, 48, 48, 48), (50, 46, 37, 31), (64, 80, 40, 64)]
FAINT_SEEDS = [1, 1, 2]   # chosen so that the tolerance cut runs through the {126, 127} patch
FLAT_EXEMPT = ('flat', 'half_flat')   # exempt from the float32 share cap: the flat part is the point


def _geometry_case(i, g):
  py, px, qy, qx = g
  rng = np.random.default_rng(100 + i)
  prev, curr = _texture(rng, 4, (py, px), (qy, qx))
  pm, cm = _class_masks(rng, 4, (py, px), (qy, qx), 0.05 + 0.01 * (i % 11))
  _full_range(prev, curr, 1)
  return Case('geo_%dx%d_%dx%d' % g, prev, curr, pm, cm)


def _faint_case(i, g, amps=(2, 4, 7), textured=True, name=None):
  py, px, qy, qx = g
  rng = np.random.default_rng(200 + i)
  b = 4
  prev, curr = _texture(rng, b, (py, px), (qy, qx))
  pm, cm = _class_masks(rng, b, (py, px), (qy, qx), 0.1)
  # patch 3 (both masked) is the textured one; 0 (clean), 1, 2 are faint
  order = [0, 1, 2] if textured else [0, 1, 2, 3]
  for k, amp in zip(order, list(amps) + [amps[0]] * 4):
    prev[k] = _faint(rng, prev[k].shape, amp)
    curr[k] = _faint(rng, curr[k].shape, amp)
  if textured:
    _full_range(prev, curr, 3)
  return Case(name or 'faint_%dx%d_%dx%d' % g, prev, curr, pm, cm,
              kind='faint' if textured else 'faint_only', faint=order)


def _flat_case(half):
  rng = np.random.default_rng(300 + half)
  P = Q = (48, 48)
  prev, curr = _texture(rng, 4, P, Q)
  pm, cm = _class_masks(rng, 4, P, Q, 0.1)
  _full_range(prev, curr, 0)
  if half:
    prev[3, :, :24] = 90
    curr[3, :, :24] = 90
  else:
    prev[3] = 90
    curr[3] = 90
  return Case('half_flat' if half else 'flat', prev, curr, pm, cm, kind='flat')


def _tie_case(P, tie, cut):
  rng = np.random.default_rng(400 + P[0] + P[1])
  prev, curr = _texture(rng, 4, P, P)
  pm, cm = _class_masks(rng, 4, P, P, 0.08)
  _full_range(prev, curr, 2)
  return Case('tie_%dx%d' % P, prev, curr, pm, cm, kind='tie', tie=(tie, cut))


def _degenerate_cases():
  out = []
  rng = np.random.default_rng(500)
  P = Q = (48, 48)
  prev, curr = _texture(rng, 5, P, Q)
  pm, cm = _class_masks(rng, 5, P, Q, 0.1)
  _full_range(prev, curr, 1)
  pm[4] = True                      # patch 4: every pre pixel masked
  out.append(Case('one_fully_masked', prev, curr, pm, cm, kind='degenerate'))
  prev, curr = _texture(rng, 2, P, Q)
  out.append(Case('all_fully_masked', prev, curr, np.ones(prev.shape, bool),
                  np.ones(curr.shape, bool), kind='degenerate'))
  prev, curr = _texture(rng, 1, P, Q)
  pm = rng.random(prev.shape) < 0.1
  cm = rng.random(curr.shape) < 0.1
  pm[0, :16, :16] = True
  out.append(Case('batch_of_1', prev, curr, pm, cm, kind='degenerate'))
  return out


def _group_case(b, seed):
  """group = 2.  Group 0: textured + faint; group 1: the same faint patch + another
  faint one, so the patch cut in group 0 is not cut in group 1.  b = 5: a ragged
  last group of one faint patch."""
  rng = np.random.default_rng(seed)
  P = Q = (48, 48)
  prev, curr = _texture(rng, b, P, Q)
  pm = rng.random(prev.shape) < 0.1
  cm = rng.random(curr.shape) < 0.1
  pm[0, :16, :16] = True
  f = _faint(rng, (2,) + P, 2)
  for k in range(1, b):
    prev[k], curr[k] = f[0], f[1]
  prev[3], curr[3] = _faint(rng, P, 4), _faint(rng, P, 4)
  pm[2], cm[2] = pm[1], cm[1]
  if b > 4:
    pm[4], cm[4] = pm[1], cm[1]
  return Case('groups_%d_by_2' % b, prev, curr, pm, cm, group=2, kind='groups', faint=(1,))


def _volume_case(P, Q):
  rng = np.random.default_rng(700 + sum(P))
  b = 3
  prev = rng.integers(0, 256, (b,) + P).astype(np.uint8)
  curr = rng.integers(0, 256, (b,) + Q).astype(np.uint8)
  prev[1], curr[1] = _faint(rng, P, 2), _faint(rng, Q, 2)
  pm = rng.random(prev.shape) < 0.1
  cm = rng.random(curr.shape) < 0.1
  pm[0, :2, :3, :4] = True
  pm[2] = False
  return Case('vol_%dx%dx%d' % P, prev, curr, pm, cm, dim=3, kind='volume', faint=(1,),
              mfma=False)


_CASES = None


def cases():
  """The shared case list (built once; the arrays must not be modified)."""
  global _CASES
  if _CASES is None:
    cs = [_geometry_case(i, g) for i, g in enumerate(GEOMETRIES)]
    cs += [_faint_case(i, g) for i, g in zip(FAINT_SEEDS, FAINT_SHAPES)]
    cs += [_flat_case(0), _flat_case(1)]
    cs.append(_faint_case(9, (48, 48, 48, 48), amps=(2, 2, 2), textured=False,
                          name='faint_only'))
    # float32(0.3) * 1700 = 510.00003: overlap 510 is cut; * 2000 = 600.0: overlap
    # 600 is kept; * 1680 = 504.00003: the rows dy = +-28 (12 x 42 = 504) are dead
    cs += [_tie_case((34, 50), 510, True), _tie_case((40, 50), 600, False),
           _tie_case((40, 42), 504, True)]
    cs += _degenerate_cases()
    cs += [_group_case(4, 604), _group_case(5, 2605)]   # (seeds: the cut runs through patch 1)
    cs += [_volume_case((5, 7, 12), (5, 6, 11)), _volume_case((12, 20, 30), (12, 20, 30))]
    for c in cs:
      for arr in (c.prev, c.curr, c.pm, c.cm):
        arr.setflags(write=False)
    _CASES = cs
  return _CASES


def case_names(pred=lambda c: True):
  return [c.name for c in cases() if pred(c)]


def case(name):
  return next(c for c in cases() if c.name == name)


def float32_form(c):
  """The reference's float32 FFT form on the case, group by group."""
  from oracle import flow_oracle
  a0, b0 = c.centred_f32()
  b = len(a0)
  g = c.group or b
  return np.concatenate([
      flow_oracle.xcorr_surface(a0[lo:lo + g], b0[lo:lo + g], c.pm[lo:lo + g],
                                c.cm[lo:lo + g], dim=c.dim, dtype=np.float32)
      for lo in range(0, b, g)])


def measure_float32(c):
  """(largest |float32 form - want| on decided elements, largest |den - tol| / tol
  among elements on which that form and `want` decide differently; exact-zero den
  left out)."""
  cls = c.classify(0.0)
  o32 = float32_form(c).astype(np.float64)
  want, den, tol = cls['want'], cls['den'], cls['tol']
  # (an element whose exact numerator is 0 shows no decision through its value)
  flips = ((o32 == 0) != (want == 0)) & cls['live'] & (den > 0) & (cls['uncut'] != 0)
  with np.errstate(divide='ignore', invalid='ignore'):
    rel = np.where(tol > 0, np.abs(den - tol) / tol, 0.0)
  flip_rel = float(rel[flips].max()) if flips.any() else 0.0
  decided = ~flips & ~(cls['live'] & (den < 2 * tol))
  dev = float(np.abs(o32 - want)[decided].max()) if decided.any() else 0.0
  return dev, flip_rel, int(flips.sum())
