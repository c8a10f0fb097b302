"""The exact masked-correlation reference, its checker and its case list (CPU).

tests/masked_exact_ref.py is what the GPU tests of the masked kernels trust, so
it is pinned here: the sums against an int64 direct correlation, the surface
against the float64 direct oracle, the conditions that keep the case list and
the checker honest, the measured float32 constants, and the checker's own
sensitivity to the errors it exists to find.
"""
import numpy as np
import pytest
import scipy.signal

from oracle import flow_oracle
from tests import masked_exact_ref as ref

ALL = ref.case_names()


def _direct_i64(a, b):
  return np.stack([scipy.signal.correlate(x, y, mode='full', method='direct')
                   for x, y in zip(a.astype(np.int64), b.astype(np.int64))])


@pytest.mark.parametrize('P,Q', [((7, 9), (5, 6)), ((12, 3), (12, 3)), ((3, 4, 5), (2, 4, 3))])
def test_sums_equal_the_int64_direct_correlation(P, Q):
  rng = np.random.default_rng(sum(P))
  dim = len(P)
  a = rng.integers(0, 256, (3,) + P)
  b = rng.integers(0, 256, (3,) + Q)
  a[0].flat[:4] = (0, 255, 255, 0)
  pm = rng.random(a.shape) < 0.3
  cm = rng.random(b.shape) < 0.2
  pm[1] = True                       # a patch without a valid pixel
  t = ref.terms(a, b, pm, cm, dim)
  va, vb = (~pm).astype(np.int64), (~cm).astype(np.int64)
  a0, b0 = a * va, b * vb
  for key, x, y in (('n', va, vb), ('sa', a0, vb), ('sb', va, b0), ('sab', a0, b0),
                    ('saa', a0 * a0, vb), ('sbb', va, b0 * b0)):
    np.testing.assert_array_equal(t[key], _direct_i64(x, y), err_msg=key)
  assert t['n'].dtype == np.int64
  assert (t['n_ov'][1] == ref.EPS32).all() and (t['den'][1] == 0).all()
  # the same quantity whatever constant the valid pixels are shifted by
  t2 = ref.terms(a + 100, b + 3, pm, cm, dim)
  live = t['n'] > 1
  np.testing.assert_allclose(t2['den'][live], t['den'][live], rtol=1e-12, atol=1e-9)
  np.testing.assert_allclose(t2['num'][live], t['num'][live], rtol=1e-12, atol=1e-9)


# (the direct oracle costs surface x patch operations: the cases below are the
# small ones of every kind)
@pytest.mark.parametrize('name', ['geo_20x48_20x48', 'geo_33x3_20x2', 'faint_50x46_37x31',
                                  'batch_of_1', 'vol_5x7x12'])
def test_want_equals_the_float64_direct_oracle(name):
  c = ref.case(name)
  cls = c.classify(ref.BAND_MFMA)
  b = len(c.prev)
  g = c.group or b
  got = np.concatenate([
      flow_oracle.xcorr_surface_direct(c.prev[lo:lo + g], c.curr[lo:lo + g], c.pm[lo:lo + g],
                                       c.cm[lo:lo + g], dim=c.dim) for lo in range(0, b, g)])
  # the oracle forms 0.3 * max in float64: elements exactly at the float32 product
  # are decided by the rounding this helper exists to pin, and left out here
  tie = cls['n_ov'] == np.rint(cls['thr'])
  decided = ~cls['undecided'] & ~tie
  assert decided.mean() > 0.9
  np.testing.assert_allclose(got[decided], cls['want'][decided], rtol=0, atol=2e-7)
  assert ((got == 0) == (cls['want'] == 0))[decided & (cls['uncut'] != 0)].all()


def test_overlap_threshold_is_the_float32_product():
  f = np.float32
  assert f(0.3) * f(1700) > 510 and f(0.3) * f(1680) > 504 and f(0.3) * f(2000) == 600
  for name, kept in (('tie_34x50', False), ('tie_40x50', True), ('tie_40x42', False)):
    c = ref.case(name)
    cls = c.classify(ref.BAND_MFMA)
    py, px = c.P
    assert cls['n_ov'].max() == py * px            # the clean patch fixes the maximum
    at = cls['n_ov'] == c.tie[0]
    assert at.sum() >= 4
    assert (cls['cut_ov'][at] != kept).all()
    if kept:
      assert (np.abs(cls['want'][at]) > ref.ATOL_MFMA).sum() >= 4
  # 40 x 42: the rows dy = +-28 reach 12 x 42 = 504 at most and are dead as a whole
  cls = ref.case('tie_40x42').classify(ref.BAND_MFMA)
  for ky in (39 - 28, 39 + 28):
    assert cls['n_ov'][0, ky].max() == 504 and cls['cut_ov'][:, ky].all()
    assert not cls['cut_ov'][0, ky + (1 if ky < 39 else -1)].all()


def test_case_list_holds_what_it_promises():
  names = set(ALL)
  assert len(names) == len(ALL)
  for g in ref.GEOMETRIES:
    assert 'geo_%dx%d_%dx%d' % g in names
  for c in ref.cases():
    if c.kind in ('geometry', 'faint', 'tie', 'flat'):
      # one patch of every assembly class, one patch with pixels 0 and 255
      p_any = c.pm.reshape(len(c.pm), -1).any(1)
      c_any = c.cm.reshape(len(c.cm), -1).any(1)
      assert {(bool(p), bool(q)) for p, q in zip(p_any, c_any)} == {
          (False, False), (True, False), (False, True), (True, True)}, c.name
      assert any((c.prev[k][~c.pm[k]] == 0).any() and (c.prev[k][~c.pm[k]] == 255).any()
                 for k in range(len(c.prev))), c.name
  g = ref.case('groups_4_by_2')
  assert (g.prev[1] == g.prev[2]).all() and (g.curr[1] == g.curr[2]).all()
  assert (g.pm[1] == g.pm[2]).all() and (g.cm[1] == g.cm[2]).all()
  for name in ('groups_4_by_2', 'groups_5_by_2'):
    cls = ref.case(name).classify(ref.BAND_MFMA)
    # the same faint patch: cut in group 0 (beside the textured patch), whole in group 1
    assert (cls['cut_tol'][1] & cls['live'][1]).sum() > 100
    assert not (cls['cut_tol'][2:] & cls['live'][2:]).any()
    assert (cls['uncut'][1] == cls['uncut'][2]).all()
  assert ref.case('all_fully_masked').classify(ref.BAND_MFMA)['want'].any() == False  # noqa: E712
  assert len(ref.case('batch_of_1').prev) == 1


@pytest.mark.parametrize('name', ALL)
def test_case_conditions(name):
  """Caps that keep the checker honest, from the reference alone."""
  c = ref.case(name)
  cls = c.classify(ref.BAND_MFMA)
  live = cls['live']
  kept = ~(cls['cut_ov'] | cls['cut_tol'])
  n_und = int(cls['undecided'].sum())
  print(name, 'undecided (matrix-core band)', n_und, 'live', int(live.sum()))
  assert n_und <= 8
  cls32 = c.classify(ref.BAND32)
  loose = cls32['undecided'] | (live & (cls32['den'] < 2 * cls32['tol']))
  print(name, 'undecided or below 2 tol (float32)', int(loose.sum()))
  if c.faint:
    # a faint patch straddles tol by design, so a share cap cannot hold for its
    # case; instead every such element belongs to a faint patch: the other
    # patches of the batch are checked element by element on the float32 paths too
    others = [k for k in range(len(c.prev)) if k not in c.faint and c.kind != 'groups']
    if c.kind == 'groups':
      others = [0]
    assert not loose[others].any()
  elif name not in ref.FLAT_EXEMPT:
    assert loose.sum() <= 0.01 * live.sum()
  if kept.any():
    assert (np.abs(cls['want'][kept]) > 10 * ref.ATOL_MFMA).mean() >= 0.5
    assert (np.abs(cls['want'][kept]) > 10 * ref.ATOL32).mean() >= 0.5
  else:
    assert name == 'all_fully_masked'
  if c.kind in ('faint', 'groups'):
    k = c.faint[0]
    below = (live[k] & cls['cut_tol'][k]).sum()
    assert 0.1 * live[k].sum() <= below <= 0.9 * live[k].sum()
  if c.kind == 'faint_only':
    assert not (live & cls['cut_tol']).any()       # nothing is cut
  if name == 'flat':
    assert (cls['den'][3] == 0).all()
  if name == 'half_flat':
    z = cls['den'][3][live[3]] == 0
    assert 0 < z.sum() < z.size
  if c.tie:
    assert (cls['n_ov'] == c.tie[0]).sum() >= 4


def test_float32_constants_cover_the_reference_float32_form():
  """ATOL32 / BAND32 against flow_oracle.xcorr_surface(dtype=float32), the
  reference's own float32 form -- never against a kernel."""
  dev = flip = 0.0
  for c in ref.cases():
    d, f, n = ref.measure_float32(c)
    print(c.name, 'deviation %.3g' % d, 'differently decided', n, 'at %.3g of tol' % f)
    dev, flip = max(dev, d), max(flip, f)
  print('largest deviation %.3g, largest distance of a differently decided element %.3g'
        % (dev, flip))
  assert ref.ATOL32 >= max(4 * dev, 5e-5)
  assert ref.BAND32 >= 4 * flip
  assert ref.ATOL32 <= max(4 * ref.MEASURED_DEV32, 5e-5)   # and no wider than measured
  assert ref.BAND32 <= max(4 * ref.MEASURED_FLIP32, ref.BAND_MFMA)
  assert ref.BAND32 < 1e-3
  # the float32 form passes the float32 check on every case
  for c in ref.cases():
    ref.check(ref.float32_form(c), c.classify(ref.BAND32), ref.ATOL32, exact_zero_den=False)


def test_matrix_core_constants_are_the_documented_bound():
  assert ref.BAND_MFMA == 4 * 2.0 ** -20 and ref.ATOL_MFMA == 2 * 2.0 ** -20


def _pick(mask, n=1):
  idx = np.argwhere(mask)
  assert len(idx) >= n
  return [tuple(i) for i in idx[:: max(1, len(idx) // n)][:n]]


@pytest.mark.parametrize('name', ['geo_96x48_96x48', 'faint_48x48_48x48', 'tie_34x50',
                                  'tie_40x50'])
def test_checker_raises_on_every_kind_of_error(name):
  c = ref.case(name)
  cls = c.classify(ref.BAND_MFMA)
  want = cls['want'].astype(np.float32)
  atol = ref.ATOL_MFMA
  ref.check(want, cls, atol)
  ref.check(cls['want'], cls, atol)
  kept = ~(cls['cut_ov'] | cls['cut_tol']) & ~cls['undecided']
  cut = (cls['cut_ov'] | cls['cut_tol']) & ~cls['undecided']

  def must_raise(bad):
    with pytest.raises(AssertionError, match='elements wrong'):
      ref.check(bad, cls, atol)

  # one kept element set to 0
  for i in _pick(kept & (np.abs(cls['want']) > 2 * atol), 3):
    bad = want.copy()
    bad[i] = 0
    must_raise(bad)
  # one cut element set to 1e-3: cut by the overlap, and cut by the tolerance
  for m in (cls['cut_ov'], cut & ~cls['cut_ov']):
    if m.any():
      bad = want.copy()
      bad[_pick(m)[0]] = 1e-3
      must_raise(bad)
  assert name != 'faint_48x48_48x48' or (cut & ~cls['cut_ov']).any()
  # a 16-element row segment shifted by one
  k, y, x = _pick(kept & (np.abs(cls['want']) > 0.05), 2)[-1]
  x = min(max(x, 1), want.shape[2] - 17)
  bad = want.copy()
  bad[k, y, x:x + 16] = want[k, y, x - 1:x + 15]
  assert np.abs(bad - want).max() > 2 * atol
  must_raise(bad)
  # one value off by 3 atol
  for sign in (1, -1):
    bad = want.copy()
    i = _pick(kept & (np.abs(cls['want']) < 0.9))[0]
    bad[i] += sign * 3 * atol
    must_raise(bad)
  # one NaN, one infinity, one value outside [-1, 1]
  for v in (np.nan, np.inf, 1.0001):
    bad = want.copy()
    bad[_pick(kept)[0]] = v
    must_raise(bad)
    bad = want.copy()
    bad[_pick(cls['cut_ov'])[0]] = v
    must_raise(bad)
    with pytest.raises(AssertionError):
      ref.check(bad, c.classify(ref.BAND32), ref.ATOL32, exact_zero_den=False)
  # one tie element on the wrong side
  if c.tie:
    at = cls['n_ov'] == c.tie[0]
    for i in _pick(at & (np.abs(cls['uncut']) > 2 * atol), 2):
      bad = want.copy()
      bad[i] = 0 if want[i] != 0 else cls['uncut'][i]
      must_raise(bad)


def test_checker_accepts_either_side_only_where_undecided():
  """A wide band makes elements undecided: there 0 and the uncut value both pass,
  anything else fails; outside the band nothing changes."""
  c = ref.case('faint_48x48_48x48')
  cls = c.classify(0.05)
  und = cls['undecided']
  assert und.sum() > 50 and (und & cls['cut_tol']).any() and (und & ~cls['cut_tol']).any()
  for fill in (0.0, None):
    got = cls['want'].copy()
    got[und] = 0.0 if fill is not None else cls['uncut'][und]
    ref.check(got, cls, ref.ATOL_MFMA)
  got = cls['want'].copy()
  i = _pick(und & (np.abs(cls['uncut']) > 0.01))[0]
  got[i] = 0.5 * cls['uncut'][i]
  with pytest.raises(AssertionError):
    ref.check(got, cls, ref.ATOL_MFMA)
  # the float32 form of the check lets the elements below 2 tol go, nothing else
  cls32 = c.classify(ref.BAND32)
  got = cls32['want'].copy()
  low = cls32['live'] & (cls32['den'] < 2 * cls32['tol'])
  got[low] = 0.3
  ref.check(got, cls32, ref.ATOL32, exact_zero_den=False)
  with pytest.raises(AssertionError):
    ref.check(got, cls32, ref.ATOL32)
  got[_pick(cls32['live'] & ~low)[0]] += 4 * ref.ATOL32
  with pytest.raises(AssertionError):
    ref.check(got, cls32, ref.ATOL32, exact_zero_den=False)
