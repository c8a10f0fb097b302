"""The exact un-masked correlation reference, its bound and its case list (CPU).

tests/xcorr_exact_ref.py is what the element-wise GPU tests of the matrix-core
correlation trust, so it is pinned here: the integer sums against an int64 loop,
the exact surface against a float64 direct correlation, every float32 restatement
of an epilogue form against its derived bound (with the recorded ratios), the path
every case must take, the measured constant of the float direct kernel, and the
checker's sensitivity to the errors it exists to find.
"""
import numpy as np
import pytest

from tests import xcorr_exact_ref as ref

ALL = ref.case_names()


def _loop_sums(a, c):
  """sab, sa, sb, n per shift by plain int64 loops."""
  (py, px), (qy, qx) = a.shape, c.shape
  a, c = a.astype(np.int64), c.astype(np.int64)
  out = np.zeros((4, py + qy - 1, px + qx - 1), np.int64)
  for ky in range(py + qy - 1):
    for kx in range(px + qx - 1):
      dy, dx = ky - (qy - 1), kx - (qx - 1)
      for y in range(qy):
        for x in range(qx):
          if 0 <= y + dy < py and 0 <= x + dx < px:
            out[:, ky, kx] += (a[y + dy, x + dx] * c[y, x], a[y + dy, x + dx], c[y, x], 1)
  return out


@pytest.mark.parametrize('P,Q', [((5, 7), (3, 4)), ((4, 6), (4, 6)), ((3, 9), (1, 1))])
def test_sums_equal_a_plain_int64_loop(P, Q):
  rng = np.random.default_rng(sum(P) + sum(Q))
  a = rng.integers(0, 256, (2,) + P).astype(np.uint8)
  c = rng.integers(0, 256, (2,) + Q).astype(np.uint8)
  a[0].flat[:2] = (0, 255)
  t = ref.sums(a, c)
  for k in range(2):
    want = _loop_sums(a[k], c[k])
    for i, key in enumerate(('sab', 'sa', 'sb', 'n')):
      np.testing.assert_array_equal(t[key][k], want[i], err_msg=key)
      assert t[key].dtype == np.int64
  # the exact surface from them, against the definition in float64 (tiny: exact there)
  for mean in (None, 0.0, 117.5, -3.0):
    ex = ref.exact(a, c, mean, t)
    for k in range(2):
      mua = a[k].mean() if mean is None else mean
      muc = c[k].mean() if mean is None else mean
      w = _loop_sums(a[k], c[k]).astype(np.float64)
      want = w[0] - muc * w[1] - mua * w[2] + mua * muc * w[3]
      np.testing.assert_allclose(ex[k], want, rtol=0, atol=1e-9 * np.abs(w[0]).max())


def test_centre_rule():
  """Nearest integer to the mean (or the given one) that keeps pixel - c in int8."""
  x = np.zeros((5, 4, 4), np.uint8)
  x[0] = 200                       # constant: its own value
  x[1].flat[:] = np.arange(16)     # mean 7.5 -> rint to even: 8
  x[2].flat[:2] = (0, 255)         # 0 and 255: forced to 128
  x[3] += 250                      # given mean 0 -> clamped to mx - 127
  x[4] += 3
  c, mu32, mu_x = ref.centre(x, None)
  assert list(c[:3]) == [200, 8, 128]
  assert mu32[0] == 0 and mu32[1] == -0.5 and abs(mu_x[2] - (255 / 16 - 128)) < 1e-12
  c, mu32, mu_x = ref.centre(x, 0.0)
  assert list(c) == [73, 0, 128, 123, 0] and list(mu32) == [-73, 0, -128, -123, 0]
  c, mu32, _ = ref.centre(x, 1000.0)
  assert list(c) == [255, 128, 128, 255, 131] and mu32[4] == 869
  for mean in (None, 117.5, -3.0):
    c, _, _ = ref.centre(x, mean)
    d = x.astype(np.int64) - c[:, None, None]
    assert d.min() >= -128 and d.max() <= 127


def test_case_list_holds_what_it_promises():
  assert len(set(ALL)) == len(ALL)
  by_form = {}
  for c in ref.cases():
    by_form.setdefault(c.form, set()).add(c.variant)
  # every chunk geometry up to (10, 11) in the compile-time form, both search-window ones
  assert by_form['same_exact'] == set(ref.GEOMETRIES[:7])
  assert by_form['wide'] == {(15, 11), (20, 11)}
  assert {'same', 'general'} <= set(by_form)
  for c in ref.cases():
    if c.kind == 'mean':
      continue
    if c.kind in ('same_exact', 'same', 'general', 'wide'):
      assert c.form == c.kind and c.mean is None, c.name
      # textured, noise, and a pair with 0 and 255 whose centre is forced to 128
      ca, _, mua = ref.centre(c.a, None)
      if c.a[2].size > 1:
        assert c.a[2].min() == 0 and c.a[2].max() == 255 and ca[2] == 128 and abs(mua[2]) > 90
  means = {(c.P, c.mean) for c in ref.cases() if c.kind == 'mean'}
  assert len(means) == 2 * len(ref.MEANS)
  assert {ref.case('mean_0_48x48_48x48').form, ref.case('mean_0_24x241_16x160').form} == {
      'same_exact', 'wide'}
  # constant pre, constant post, both, and a faint pair
  for (P, Q) in ref.CONTENT_SHAPES:
    c = ref.case('content_' + ref._name(P, Q))
    assert c.a[0].max() - c.a[0].min() == 1 and c.a[0].min() == 200
    flat = [(x.min() == x.max(), y.min() == y.max()) for x, y in zip(c.a, c.c)]
    assert flat == [(False, False), (True, False), (False, True), (True, True), (False, False)]
    z = c.reference()['zero']
    assert z[1:4].all() and not z[0].any() and not z[4].any()
  assert {c.form for c in ref.cases() if c.kind == 'content'} == {
      'same_exact', 'same', 'general', 'wide'}


# the path every named shape must reach: (NCA, NCE), form, eligible as stacked
PATHS = {
    'same_exact_37x64_37x64': ((4, 5), 'same_exact', True),
    'same_exact_160x160_160x160': ((10, 11), 'same_exact', True),
    'same_17x17_17x17': ((3, 4), 'same', True),
    'same_127x129_127x129': ((10, 11), 'same', True),
    'same_144x144_144x144': ((10, 11), 'same', True),
    'same_200x150_200x150': ((10, 11), 'same', True),
    'general_48x48_32x32': ((3, 4), 'general', True),
    'general_160x160_96x112': ((10, 11), 'general', True),
    'general_160x160_1x1': ((10, 11), 'general', False),    # post image of 3 bytes
    'general_33x40_33x1': ((3, 4), 'general', True),
    'wide_24x161_16x160': ((15, 11), 'wide', True),
    'wide_24x176_16x160': ((15, 11), 'wide', True),
    'wide_40x240_33x97': ((15, 11), 'wide', True),
    'wide_20x240_20x16': ((15, 11), 'wide', True),
    'wide_24x241_16x160': ((20, 11), 'wide', True),
    'wide_24x320_16x160': ((20, 11), 'wide', True),
    'wide_37x257_20x33': ((20, 11), 'wide', True),
    'wide_18x320_18x160': ((20, 11), 'wide', True),
    'degenerate_1x16_1x16': ((3, 4), 'same', True),
    'degenerate_1x48_1x1': ((3, 4), 'general', False),      # post image of 3 bytes
    'degenerate_16x1_16x1': ((3, 4), 'same', True),
}


def test_same_size_pair_161_wide_is_not_eligible():
  """Px = Qx = 161 is the one shape that picks a search-window variant ((15, 11)) and
  the same-size mode, which those variants do not have."""
  assert ref.pick_variant(161, 161) == (15, 11) and ref.pick_variant(162, 162) is None
  assert not ref.eligible((24, 161), (24, 161), 10 ** 4, 10 ** 4)
  assert ref.eligible((24, 161), (24, 160), 10 ** 4, 10 ** 4)
  assert ref.eligible((24, 162), (24, 161), 10 ** 4, 10 ** 4)
  assert ref.eligible((24, 160), (24, 160), 10 ** 4, 10 ** 4)


@pytest.mark.parametrize('name', sorted(PATHS))
def test_case_reaches_the_path_it_names(name):
  c = ref.case(name)
  assert (c.variant, c.form, c.eligible) == PATHS[name]


def test_search_window_cases_put_the_regime_boundaries_where_they_should():
  """A regime boundary on a 16-column tile boundary (no per-lane tile between the
  runs) and inside a tile (REG 3 between them); clamped columns in the last tiles."""
  reg = {name: list(ref.tile_regimes(ref.case(name).P, ref.case(name).Q))
         for name in ref.case_names(lambda c: c.kind == 'wide')}
  # Qx = 160: L ends with tile 9, M starts with tile 10; Px = 161: R starts with tile 10
  # too -- there is no M tile and no boundary tile, the last tile (320 = Sx) is padding only
  assert reg['wide_24x161_16x160'][:21] == [0] * 10 + [2] * 10 + [3]
  # Px = 176: M is dx 1 .. 15, R from kx = 175: tile 10 holds both (per lane)
  assert reg['wide_24x176_16x160'][9:12] == [0, 3, 2]
  # Qx = 97: the L | M boundary inside tile 6; Px = 240: the M | R boundary inside tile 14
  r = reg['wide_40x240_33x97']
  assert r[5:8] == [0, 3, 1] and r[13:16] == [1, 3, 2]
  # Qx = 16: tile 0 is all L, tile 1 all M
  assert reg['wide_20x240_20x16'][:3] == [0, 1, 1]
  # Px = 241, 257: kx = Px - 1 is a multiple of 16 -- M ends with a tile, R starts with one
  assert reg['wide_24x241_16x160'][9:16] == [0, 1, 1, 1, 1, 1, 2]
  assert reg['wide_37x257_20x33'][14:18] == [1, 1, 2, 2]
  assert reg['wide_24x320_16x160'][18:21] == [1, 3, 2]
  for name, r in reg.items():
    c = ref.case(name)
    sx = c.P[1] + c.Q[1] - 1
    # the padding column kx = Sx lies in a per-lane tile
    # ((20, 240) / (20, 16): Sx = 255, its R columns share tile 14 with M ones)
    assert r[sx // 16] == 3 and {0, 3} <= set(r), name
    assert 2 in r or name == 'wide_20x240_20x16', name
    # the per-lane classification agrees with the tile runs
    for q, g in enumerate(r):
      lanes = {ref.lane_regime(c.P, c.Q, min(16 * q + n, sx - 1)) for n in range(16)}
      if g != 3:
        assert lanes == {'LMR'[g]}, (name, q)
  assert any(1 in r for r in reg.values())


def _ratios(c):
  """{form: error / (bound / K)} of the case's own restatement and, for the box-sum
  forms, of the other box-sum restatement on the same data (each within its own K)."""
  r = c.reference()
  out = {c.form: ref.check(r['restated'], r, c.P, c.Q, c.form, c.name) * ref.K[c.form]}
  if c.form in ('general', 'wide'):
    other = 'wide' if c.form == 'general' else 'general'
    r2 = dict(r, bound=ref.K[other] * r['unit'])
    got = ref._restate_box(r['terms'], fused=other == 'wide')
    out[other] = ref.check(got, r2, c.P, c.Q, other, c.name) * ref.K[other]
  return out


@pytest.mark.parametrize('name', ALL)
def test_restatement_is_within_the_derived_bound(name):
  """The float32 restatement of the form the case takes, every element; exact zeros
  where a patch is constant."""
  c = ref.case(name)
  for form, worst in _ratios(c).items():
    print(f'{name}: form {form} error / (bound / K) {worst:.3f}')
    assert worst <= ref.MEASURED_RATIO[form], 'the recorded ratio no longer covers this case'


def test_recorded_ratios_are_what_the_case_list_gives():
  """The record is reached to within 10 %, and K keeps its margin over it."""
  for form, k in ref.K.items():
    assert k >= ref.MARGIN[form] * ref.MEASURED_RATIO[form], form
  assert {f: m for f, m in ref.MARGIN.items() if m != 2.0} == {'wide': 1.9}
  worst = {}
  for c in ref.cases():
    for form, v in _ratios(c).items():
      worst[form] = max(worst.get(form, 0.0), v)
  assert set(worst) == set(ref.K)
  for form, v in worst.items():
    assert 0.9 * ref.MEASURED_RATIO[form] <= v <= ref.MEASURED_RATIO[form], (form, v)


@pytest.mark.parametrize('name', ALL)
def test_peak_pattern_is_the_recorded_one(name):
  """Which patches the peak test holds to the exact argmax, which to "no peak" and
  which it leaves out: equal to the table, so that none drops out unseen."""
  assert ref.peak_pattern(ref.case(name)) == ref.PEAK_PATTERN[name]
  assert set(ref.PEAK_PATTERN) == set(ALL)


def test_same_size_tables_need_the_corner_magnitudes():
  """Why TA / TB of the same-size forms are corner sums: with the box sums in their
  place the restated `emit` exceeds even K = 6 -- at small overlaps, where the table
  entries it rounds are far larger than the box sum they add up to."""
  c = ref.case('same_exact_48x48_48x48')
  r = c.reference()
  t = r['terms']
  e = (slice(None), None, None)
  box_unit = ref.U * (np.abs(t['S']) + np.abs(t['mub_x'][e] * t['SA']) +
                      np.abs(t['mua_x'][e] * t['SB']) +
                      np.abs(t['mua_x'] * t['mub_x'])[e] * t['n'] + np.abs(r['exact']))
  assert (box_unit <= r['unit'] * (1 + 1e-12)).all()
  err = np.abs(r['restated'].astype(np.float64) - r['exact'])
  assert (err > ref.K['same'] * box_unit).any()
  # ... and the general form on the same patches is within the box-sum bound
  r2 = dict(r, bound=ref.K['general'] * box_unit)
  ref.check(ref._restate_box(t, fused=False), r2, c.P, c.Q, 'general')


@pytest.mark.parametrize('name', ['same_exact_48x48_48x48', 'same_33x40_33x40',
                                  'general_48x48_32x32', 'wide_40x240_33x97'])
def test_checker_sees_the_errors_it_exists_for(name):
  """A wrong column term, a regime taken for another, a dropped n term: each is
  rejected, and named by tile."""
  c = ref.case(name)
  r = c.reference()
  t = r['terms']
  e = (slice(None), None, None)
  good = r['restated']
  ref.check(good, r, c.P, c.Q, c.form)
  # (c) the mA' mB' n term dropped
  muab = (t['mua'] * t['mub']).astype(np.float32)[e]
  with pytest.raises(AssertionError, match='tile q'):
    ref.check(good - muab * t['n'].astype(np.float32), r, c.P, c.Q, c.form)
  # (a) one column's SA taken from its neighbour (a wrong column term)
  bad = dict(t, SA=np.roll(t['SA'], 1, axis=2))
  with pytest.raises(AssertionError, match='tile q'):
    ref.check(ref._restate_box(bad, fused=True), dict(r, bound=ref.K['wide'] * r['unit']),
              c.P, c.Q, c.form)
  # (b) the overlap width of another regime: n off by one column in one tile
  n2 = t['n'].copy()
  n2[:, :, 16:32] += (c.Q[0] - np.abs(np.arange(n2.shape[1]) - (c.Q[0] - 1)))[None, :, None].clip(0, c.P[0])
  with pytest.raises(AssertionError, match='tile q 1'):
    ref.check(ref._restate_box(dict(t, n=n2), fused=True),
              dict(r, bound=ref.K['wide'] * r['unit']), c.P, c.Q, c.form)
  # a constant patch must give exact zeros; one element left at a sentinel is seen
  z = ref.case('content_48x48_48x48')
  rz = z.reference()
  g = rz['restated'].copy()
  assert (g[1:4] == 0).all()
  g[2, 5, 7] = 1e-30
  with pytest.raises(AssertionError, match='exactly 0'):
    ref.check(g, rz, z.P, z.Q, z.form)
  g = rz['restated'].copy()
  g[0, 3, 3] = -7.0
  with pytest.raises(AssertionError):
    ref.check(g, rz, z.P, z.Q, z.form)


def test_float32_constant_of_the_direct_kernel_covers_the_case_list():
  worst = max(ref.measure_float32(c) for c in ref.cases())
  print(f'largest float32 deviation / E: {worst:.3g}')
  assert worst <= ref.MEASURED_DEV32
  assert worst >= 0.5 * ref.MEASURED_DEV32, 'the record is stale'
  assert ref.TOL32 == 4 * ref.MEASURED_DEV32
