"""Pins tests/mesh_ref64.py, the statement of the spring-mesh operation, on the CPU:
against the golden vectors made from the reference, against the float32 oracle, and
its recorded constants K_F / K_S / K_E against what its own float32 form measures, and
its checks against CPU-made wrong results.  No kernel takes part."""
import json

import numpy as np
import pytest

from oracle import mesh_oracle
from tests import mesh_ref64 as ref

PLANAR = ((1, 0, 0), (0, 1, 0), (1, 1, 0), (-1, 1, 0))


def test_rest_lengths_of_the_case_strides_have_one_float32_value():
  """The kernel takes |rest| in float32 from the float32 rest vector, the reference's
  in-plane code rounds the double norm of the stride: the same float for every stride
  the case lists use (else the bit-equality check would compare two rest lengths)."""
  f32 = np.float32
  for st in ref.STRIDES_2D + (ref.STEP_STRIDE_2D, (40.0, 40.0)):
    assert np.sqrt(f32(st[0]) * f32(st[0]) + f32(st[1]) * f32(st[1])) == \
        f32(np.linalg.norm(np.array(st)))
  for st in ref.STRIDES_3D + (ref.STEP_STRIDE_3D, (40.0, 40.0, 40.0)):
    for d, rest, l0, _ in ref.families(3, 0.1, st):
      # mesh.py:249-253: np.linalg.norm of the float32 rest vector
      assert l0 == np.linalg.norm(rest.reshape(3, 1, 1, 1)), (st, d)


def test_float32_form_matches_the_golden_forces(golden):
  """mesh_force.npz was produced by the reference's source over a NumPy stand-in for
  jax, which keeps some intermediate products in double: it lies between the float32
  form and the float64 statement, not bit for bit on either.  Measured: at most 0.21
  units of 2^-24 S from the float32 form (K_F, form against float64, is 2.4)."""
  g = golden('mesh_force')
  worst = 0.0
  cases = []
  for poo in (0, 1):
    cases += [(g['x2'], 0.1, (40.0, 30.0), bool(poo), None, g[f'f2_{poo}']),
              (g['x3'], 0.1, (20.0, 25.0, 14.0), bool(poo), None, g[f'f3_{poo}']),
              (g['x3b'], 0.05, 16.0, bool(poo), None, g[f'f3b_{poo}']),
              (g['xf'], 0.1, (40.0, 40.0), bool(poo), None, g[f'ff_{poo}'])]
  cases.append((g['x3'], 0.1, (20.0, 25.0, 14.0), False, PLANAR, g['f3_planar']))
  for x, k, st, poo, links, want in cases:
    form, S = ref.force_bound(x, k, st, poo, links, np.float32)
    f64 = ref.force(x, k, st, poo, links, np.float64)
    # (no zero pattern here: at rest the stand-in's double diagonal length leaves
    # residues of 7e-10 where float32 gives exactly 0)
    worst = max(worst, ref.units(form, want, S[None]))
    assert ref.units(f64, want, S[None]) <= ref.K_F
  print('golden forces: float32 form within %.3g units' % worst)
  assert worst <= 0.25


def test_float32_form_matches_the_golden_first_step(golden):
  """mesh_vv.npz, `fire1` (the only fixture of at most three steps): positions bit for
  bit, scalars equal; v and a within the stand-in's mixed precision (measured 2.5 and
  0.2 units)."""
  g = golden('mesh_vv')
  c = json.loads(str(g['cfgs']))['fire1']
  cap = c.pop('_force_cap')
  c['stride'] = tuple(c['stride'])
  cfg = ref.Cfg(**c)
  scales = {}
  got = ref.step(g['x0'], np.zeros_like(g['x0']), g['prev'], cfg, cap, 1, np.float32, None,
                 scales)
  np.testing.assert_array_equal(got[0], g['fire1_x'])
  assert ref.units(got[1], g['fire1_v'], scales['v']) <= 3.0
  assert ref.units(got[2], g['fire1_a'], scales['a']) <= 0.25
  assert [float(s) for s in got[3:]] == list(g['fire1_scal'])


def test_oracle_agrees_within_the_bound():
  """oracle.mesh_oracle adds the in-plane families in another order (far, near per
  family): not the float32 form, but within the device's allowance of the statement
  and of the form, on every case of the list."""
  worst = 0.0
  for c in ref.force_cases():
    if c.group == 'grid':
      continue
    for poo in (False, True):
      want, S, form = ref.force_refs(c.name, poo)
      with np.errstate(all='ignore'):
        if c.ncomp == 2:
          got = mesh_oracle.inplane_force(c.x, c.k, c.stride, poo)
        else:
          got = mesh_oracle.elastic_mesh_3d(c.x, c.k, c.stride, poo,
                                            links=c.links or mesh_oracle.LINKS_3D)
      u = max(ref.units(got, want, S[None]), ref.units(got, form, S[None]))
      assert u <= ref.DEV_FACTOR * ref.K_F, (c.name, poo, u)
      if c.ncomp == 3:
        # same order per link: the volumetric oracle IS the float32 form
        assert np.array_equal(got, form), (c.name, poo)
      worst = max(worst, u)
  print('oracle within %.3g units of 2^-24 S' % worst)


def test_measured_force_constant():
  """K_F: the float32 form against the float64 statement over the whole case list."""
  worst, where = 0.0, None
  for c in ref.force_cases():
    for poo in (False, True):
      want, S, form = ref.force_refs(c.name, poo)
      u = ref.check_force(form, c.name, poo, factor=1.0)   # the form passes its own check
      if u > worst:
        worst, where = u, (c.name, poo)
  print('measured K_F = %.3f at %s (recorded %.3g; %d cases)'
        % (worst, where, ref.K_F, len(ref.force_cases())))
  assert worst <= ref.K_F <= 1.25 * worst


def test_measured_step_constants():
  """K_S for x, v, a: the float32 form of `step` against float64 over the step cases;
  the FIRE scalars are equal."""
  worst = {'x': 0.0, 'v': 0.0, 'a': 0.0, 'e': 0.0}
  where = {}
  cases = ref.step_cases()
  uphill = 0

  def measure(got, want, scales, name):
    for i, key in enumerate('xva'):
      u = ref.units(got[i], want[i], scales[key])
      if u > worst[key]:
        worst[key], where[key] = u, name
    # K_E: the float32 form's |v_n|^2 terms, summed in float32 one after the other (the
    # worst order a kernel could choose), against their float64 sum
    v = got[1]
    v2 = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] if v.shape[0] == 3 else np.float32(0))
    assert v2.dtype == np.float32
    exact = float(v2.sum(dtype=np.float64))
    if exact > 0:
      u = abs(float(np.cumsum(v2.ravel(), dtype=np.float32)[-1]) - exact) / (ref.EPS * exact)
      if u > worst['e']:
        worst['e'], where['e'] = u, name
    # the form passes the checks on the statistics with its own sums
    ref.check_stats(np.float32(exact), np.sqrt(v2.max()), want[1], scales['v'], name)

  for c in cases:
    want, scales = ref.step_refs(c)
    got = ref.step(c.x, c.v, c.prev, c.cfg, c.force_cap, c.n, np.float32, c.links,
                   dt0=c.dt0, alpha0=c.alpha0)
    assert got[3:] == want[3:], c.name
    uphill += bool(c.cfg.fire and want[5] < c.n)
    measure(got, want, scales, c.name)
  relax = ref.relax_cases()
  for c in relax:
    chunks, e_kin, t = ref.relax_refs(c)
    got, got_e, got_t = ref.relax_chunks(c, 3, np.float32)
    assert got_t == t == c.cfg.max_iters and len(got_e) == len(e_kin) == t, c.name
    # max_iters = 3 ends on the cap (the third chunk runs at final_cap), 2 on max_iters
    assert [float(ch[7][2]) for ch in chunks] == [1.0, 1.5, 2.0][:t], c.name
    for g, w in zip(got, chunks):
      assert g[3] == w[3] and g[7] == w[7], c.name
      measure(g, w, w[6], c.name)
    ref.check_relax(got[-1][0], got_e, got_t, c, 'float32 form',
                    [g[7] for g in got], [g[3] for g in got])
  print('measured K_S = %s, K_E = %.3f at %s (recorded %s, %s; %d + %d cases, %d with an '
        'uphill step)' % ({k: round(worst[k], 3) for k in 'xva'}, worst['e'], where, ref.K_S,
                          ref.K_E, len(cases), len(relax), uphill))
  assert uphill >= 50
  for key in 'xva':
    assert worst[key] <= ref.K_S[key] <= 1.25 * worst[key], key
  assert worst['e'] <= ref.K_E <= 1.25 * worst['e']


def test_large_drift_means_need_no_term_of_their_own():
  """The drift means of the meshes past 262 144 nodes: a float32 mean summed one after
  the other against NumPy's pairwise one (the float32 form's), in K_S['x'] / K_S['v']
  units.  Both orders stay far inside the (DEV_FACTOR - 1) x K_S that the device has
  beyond the form's own error, so the grid-stride cases get no summation term."""
  for shape in ref.GRID_STRIDE:
    case = ref.step_cases_large(shape)[1]
    assert case.cfg.remove_drift
    (x, v, _, *_), scales = ref.step_refs(case)
    for key, t in (('x', x), ('v', v)):
      t32 = t.astype(np.float32).reshape(t.shape[0], -1)
      n = t32.shape[1]
      seq = np.cumsum(t32, axis=1, dtype=np.float32)[:, -1] / np.float32(n)
      pair = t32.mean(axis=1, dtype=np.float32)
      exact = t32.mean(axis=1, dtype=np.float64)
      u = max(ref.units(seq, pair, scales[key]), ref.units(seq, exact, scales[key]),
              ref.units(pair, exact, scales[key]))
      print('%s: mean of %s over %d nodes, sequential / pairwise / exact within %.3g units'
            % (case.name, key, n, u))
      assert u <= 0.25 * (ref.DEV_FACTOR - 1) * ref.K_S[key]


def test_step_cases_move_every_fire_scalar():
  """The downhill configuration changes dt, alpha and the cap on every step and reaches
  final_cap at the second; the uphill one halves dt, zeroes v and resets alpha."""
  shape = (2, 1, 5, 1)
  seen = []
  for n in (1, 2, 3):
    c = ref.step_case(shape, 'fire_down', 'prev', n, False)
    seen.append(ref.step_refs(c)[0][3:])
  assert [s[2] for s in seen] == [1, 2, 3]
  assert seen[0][0] < seen[1][0] < seen[2][0] and seen[0][1] > seen[1][1] > seen[2][1]
  assert seen[0][3] == np.float32(1.5) and seen[1][3] == seen[2][3] == np.float32(2.0)
  c = ref.step_case(shape, 'fire_up', 'prev', 1, False)
  (x, v, a, dt, alpha, n_pos, cap), _ = ref.step_refs(c)
  assert n_pos == 0 and dt == np.float32(np.float32(0.3) * np.float32(0.5))
  assert alpha == np.float32(0.1) and not v.any()


def test_the_checks_reject_wrong_results():
  """check_force fails on one flipped ulp, one lost spring term and a NaN."""
  name = 'deg2d_2x5x2x2_s1_a3'
  want, S, form = ref.force_refs(name, True)
  ref.check_force(form, name, True)
  bad = form.copy()
  bad[0, 2, 1, 1] = np.nextafter(bad[0, 2, 1, 1], np.float32(np.inf))
  with pytest.raises(AssertionError):
    ref.check_force(bad, name, True)
  ref.check_force(bad, name, True, bitwise=False)          # one ulp is inside the bound
  bad = form.copy()
  bad[1, 0, 0, 0] += np.float32(1e-3) * np.float32(S[0, 0, 0])
  with pytest.raises(AssertionError):
    ref.check_force(bad, name, True, bitwise=False)
  bad = form.copy()
  bad[0, 0, 0, 0] = np.nan
  with pytest.raises(AssertionError):
    ref.check_force(bad, name, True, bitwise=False)
  zero = ref.force_refs('deg2d_2x1x1x1_s0_a3', False)[2].copy()
  assert zero.view(np.uint32).max() == 0
  zero[0, 0, 0, 0] = 1e-30
  with pytest.raises(AssertionError):
    ref.check_force(zero, 'deg2d_2x1x1x1_s0_a3', False, bitwise=False)


def _form(case, taps=None, **wrong):
  """The float32 form of a case's chunk, optionally wrong in one named way."""
  return ref.step(case.x, case.v, case.prev, case.cfg, case.force_cap, case.n, np.float32,
                  case.links, dt0=case.dt0, alpha0=case.alpha0, taps=taps, _wrong=wrong)


def _stats32(v):
  e, vm = ref.chunk_stats(v)
  return np.float32(e), np.float32(vm)


def test_the_checks_reject_wrong_steps_statistics_and_carry_over():
  """check_step, check_case_stats and check_relax pass the float32 form and fail on
  CPU-made results that are wrong the way a kernel hand-over can be."""
  vol, vol5 = (3, 3, 4, 5), (3, 2, 3, 4, 5)
  # the last step's pending update not applied: scalars one step behind, and the last
  # gate / drift missing
  for shape, kind in ((vol, 'fire_down'), (vol, 'fire_up'), (vol5, 'fire_drift'),
                      ((2, 1, 4, 40), 'fire_drift')):
    for n in (1, 2):
      c = ref.step_case(shape, kind, 'prev', n, False)
      ref.check_step(_form(c), c)
      bad = _form(c, pending_lost=True)
      with pytest.raises(AssertionError):
        ref.check_step(bad, c)
      good = ref.step_refs(c)[0]
      # (after a downhill step without drift only the scalars are pending)
      if kind == 'fire_drift' or (kind == 'fire_up' and n == 1):
        with pytest.raises(AssertionError):    # the arrays alone give it away, too
          ref.check_step(bad[:3] + good[3:], c)
  # 5-D drift taken globally, and per column over B * z only
  for shape in (vol5, (3, 1, 3, 4, 5)):
    c = ref.step_case(shape, 'fire_drift', 'prev_nan', 1, True)
    ref.check_step(_form(c), c)
    for axes in ((1, 2, 3, 4), (1, 2)):
      with pytest.raises(AssertionError):
        ref.check_step(_form(c, drift_axes=axes), c)
  # e_kin / v_max taken before the last gate, and with the drift of v missing
  for c in ref.uphill_end_cases(vol)[:2] + ref.uphill_end_cases((2, 2, 17, 63))[:2]:
    taps = {}
    got = _form(c, taps)
    assert ref.check_case_stats(*_stats32(got[1]), c) == (0.0, 0.0)
    for wrong in (_stats32(taps['v_gate']), (np.float32(0), np.float32(1e-30)),
                  (np.float32(1e-30), np.float32(0)), (np.float32(np.nan), np.float32(0))):
      with pytest.raises(AssertionError):
        ref.check_case_stats(*wrong, c)
  for shape in (vol, vol5, (2, 1, 4, 40)):
    # (with the pull to prev: springs alone leave the mean velocity at 0)
    c = ref.step_case(shape, 'fire_drift', 'prev', 2, False)
    taps = {}
    got = _form(c, taps)
    e, vm = _stats32(got[1])
    ref.check_case_stats(e, vm, c)
    we, wvm = _stats32(taps['v_drift'])
    with pytest.raises(AssertionError):
      ref.check_case_stats(we, wvm, c)
    # (v_max is the sharper of the two: the mean adds to e_kin only in second order)
    with pytest.raises(AssertionError):
      ref.check_case_stats(e, wvm, c)
    with pytest.raises(AssertionError):
      ref.check_case_stats(e * np.float32(1.001), vm, c)
    with pytest.raises(AssertionError):
      ref.check_case_stats(e, vm * np.float32(1.001), c)
  # a second chunk that keeps n_pos, that limits dt by the carried dt, and that reuses
  # the old a instead of recomputing it with the carried cap
  for shape in ref.CHUNK_SHAPES:
    for c in ref.second_chunk_cases(shape):
      got = _form(c)
      ref.check_step(got, c)
      assert got[3] == np.float32(1.3 * 0.3) and got[5] == c.n
      for wrong in (dict(n_pos0=2), dict(dt_carried=True), dict(a0_cap=1.0)):
        with pytest.raises(AssertionError):
          ref.check_step(_form(c, **wrong), c)
    for c in ref.cap_raise_cases(shape):
      for wrong in (dict(n_pos0=1), dict(a0_cap=1.0)):     # (dt_max does not bind here)
        got, e_kin, t = ref.relax_chunks(c, 3, np.float32, _wrong=wrong)
        with pytest.raises(AssertionError):
          ref.check_relax(got[-1][0], e_kin, t, c, 'wrong', [g[7] for g in got],
                          [g[3] for g in got])
      # a loop that never raises the cap stops one chunk early or runs at the old cap
      got, e_kin, t = ref.relax_chunks(c, 3, np.float32)
      with pytest.raises(AssertionError):
        ref.check_relax(got[-1][0], e_kin[:-1], t - 1, c)
