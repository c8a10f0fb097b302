"""The spring-mesh operation, stated once in plain NumPy.  TEST INFRASTRUCTURE.

`force` is the spring law of the reference (mesh.py:42-169 in-plane, :192-279
volumetric), `step` its damped velocity Verlet / FIRE step (mesh.py:371-521),
written from their observable behaviour.  CPU only; nothing under sofima_amd/
imports this module.

Two forms of the same code:

  dtype=np.float64  the statement: the float32 inputs the kernel gets (positions,
                    rest vectors, spring constants), widened, every operation in
                    double.  Every spring term is rounded to float32 and passed
                    through nan_to_num(nan=0, posinf=0, neginf=0) as in the
                    reference, so a term that overflows float32 is zeroed there too.
  dtype=np.float32  the *float32 form*: the reference's operations in the
                    reference's order -- in-plane f1p + f2p + f3p + f4p - f1n - f2n -
                    f3n - f4n (mesh.py:169), volumetric per link += far, -= near
                    (mesh.py:271-277).  oracle/mesh_oracle.py adds the in-plane
                    families far, near, far, near: that is why it is not this form.

Parameters are formed as build_params (csrc/sfm_mesh.hip) forms them: rest =
float32(stride * dir); in-plane constants k and float32(k) / sqrt(float32(2)), rest
lengths float32(stride) and float32(|stride|); the volumetric rest length is the
float32 norm of the float32 rest vector and k_eff = float32(k * stride_x / l0) with
the quotient taken in double.  For every stride of the case lists the float32 norm
of the rest vector and the rounded double norm are the same float
(tests/test_mesh_ref64.py asserts it), so the kernel's own rest lengths are these.

Error bound.  `force_bound` returns, next to the force, the per-node magnitude sum

  S(n) = sum over the node's springs of
         k_s * (max_c |x_far| + max_c |x_near| + max_c |rest|) * (1 + l0_s / l_s)

with l_s taken from float64.  (1 + l0 / l) is the conditioning of d / l: without it
near-coincident nodes break any bound.  A spring with a NaN end, or of length 0,
contributes exactly nothing to the force and nothing to S.  A spring with an
infinite end (and no NaN) still pulls on its finite components with -k d (l0 / inf
is 0): it enters S with its finite components and the factor 1.  (The issue's
wording drops such a spring from S altogether; an end node whose only spring it is
would then have S = 0 next to a rounded, non-zero force.)  Components are in units
of 2^-24 * S.

Measured constants (tests/test_mesh_ref64.py recomputes them on the CPU, prints them
and asserts that the values below still cover them; never taken from a kernel):

  K_F   largest |float32 form - float64| / (2^-24 S) over force_cases()
  K_S   the same for x, v, a after 1 .. 3 steps over step_cases(), in units of
        2^-24 * scale: scale(x), scale(v) = largest |float64 value| of the array,
        scale(a) = largest S(n) + k0 |x - prev| (it does not vanish at equilibrium)
  K_E   largest error of a float32 sum, one term after the other, of the float32 form's
        |v_n|^2 terms against their float64 sum, in units of 2^-24 e_kin (stat_bounds)

The device is allowed 4 x: the project's usual margin (ATOL32 = 4 x MEASURED_DEV32),
for one-ulp differences between correctly rounded sequences and other summation
orders of the FIRE sums.
"""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

f32 = np.float32
EPS = 2.0 ** -24

# Measured by tests/test_mesh_ref64.py on the CPU (2.357; 3.613, 53.74, 1.053; 95.47),
# rounded up.  (K_S['x'] was 3.2, measured 3.140, before the volumetric and chunk cases.)
K_F = 2.4
K_S = {'x': 3.7, 'v': 54.0, 'a': 1.1}
K_E = 96.0
DEV_FACTOR = 4.0

LINKS_3D = (
    (1, 0, 0), (0, 1, 0), (0, 0, 1),
    (1, 1, 0), (-1, 1, 0), (1, 0, 1), (-1, 0, 1), (0, 1, 1), (0, -1, 1),
    (1, 1, 1), (1, 1, -1), (1, -1, 1), (-1, 1, 1),
)
PLANAR = ((1, 0, 0), (0, 1, 0), (1, 1, 0), (-1, 1, 0))


# ---------------------------------------------------------------------------
# the spring law
# ---------------------------------------------------------------------------
def families(ncomp, k, stride, links=None):
  """[(dir xyz, rest float32[ncomp], l0 float32, k_eff float32)] as build_params."""
  out = []
  if ncomp == 2:
    if len(stride) != 2:
      raise ValueError('stride must be 2D.')
    sx, sy = float(stride[0]), float(stride[1])
    kf = f32(k)
    k2 = kf / np.sqrt(f32(2.0))
    diag = f32(np.linalg.norm(np.array([sx, sy])))
    for d, l0, kk in (((1, 0, 0), f32(sx), kf), ((0, 1, 0), f32(sy), kf),
                      ((1, 1, 0), diag, k2), ((-1, 1, 0), diag, k2)):
      out.append((d, np.array([f32(d[0] * sx), f32(d[1] * sy)], f32), l0, f32(kk)))
    return out
  if np.ndim(stride) == 0:
    stride = (stride,) * 3
  st = np.array(stride, np.float64)
  for d in (LINKS_3D if links is None else links):
    d = tuple(int(v) for v in d)
    if len(d) != 3 or any(abs(v) > 1 for v in d):
      raise ValueError('Only |v| <= 1 values supported within links.')
    rest = np.array(st * np.array(d), f32)
    l0 = np.sqrt((rest[0] * rest[0] + rest[1] * rest[1]) + rest[2] * rest[2])
    with np.errstate(divide='ignore', invalid='ignore'):
      k_eff = f32(float(k) * st[0] / np.float64(l0))
    out.append((d, rest, f32(l0), k_eff))
  return out


def _ends(nsp, d):
  """Slices of the far and the near end over the last nsp axes ([z]yx; d is xyz)."""
  far, near = [], []
  for v in d[::-1][-nsp:]:
    if v == 1:
      far.append(slice(1, None)); near.append(slice(None, -1))
    elif v == -1:
      far.append(slice(None, -1)); near.append(slice(1, None))
    else:
      far.append(slice(None)); near.append(slice(None))
  return tuple(far), tuple(near)


def _spring_terms(x, fams, prefer, dtype):
  """Per family: (far index, near index, spring term [C, ...] in dtype, after the
  float32 rounding and nan_to_num)."""
  nc = x.shape[0]
  nsp = 2 if nc == 2 else 3
  lead = (slice(None),) * (x.ndim - nsp)
  xs = x.astype(dtype)
  for d, rest, l0, kk in fams:
    far, near = _ends(nsp, d)
    far, near = lead + far, lead + near
    r = rest.astype(dtype).reshape((nc,) + (1,) * (x.ndim - 1))
    with np.errstate(all='ignore'):
      dd = xs[far] - xs[near] + r
      sq = dd[0] * dd[0] + dd[1] * dd[1]
      if nc == 3:
        sq = sq + dd[2] * dd[2]
      l = np.sqrt(sq)
      if prefer:
        fac = np.ones_like(dd)
        for c in range(nc):
          if d[c] != 0:
            fac[c] = dtype(d[c]) * np.sign(dd[c])
        t = (dtype(l0) * fac) / l
      else:
        t = dtype(l0) / l
      f = (dtype(-kk) * (dtype(1.0) - t)) * dd
      f = np.nan_to_num(f.astype(f32), nan=0.0, posinf=0.0, neginf=0.0).astype(dtype)
    yield far, near, f


def force_bound(x, k, stride, prefer_orig_order, links=None, dtype=np.float64):
  """(force in `dtype`, S float64 [spatial shape of x])."""
  x = np.asarray(x)
  if x.dtype != np.float64 or dtype == np.float32:
    x = np.asarray(x, f32)     # (a float64 array is the float64 form's own state)
  nc = x.shape[0]
  if nc not in (2, 3):
    raise ValueError('x must be [2 | 3, ...]')
  if nc == 2 and x.ndim != 4:
    raise ValueError('in-plane meshes are [2, z, y, x]')
  if nc == 3 and x.ndim < 4:
    raise ValueError('volumetric meshes are [3, [batch..], z, y, x]')
  fams = families(nc, k, stride, links)
  out = np.zeros(x.shape, dtype)
  terms = list(_spring_terms(x, fams, bool(prefer_orig_order), dtype))
  if nc == 2:
    for far, near, f in terms:       # f1p + f2p + f3p + f4p ...
      out[far] += f
    for far, near, f in terms:       # ... - f1n - f2n - f3n - f4n
      out[near] -= f
  else:
    for far, near, f in terms:       # per link: += far, -= near
      out[far] += f
      out[near] -= f
  # magnitude sum, always from float64
  S = np.zeros(x.shape[1:], np.float64)
  x64 = x.astype(np.float64)
  for (far, near, _), (d, rest, l0, kk) in zip(terms, fams):
    xf, xn = x64[far], x64[near]
    r = rest.astype(np.float64).reshape((nc,) + (1,) * (x.ndim - 1))
    with np.errstate(all='ignore'):
      dd = xf - xn + r
      l = np.sqrt(np.sum(dd * dd, axis=0))
      has_nan = np.isnan(xf).any(axis=0) | np.isnan(xn).any(axis=0) | np.isnan(l)
      fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0).max(axis=0)
      mag = fin(xf) + fin(xn) + np.abs(rest.astype(np.float64)).max()
      cond = np.where(np.isinf(l), 1.0, 1.0 + float(l0) / l)
      s = abs(float(kk)) * mag * cond
    s = np.where(has_nan | (l == 0), 0.0, s)
    S[far[1:]] += s
    S[near[1:]] += s
  return out, S


def force(x, k, stride, prefer_orig_order, links=None, dtype=np.float64):
  return force_bound(x, k, stride, prefer_orig_order, links, dtype)[0]


# ---------------------------------------------------------------------------
# the integrator
# ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Cfg:
  """The fields of mesh.IntegrationConfig (mesh.py:282-338)."""
  dt: float
  gamma: float
  k0: float
  k: float
  stride: tuple
  num_iters: int
  max_iters: int
  stop_v_max: float
  fire: bool = True
  f_alpha: float = 0.99
  f_inc: float = 1.1
  f_dec: float = 0.5
  alpha: float = 0.1
  n_min: int = 5
  dt_max: float = 10.0
  start_cap: float = 1e6
  final_cap: float = 1e6
  cap_scale: float = 1.1
  cap_upscale_every: int = 100
  prefer_orig_order: bool = False
  remove_drift: bool = False


def fire_next(dt, alpha, n_pos, cap, downhill, cfg, dt_lim=None):
  """The FIRE scalar update (mesh.py:459-490), in float32 like the kernel's fire_next.
  dt is limited by dt_max x config.dt whatever dt the chunk started from (`dt_lim` is
  for the wrong results of tests/test_mesh_ref64.py only)."""
  n_pos = n_pos + 1 if downhill else 0
  if dt_lim is None:
    dt_lim = f32(float(cfg.dt_max) * float(cfg.dt))
  if downhill:
    if n_pos > cfg.n_min:
      dt = min(f32(dt * f32(cfg.f_inc)), dt_lim)
      alpha = f32(alpha * f32(cfg.f_alpha))
    if n_pos > 0 and n_pos % max(int(cfg.cap_upscale_every), 1) == 0:
      cap = f32(f32(cfg.cap_scale) * cap)
  else:
    dt = f32(dt * f32(cfg.f_dec))
    alpha = f32(cfg.alpha)
  cap = min(cap, f32(cfg.final_cap))
  return f32(dt), f32(alpha), n_pos, f32(cap)


def _widen(t, dtype):
  """The float32 array a kernel gets, in `dtype`; a float64 array is the float64
  statement's own state between two chunks and stays as it is."""
  t = np.asarray(t)
  if t.dtype == np.float64 and dtype == np.float64:
    return t
  return np.asarray(t, f32).astype(dtype)


def step(x, v, prev, cfg, force_cap, n, dtype=np.float64, links=None, scales=None,
         dt0=None, alpha0=None, taps=None, _wrong=None):
  """`n` <= 3 steps of mesh.velocity_verlet: one chunk.  Returns (x, v, a, dt, alpha,
  n_pos, cap); the four scalars are float32 / int with FIRE and None without.  `scales`,
  a dict, receives the error scales of x, v and a (see the module docstring).

  `dt0` / `alpha0` are the chunk's starting fire_dt / fire_alpha (default cfg.dt,
  cfg.alpha); n_pos starts at 0 in every chunk (mesh.py:513), the first force is taken
  with `force_cap`, and dt stays limited by f32(dt_max * cfg.dt), not by dt0.

  States may be 5-D [3, B, z, y, x]: the force treats every axis in front of (z, y, x)
  as a batch, and the drift means are over axes (1, 2, 3) as the reference hard-codes
  them (mesh.py:496-497) -- global for a 4-D state, one mean per x column over
  (B, z, y) for a 5-D one.

  With FIRE every step asserts |power| > 1e-3 |a| |v| (or an exactly zero state):
  the branch taken does not depend on round-off.

  `taps`, a dict, receives the last step's velocity before the gate (`v_gate`) and
  before the drift removal (`v_drift`).  `_wrong` (a dict) makes the deliberately wrong
  results that tests/test_mesh_ref64.py feeds to the checks: `pending_lost`,
  `drift_axes`, `n_pos0`, `dt_carried`, `a0_cap`.  Never used for an expectation.
  """
  assert 0 <= n <= 3
  wrong = _wrong or {}
  x = _widen(x, dtype)
  v = _widen(v, dtype)
  pv = None if prev is None else np.asarray(prev, f32).astype(dtype)
  poo = cfg.prefer_orig_order
  s_a = [0.0]

  def total(x, cap):
    with np.errstate(all='ignore'):
      a, S = force_bound(x, cfg.k, cfg.stride, poo, links, dtype)
      pull_mag = 0.0
      if pv is not None:
        pull = dtype(-f32(cfg.k0)) * np.nan_to_num(x - pv)
        a = a + np.clip(pull, -dtype(cap), dtype(cap))
        pull_mag = np.abs(np.nan_to_num(x - pv, posinf=0.0, neginf=0.0)) * abs(float(cfg.k0))
        pull_mag = pull_mag.max(axis=0)
      s_a[0] = float(np.max(S + pull_mag))
    return a.astype(dtype)

  half, one = dtype(0.5), dtype(1.0)
  g = dtype(f32(cfg.gamma))
  cap = f32(force_cap)
  a = total(x, f32(wrong.get('a0_cap', cap)))
  dt = f32(cfg.dt if dt0 is None else dt0)
  alpha = f32(cfg.alpha if alpha0 is None else alpha0)
  dt_lim = f32(float(cfg.dt_max) * float(dt)) if wrong.get('dt_carried') else None
  n_pos = int(wrong.get('n_pos0', 0))
  for it in range(n):
    dtw = dtype(dt)
    x = x + (dtw * v + (half * (dtw * dtw)) * a)
    a_new = total(x, cap)
    hdtg = (half * dtw) * g
    v = (one / (one + hdtg)) * (v * (one - hdtg) + (half * dtw) * (a + a_new))
    a = a_new
    if not cfg.fire:
      continue
    with np.errstate(all='ignore'):
      a_n = np.sqrt(np.sum(a * a, axis=0, keepdims=True)) + dtype(1e-6)
      v_n = np.sqrt(np.sum(v * v, axis=0, keepdims=True))
      power = float(np.sum(a.astype(np.float64) * v.astype(np.float64)))
      size = float(np.linalg.norm(a.astype(np.float64)) * np.linalg.norm(v.astype(np.float64)))
      v = v + dtype(alpha) * (a / a_n * v_n - v)
    assert abs(power) > 1e-3 * size or (power == 0 and size == 0), (power, size)
    if taps is not None and it == n - 1:
      taps['v_gate'] = v
    if wrong.get('pending_lost') and it == n - 1:
      continue
    downhill = power >= 0
    dt, alpha, n_pos, cap = fire_next(dt, alpha, n_pos, cap, downhill, cfg, dt_lim)
    v = v * dtype(1.0 if downhill else 0.0)
    if taps is not None and it == n - 1:
      taps['v_drift'] = v
    if cfg.remove_drift:
      # the reference hard-codes axes (1, 2, 3) (mesh.py:496-497)
      axes = wrong.get('drift_axes', (1, 2, 3))
      x = x - x.mean(axis=axes, keepdims=True, dtype=dtype)
      v = v - v.mean(axis=axes, keepdims=True, dtype=dtype)
  if scales is not None:
    top = lambda t: float(np.abs(np.nan_to_num(t, posinf=0.0, neginf=0.0)).max())
    scales.update(x=top(x), v=top(v), a=s_a[0])
  if not cfg.fire:
    return x, v, a, None, None, None, None
  return x, v, a, f32(dt), f32(alpha), int(n_pos), f32(cap)


def chunk_stats(v):
  """(e_kin, v_max) as relax_mesh forms them from a chunk's velocities (mesh.py:584-586):
  sum of |v_n|^2 and largest |v_n| over the nodes, in float64."""
  v2 = np.sum(np.asarray(v, np.float64) ** 2, axis=0)
  return float(v2.sum()), float(np.sqrt(v2.max()))


def assert_v_max_margin(v_max, stop_v_max):
  """A condition on a chunk case's inputs: the float64 v_max is exactly 0 or at least
  1 % away from stop_v_max, so the stop rule does not depend on round-off."""
  assert v_max == 0 or abs(v_max - stop_v_max) >= 0.01 * stop_v_max, (v_max, stop_v_max)


def relax_chunks(case, n_chunks, dtype=np.float64, _wrong=None):
  """The chunk loop of relax_mesh (mesh.py:570-606) around `step`, from v = 0: x and v
  pass from chunk to chunk, dt / alpha / cap are carried with FIRE, n_pos restarts and
  the first force of every chunk is taken again with the carried cap.  Stops on
  max_iters, or on v_max < stop_v_max once the cap has reached final_cap (compared in
  float32 like mesh._relax_loop); below final_cap it raises the cap to
  min(cap * cap_scale, final_cap) instead.

  Returns ([(x, v, a, (dt, alpha, n_pos, cap), e_kin, v_max, scales, (dt0, alpha0,
  cap0))] per chunk, the e_kin list, t).  At most `n_chunks` chunks and three steps
  in all: the n <= 3 contract of `step`, and the meaning of K_S, hold.
  """
  cfg = case.cfg
  x, v = case.x, np.zeros_like(case.x)
  t, dt, alpha, cap = 0, f32(cfg.dt), f32(cfg.alpha), f32(cfg.start_cap)
  chunks, e_kin = [], []
  while t < cfg.max_iters:
    assert len(chunks) < n_chunks and t + cfg.num_iters <= 3, (case.name, t)
    scales = {}
    start = (dt, alpha, cap)
    out = step(x, v, case.prev, cfg, cap, cfg.num_iters, dtype, case.links, scales,
               dt0=dt, alpha0=alpha, _wrong=_wrong)
    t += cfg.num_iters
    x, v = out[:2]
    e, v_max = chunk_stats(v)
    if dtype == np.float64:
      assert_v_max_margin(v_max, cfg.stop_v_max)
    e_kin.append(e)
    if cfg.fire:
      dt, alpha, cap = out[3], out[4], out[6]
    chunks.append((x, v, out[2], out[3:], e, v_max, scales, start))
    if v_max < cfg.stop_v_max:
      if f32(cap) >= f32(cfg.final_cap):
        break
      cap = f32(min(float(cap) * float(cfg.cap_scale), float(cfg.final_cap)))
  return chunks, e_kin, t


# ---------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class ForceCase:
  name: str
  x: np.ndarray                 # float32 [2 | 3, ...]
  k: float
  stride: tuple
  links: tuple | None = None    # volumetric only; None: the 13 default links
  group: str = ''

  @property
  def ncomp(self):
    return int(self.x.shape[0])


def _rng(name):
  return np.random.default_rng(zlib.crc32(name.encode()))


def _rand(name, shape, amp):
  return (_rng(name).standard_normal(shape) * amp).astype(f32)


STRIDES_2D = ((40.0, 30.0), (14.3, 9.7))
STRIDES_3D = ((40.0, 40.0, 30.0), (14.3, 9.7, 31.1))
DEGENERATE_2D = ((2, 1, 1, 1), (2, 3, 1, 1), (2, 1, 1, 2), (2, 1, 2, 1), (2, 1, 2, 2),
                 (2, 5, 2, 2), (2, 2, 1, 37), (2, 2, 37, 1), (2, 1, 3, 300), (2, 1, 300, 3))
DEGENERATE_3D = ((3, 1, 1, 1), (3, 1, 1, 2), (3, 1, 2, 1), (3, 2, 1, 1), (3, 2, 2, 2),
                 (3, 1, 5, 7), (3, 5, 1, 7), (3, 5, 7, 1), (3, 2, 1, 4, 5),
                 (3, 2, 2, 3, 4, 5))
# one mesh just beyond kMaxBlocks * kBlock = 262 144 nodes: the grid-stride loop
GRID_STRIDE = ((2, 1, 515, 511), (3, 65, 64, 65))
LINK_SHAPE = (3, 3, 4, 5)
NONFINITE_2D = ((2, 2, 9, 11), (2, 1, 1, 12))
NONFINITE_3D = (3, 2, 5, 6)


def _shape_tag(shape):
  return 'x'.join(str(s) for s in shape)


def _nonfinite_sites(shape):
  """(name, [(y, x), ...]) on the last two axes: a corner, each edge, the interior,
  two adjacent nodes."""
  Y, X = shape[-2:]
  my, mx = Y // 2, X // 2
  sites = [('corner', [(0, 0)]), ('corner_far', [(Y - 1, X - 1)]),
           ('edge_left', [(my, 0)]), ('edge_right', [(my, X - 1)]),
           ('edge_top', [(0, mx)]), ('edge_bottom', [(Y - 1, mx)]),
           ('interior', [(my, mx)]),
           ('adjacent_x', [(my, mx), (my, min(mx + 1, X - 1))])]
  if Y > 1:
    sites.append(('adjacent_y', [(my, mx), (min(my + 1, Y - 1), mx)]))
  return sites


@functools.lru_cache(maxsize=None)
def force_cases():
  """Every force case, by name (the GPU tests and the CPU pin iterate this list)."""
  cs = []
  # degenerate extents; amplitudes from a hundredth of a node spacing to folds
  for shape in DEGENERATE_2D:
    for si, st in enumerate(STRIDES_2D):
      for amp in (0.01, 3.0, 200.0):
        n = f'deg2d_{_shape_tag(shape)}_s{si}_a{amp:g}'
        cs.append(ForceCase(n, _rand(n, shape, amp), 0.1, st, group='degenerate2d'))
  for shape in DEGENERATE_3D:
    for si, st in enumerate(STRIDES_3D):
      for amp in (0.01, 3.0, 200.0):
        n = f'deg3d_{_shape_tag(shape)}_s{si}_a{amp:g}'
        cs.append(ForceCase(n, _rand(n, shape, amp), 0.1, st, group='degenerate3d'))
  # the grid-stride loop
  n = 'grid2d_' + _shape_tag(GRID_STRIDE[0])
  cs.append(ForceCase(n, _rand(n, GRID_STRIDE[0], 3.0), 0.1, STRIDES_2D[1], group='grid'))
  n = 'grid3d_' + _shape_tag(GRID_STRIDE[1])
  cs.append(ForceCase(n, _rand(n, GRID_STRIDE[1], 3.0), 0.1, STRIDES_3D[1], group='grid'))
  n = 'grid3d_links_' + _shape_tag(GRID_STRIDE[1])
  cs.append(ForceCase(n, _rand(n, GRID_STRIDE[1], 3.0), 0.1, STRIDES_3D[1],
                      links=LINKS_3D[::-1], group='grid'))
  # link sets through the generic loop
  xl = _rand('links', LINK_SHAPE, 4.0)
  for i, d in enumerate(LINKS_3D):
    cs.append(ForceCase(f'link_{i}_pos', xl, 0.1, STRIDES_3D[1], links=(d,), group='links'))
    cs.append(ForceCase(f'link_{i}_neg', xl, 0.1, STRIDES_3D[1],
                        links=(tuple(-v for v in d),), group='links'))
  perm = tuple(LINKS_3D[i] for i in _rng('perm').permutation(13))
  cs.append(ForceCase('links_permuted', xl, 0.1, STRIDES_3D[1], links=perm, group='links'))
  cs.append(ForceCase('links_twice', xl, 0.1, STRIDES_3D[1],
                      links=((1, 1, 0), (0, 0, 1), (1, 1, 0)), group='links'))
  cs.append(ForceCase('links_planar_z3', xl, 0.1, STRIDES_3D[1], links=PLANAR, group='links'))
  # The reference accepts a (0, 0, 0) link (mesh.py:241-245 takes dim == 0 on every
  # axis): rest = 0, l0 = 0, k_eff = k * stride_x / 0 = inf, d = x - x + 0 = 0 (NaN at
  # a non-finite node), every term inf * 0 or NaN -> nan_to_num -> 0.
  cs.append(ForceCase('links_zero_beside_x', xl, 0.1, STRIDES_3D[1],
                      links=((0, 0, 0), (1, 0, 0)), group='links'))
  # folds and coincidence
  for nc, shape, st in ((2, (2, 2, 7, 9), (40.0, 40.0)), (3, (3, 3, 5, 6), (40.0, 40.0, 40.0))):
    tag = f'{nc}d'
    n = 'fold_1.5_strides_' + tag
    cs.append(ForceCase(n, (_rng(n).uniform(-1.5, 1.5, shape) * 40.0).astype(f32), 0.1, st,
                        group='folds'))
    x = _rand('coincide_' + tag, shape, 2.0)
    x = np.round(x * 4) / 4          # representable quarter units
    x = x.astype(f32)
    # node (.., 2, 3) exactly on its left neighbour (.., 2, 2): displacement -40 in x
    x[..., 2, 3] = x[..., 2, 2]
    x[0, ..., 2, 3] -= f32(40.0)
    # d_x exactly 0 on the (1, 1) link between (.., 3, 4) and (.., 4, 5)
    x[0, ..., 4, 5] = x[0, ..., 3, 4] - f32(40.0)
    cs.append(ForceCase('coincident_' + tag, x, 0.1, st, group='folds'))
    # a spring of length 1e-15: d = (0, 1e-15[, 0]) on the (1, 0) link of (.., 1, 1)-(.., 1, 2).
    # Lengths below 1e-19 (sub-normal squares) are outside sfm_sqrt's documented contract
    # (csrc/sfm_mesh.hip, comment above sfm_sqrt: "Lengths below 1e-19 ... are outside the
    # contract") and are not tested.
    x = np.zeros(shape, f32)
    x[0, ..., 1, 2] = f32(-40.0)
    x[1, ..., 1, 2] = f32(1e-15)
    cs.append(ForceCase('length_1e-15_' + tag, x, 0.1, st, group='folds'))
  # non-finite positions: in-plane, and through the volumetric generic loop with the planar links
  for shape, links in ((NONFINITE_2D[0], None), (NONFINITE_2D[1], None), (NONFINITE_3D, PLANAR)):
    st = STRIDES_2D[0] if shape[0] == 2 else STRIDES_3D[0]
    base = _rand('nonfinite_' + _shape_tag(shape), shape, 3.0)
    for site, nodes in _nonfinite_sites(shape):
      for vi, val in enumerate((np.nan, np.inf, -np.inf)):
        for comp in (0, 1):
          x = base.copy()
          for (yy, xx) in nodes:
            x[comp, ..., yy, xx] = val
          n = f'nonfinite_{_shape_tag(shape)}_{site}_{("nan", "pinf", "ninf")[vi]}_c{comp}'
          cs.append(ForceCase(n, x, 0.1, st, links=links, group='nonfinite'))
  # magnitudes
  for nc, shape, st in ((2, (2, 1, 5, 6), (40.0, 30.0)), (3, (3, 2, 4, 5), (40.0, 40.0, 30.0))):
    tag = f'{nc}d'
    base = _rand('magnitude_' + tag, shape, 3.0)
    x = base.copy()
    x[0, ..., 1, 1] = f32(3e19)        # squared length overflows float32
    x[1, ..., 3, 4] = f32(1e30)
    cs.append(ForceCase('huge_' + tag, x, 0.1, st, group='magnitude'))
    cs.append(ForceCase('k0_' + tag, base, 0.0, st, group='magnitude'))
    cs.append(ForceCase('k1e-30_' + tag, base, 1e-30, st, group='magnitude'))
    n = 'disp1e-6_' + tag
    cs.append(ForceCase(n, _rand(n, shape, 1e-6), 0.1, (40.0,) * nc, group='magnitude'))
  names = [c.name for c in cs]
  assert len(set(names)) == len(names)
  return tuple(cs)


def force_case(name):
  c = next(c for c in force_cases() if c.name == name)
  c.x.setflags(write=False)
  return c


@functools.lru_cache(maxsize=None)
def force_refs(name, poo):
  """(float64 force, S, float32 form) of a case; computed once, read-only."""
  c = force_case(name)
  want, S = force_bound(c.x, c.k, c.stride, poo, c.links, np.float64)
  form = force(c.x, c.k, c.stride, poo, c.links, np.float32)
  for arr in (want, S, form):
    arr.setflags(write=False)
  return want, S, form


# --- first steps ------------------------------------------------------------
STEP_SHAPES_2D = ((2, 1, 1, 1), (2, 1, 1, 5), (2, 1, 5, 1), (2, 1, 2, 2), (2, 3, 1, 70),
                  (2, 1, 70, 1),
                  (2, 1, 16, 16), (2, 1, 16, 17),      # 256 / 272 nodes: the small-mesh limit
                  (2, 1, 3, 40), (2, 1, 4, 39), (2, 1, 4, 40), (2, 2, 4, 41),   # tiled threshold
                  (2, 2, 17, 63))                      # one row / column past a tile
STEP_STRIDE_2D = (40.0, 30.0)
STEP_STRIDE_3D = (40.0, 40.0, 30.0)
STEP_CONFIGS = ('verlet', 'fire_down', 'fire_up', 'fire_drift')
PREV_KINDS = ('prev', 'prev_nan', 'none')


# Volumetric first steps: each the smallest shape that reaches the edge named.
VOL_SHAPES = (
    (3, 3, 4, 5),          # an interior node with all 26 springs; still mesh_small_kernel
    (3, 5, 7, 9),          # 315 nodes: past the small limit, two workgroups per node kernel
    (3, 1, 3, 4, 5), (3, 2, 3, 4, 5),        # 5-D: drift per x column, G = 51 row groups
    (3, 1, 2, 3, 256), (3, 1, 2, 3, 257),    # drift_cols_kernel at G = 1, two passes over x
    (3, 3, 7, 100), (3, 2, 3, 7, 100),       # z-march at T = 256: several tile columns in x
    (3, 3, 20, 100),       # ... and 5 x 2 tiles (plan_march3d takes 4 x 1 for Y = 7)
    (3, 1, 6, 40), (3, 4, 1, 40), (3, 4, 6, 1))          # z-march with an axis of 1
VOL_LINK_SHAPES = ((3, 3, 4, 5), (3, 5, 7, 9), (3, 2, 3, 4, 5), (3, 1, 2, 3, 257))
# Above 50 000 nodes: fire_down and fire_drift, prev_nan, n = 2, one prefer_orig_order each.
LARGE_SHAPES = (
    (3, 2, 9, 30, 100),    # 540 rows at G = 2: 17 chunks, a second closing batch of 16
    (3, 2, 16, 65, 100),   # 2080 rows: the 64-chunk cap, rows_per no multiple of G * 16
    GRID_STRIDE[1],        # 270 400 nodes: grid-stride step kernels, 1024 partial rows
    GRID_STRIDE[0])        # the same in-plane (multi-launch and tiled)
CHUNK_SHAPES = ((2, 1, 4, 40), (2, 2, 17, 63), (3, 3, 4, 5), (3, 2, 3, 4, 5))
CHUNK_KINDS = ('second_chunk', 'cap_raise3', 'cap_raise2')
SECOND_DT0 = f32(0.3 * 1.1 ** 2)
SECOND_ALPHA0 = f32(0.1 * 0.99 ** 2)


@dataclasses.dataclass(frozen=True, eq=False)
class StepCase:
  name: str
  x: np.ndarray
  v: np.ndarray
  prev: np.ndarray | None
  cfg: Cfg
  force_cap: float
  links: tuple | None = None
  dt0: float | None = None      # the chunk's starting fire_dt / fire_alpha (None: cfg's)
  alpha0: float | None = None

  @property
  def n(self):
    return self.cfg.num_iters


def _step_cfg(kind, stride, n, poo):
  base = dict(dt=0.3, gamma=0.0, k0=0.05, k=0.1, stride=tuple(stride), num_iters=n,
              max_iters=n, stop_v_max=1e-9, dt_max=100.0, prefer_orig_order=poo)
  if kind == 'verlet':
    base.update(fire=False, gamma=0.5, start_cap=10.0, final_cap=10.0)
  else:
    # dt, alpha and the cap move on every step: cap 1 -> 1.5 -> 2 (= final_cap)
    base.update(n_min=0, cap_upscale_every=1, start_cap=1.0, final_cap=2.0, cap_scale=1.5,
                remove_drift=kind == 'fire_drift')
  if kind == 'second_chunk':
    # dt_max * cfg.dt = 0.39 binds on the first growth (0.363 * 1.1 = 0.3993)
    base.update(dt_max=1.3)
  if kind in CHUNK_KINDS:
    # |x - prev| reaches 13.5: with k0 = 0.2 the pull is clipped at every cap from 1 to 2
    # (the first force of a chunk depends on the cap it is taken with)
    base.update(k0=0.2)
  if kind.startswith('cap_raise'):
    # one step per chunk; only the chunk loop raises the cap: 1 -> 1.5 -> 2.  With
    # max_iters = 3 the third chunk runs at final_cap and the loop stops on the cap,
    # with max_iters = 2 it stops on max_iters with the cap raised once more, unused.
    base.update(num_iters=1, max_iters=int(kind[-1]), stop_v_max=1e9, cap_upscale_every=100)
  return Cfg(**base)


@functools.lru_cache(maxsize=None)
def step_case(shape, kind, prev_kind, n, poo, links=None):
  """One first-steps case.  Displacements stay at or below a quarter of the stride."""
  stride = STEP_STRIDE_2D if shape[0] == 2 else STEP_STRIDE_3D
  name = f'step_{_shape_tag(shape)}_{kind}_{prev_kind}_n{n}_p{int(poo)}'
  name += '_links' if links else ''
  rng = _rng(f'step_{_shape_tag(shape)}_{prev_kind}')
  q = 0.25 * min(stride)
  x = rng.uniform(-0.8 * q, 0.8 * q, shape).astype(f32)
  prev = None
  if prev_kind != 'none':
    prev = rng.uniform(-q, q, shape).astype(f32)
    if prev_kind == 'prev_nan':
      prev[..., 0, :] = np.nan
  cfg = _step_cfg(kind, stride, n, poo)
  v = np.zeros(shape, f32)
  cap, dt0, alpha0 = cfg.start_cap, None, None
  if kind == 'fire_up':
    # against the first force: the first update halves dt, zeroes v, resets alpha
    a0 = step(x, v, prev, cfg, cfg.start_cap, 0, np.float64, links)[2]
    v = (-0.5 * a0).astype(f32)
  if kind == 'second_chunk':
    # what a first chunk of two downhill steps hands over: dt and alpha grown twice,
    # the cap at 1.5, a downhill velocity
    cap, dt0, alpha0 = 1.5, SECOND_DT0, SECOND_ALPHA0
    a0 = step(x, v, prev, cfg, cap, 0, np.float64, links)[2]
    v = (0.5 * a0).astype(f32)
  for arr in (x, v) + (() if prev is None else (prev,)):
    arr.setflags(write=False)
  return StepCase(name, x, v, prev, cfg, cap, links, dt0, alpha0)


@functools.lru_cache(maxsize=None)
def step_refs(case):
  """(float64 result tuple, scales dict) of a StepCase; computed once."""
  scales = {}
  want = step(case.x, case.v, case.prev, case.cfg, case.force_cap, case.n, np.float64,
              case.links, scales, dt0=case.dt0, alpha0=case.alpha0)
  for arr in want[:3]:
    arr.setflags(write=False)
  e_kin, v_max = chunk_stats(want[1])
  assert_v_max_margin(v_max, case.cfg.stop_v_max)
  return want, scales


@functools.lru_cache(maxsize=None)
def relax_refs(case):
  """relax_chunks of a cap_raise case in float64; computed once."""
  chunks, e_kin, t = relax_chunks(case, 3)
  for ch in chunks:
    for arr in ch[:3]:
      arr.setflags(write=False)
  return chunks, e_kin, t


def step_cases_2d(shape):
  return [step_case(shape, kind, pk, n, poo)
          for kind in STEP_CONFIGS for pk in PREV_KINDS for n in (1, 2, 3)
          for poo in (False, True)]


STEP_LINKS_3D = tuple(LINKS_3D[i] for i in (7, 2, 11, 0, 5, 12, 3, 9, 1, 10, 4, 8, 6))


def step_cases_3d(shape, links=None):
  return [step_case(shape, kind, pk, n, poo, links)
          for kind in ('verlet', 'fire_down') for pk in ('prev_nan', 'none') for n in (1, 2)
          for poo in (False, True)]


def step_cases_vol(shape, links=None):
  """The full in-plane matrix on a volumetric shape."""
  return [step_case(shape, kind, pk, n, poo, links)
          for kind in STEP_CONFIGS for pk in PREV_KINDS for n in (1, 2, 3)
          for poo in (False, True)]


def step_cases_large(shape):
  poo = bool(LARGE_SHAPES.index(shape) % 2)
  return [step_case(shape, kind, 'prev_nan', 2, poo) for kind in ('fire_down', 'fire_drift')]


def second_chunk_cases(shape, links=None):
  return [step_case(shape, 'second_chunk', pk, n, poo, links)
          for pk in ('prev', 'prev_nan') for n in (1, 2) for poo in (False, True)]


def cap_raise_cases(shape, links=None):
  return [step_case(shape, kind, 'prev', 1, poo, links)
          for kind in ('cap_raise3', 'cap_raise2') for poo in (False, True)]


def uphill_end_cases(shape, links=None):
  """Chunks whose last step is uphill: v is gated to exactly 0."""
  return [step_case(shape, 'fire_up', pk, 1, poo, links)
          for pk in PREV_KINDS for poo in (False, True)]


def step_cases():
  """Every single-chunk case (the cap_raise cases run through relax_chunks)."""
  out = []
  for shape in STEP_SHAPES_2D:
    out += step_cases_2d(shape)
  for shape in DEGENERATE_3D:
    out += step_cases_3d(shape)
    out += step_cases_3d(shape, STEP_LINKS_3D)
  for shape in VOL_SHAPES:
    out += step_cases_vol(shape)
  for shape in VOL_LINK_SHAPES:
    out += step_cases_vol(shape, STEP_LINKS_3D)
  for shape in LARGE_SHAPES:
    out += step_cases_large(shape)
  for shape in CHUNK_SHAPES:
    out += second_chunk_cases(shape)
    if shape[0] == 3:
      out += second_chunk_cases(shape, STEP_LINKS_3D)
  return out


def relax_cases():
  out = []
  for shape in CHUNK_SHAPES:
    out += cap_raise_cases(shape)
    if shape[0] == 3:
      out += cap_raise_cases(shape, STEP_LINKS_3D)
  return out


# ---------------------------------------------------------------------------
# checks shared by the GPU tests and the CPU pin
# ---------------------------------------------------------------------------
def units(got, want, scale):
  """Largest |got - want| in units of 2^-24 * scale (scale: array or number; where
  it is 0 the two must be equal and the element counts as 0 units, else inf)."""
  got = np.asarray(got, np.float64)
  want = np.asarray(want, np.float64)
  with np.errstate(all='ignore'):
    diff = np.abs(got - want)
    diff = np.where((got == want) | (np.isnan(got) & np.isnan(want)), 0.0, diff)
    diff = np.where(np.isnan(diff), np.inf, diff)
    scale = np.broadcast_to(np.asarray(scale, np.float64), diff.shape)
    safe = np.where(scale > 0, scale, 1.0)
    u = np.where(diff == 0, 0.0, np.where(scale > 0, diff / (EPS * safe), np.inf))
  return float(u.max()) if u.size else 0.0


def check_force(got, name, poo, factor=DEV_FACTOR, bitwise=True):
  """The assertions on one force result (float32 array of the case's shape)."""
  want, S, form = force_refs(name, poo)
  got = np.asarray(got)
  assert got.dtype == np.float32 and got.shape == want.shape, name
  assert not np.isnan(want).any() and np.array_equal(np.isnan(got), np.isnan(want)), name
  # exact zeros are those of the float32 form (a missing spring, coincident nodes, a
  # zeroed term, a mesh at rest: float32 gives 0 where the float64 statement of the same
  # inputs keeps a rounding residue, and a float64 sum may cancel where float32 leaves
  # an ulp); a node with no live spring (S = 0) is exactly 0 in all three
  assert np.array_equal(got == 0, form == 0), name
  assert (got[:, S == 0] == 0).all() and (want[:, S == 0] == 0).all(), name
  u = units(got, want, S[None])
  assert u <= factor * K_F, (name, poo, u)
  if bitwise:
    assert np.array_equal(got, form), (name, poo, units(got, form, S[None]))
  return u


def check_state(got, want, scales, what, factor=DEV_FACTOR):
  """x, v, a (the first three of `got`) within factor x K_S of the float64 ones.
  Returns the units measured."""
  out = {}
  for i, key in enumerate('xva'):
    g = np.asarray(got[i])
    assert g.shape == want[i].shape and not np.isnan(g).any(), (what, key)
    out[key] = units(g, want[i], scales[key])
    assert out[key] <= factor * K_S[key], (what, key, out[key])
  return out


def check_step(got, case, what='', factor=DEV_FACTOR):
  """The assertions on one chunk's result (x, v, a[, dt, alpha, n_pos, cap]) against the
  float64 statement: the arrays within factor x K_S, the FIRE scalars equal."""
  want, scales = step_refs(case)
  u = check_state(got, want, scales, (what, case.name), factor)
  if case.cfg.fire:
    # dt, alpha, n_pos, cap: float32 like fire_next, compared with ==
    assert tuple(got[3:7]) == tuple(want[3:]), (what, case.name, got[3:7], want[3:])
  else:
    assert len(got) == 3 or got[3] is None, (what, case.name)
  return u


def stat_bounds(v64, scale_v):
  """(e_kin, v_max, allowed |error| of e_kin, of v_max) for a chunk whose float64
  velocities are `v64`.  delta = DEV_FACTOR K_S['v'] 2^-24 scale(v) is what a device
  velocity component may be off by.  The node norm is 1-Lipschitz in the components
  (sqrt(C) delta), and its square, sum and root round twice at most (2 x 2^-24 v_max);
  |v + d|^2 - |v|^2 <= 2 |v| d + d^2 per component, and the float32 sum of the terms
  is allowed DEV_FACTOR x K_E, K_E being the error of the worst (sequential) order."""
  v64 = np.asarray(v64, np.float64)
  e_kin, v_max = chunk_stats(v64)
  delta = DEV_FACTOR * K_S['v'] * EPS * scale_v
  tol_v = np.sqrt(v64.shape[0]) * delta + 2 * EPS * v_max
  tol_e = float(np.sum(2 * np.abs(v64) * delta + delta * delta)) + DEV_FACTOR * K_E * EPS * e_kin
  return e_kin, v_max, tol_e, tol_v


def check_stats(e_kin, v_max, v64, scale_v, what=''):
  """The assertions on a chunk's statistics (what relax_mesh stops on).  Where the
  float64 velocities are all 0 (a chunk that ends uphill), both are exactly 0."""
  want_e, want_v, tol_e, tol_v = stat_bounds(v64, scale_v)
  e_kin, v_max = float(e_kin), float(v_max)
  assert np.isfinite(e_kin) and np.isfinite(v_max), (what, e_kin, v_max)
  if want_v == 0:
    assert e_kin == 0.0 and v_max == 0.0, (what, e_kin, v_max)
    return 0.0, 0.0
  assert abs(e_kin - want_e) <= tol_e, (what, 'e_kin', e_kin, want_e, tol_e)
  assert abs(v_max - want_v) <= tol_v, (what, 'v_max', v_max, want_v, tol_v)
  return abs(e_kin - want_e) / tol_e, abs(v_max - want_v) / tol_v


def check_case_stats(e_kin, v_max, case, what=''):
  want, scales = step_refs(case)
  return check_stats(e_kin, v_max, want[1], scales['v'], (what, case.name))


def check_relax(x, e_kin, t, case, what='', starts=None, ends=None):
  """relax_mesh on a cap_raise case against relax_chunks: t and the number of chunks
  equal, every e_kin[i] within its bound, the final positions within DEV_FACTOR x
  K_S['x'].  `starts` / `ends`: the (dt, alpha, cap) every chunk was started with and
  the (dt, alpha, n_pos, cap) it returned, compared with ==."""
  chunks, want_e, want_t = relax_refs(case)
  what = (what, case.name)
  assert t == want_t and len(e_kin) == len(want_e), (what, t, want_t, len(e_kin))
  for i, ch in enumerate(chunks):
    want_v, tol_e = ch[5], stat_bounds(ch[1], ch[6]['v'])[2]
    assert np.isfinite(e_kin[i]) and abs(e_kin[i] - want_e[i]) <= tol_e, \
        (what, i, e_kin[i], want_e[i], tol_e)
    if starts is not None:
      assert tuple(f32(s) for s in starts[i]) == tuple(ch[7]), (what, i, starts[i], ch[7])
    if ends is not None:
      assert tuple(ends[i]) == tuple(ch[3]), (what, i, ends[i], ch[3])
  last = chunks[-1]
  x = np.asarray(x)
  assert not np.isnan(x).any(), what
  u = units(x, last[0], last[6]['x'])
  assert u <= DEV_FACTOR * K_S['x'], (what, 'x', u)
  return u
