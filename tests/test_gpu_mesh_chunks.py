"""Edge tests for what a chunk of mesh steps hands on: volumetric first steps on real
volumes (an interior node with 26 springs, more than one workgroup, 5-D states with the
drift per x column, the z-march tilings, a mesh past kMaxBlocks * kBlock nodes), the
chunk statistics e_kin / v_max that relax_mesh stops on, and the carry-over of fire_dt /
fire_alpha / force_cap into a second chunk -- against tests/mesh_ref64.py (pinned on the
CPU by tests/test_mesh_ref64.py), with the helpers of tests/test_gpu_mesh_edges.py.

A chunk runs through mesh._run_chunk, the one call behind velocity_verlet and relax_mesh,
so that one run gives the state, the FIRE scalars and the statistics; the carry-over
tests go through the public velocity_verlet and relax_mesh.  Every case asserts through
sfm_debug_mesh_plan which integrator ran.
"""
import numpy as np
import pytest

from tests import mesh_ref64 as ref
from tests.test_gpu_mesh_edges import (PATHS, _can_take, _config, _expect_plan, _mesh_force,
                                       _switches)
from tests.util import mesh_plan

pytestmark = pytest.mark.gpu
f32 = np.float32


# ---------------------------------------------------------------------------
# paths
# ---------------------------------------------------------------------------
def _march(t, zc):
  return {'SFM_MESH_MARCH3D': 1, 'SFM_MESH_MARCH3D_T': t, 'SFM_MESH_MARCH3D_ZC': zc}


# name -> (switches, links)
VOL_PATHS = {
    'per_node': ({}, None),
    'small': ({'SFM_MESH_SMALL': 1}, None),
    'links': ({}, ref.STEP_LINKS_3D),
}
for _t in (256, 512, 1024):
  VOL_PATHS[f'march{_t}'] = (_march(_t, 0), None)
  VOL_PATHS[f'march{_t}_zc2'] = (_march(_t, 2), None)


def _march_plan(t, shape, zc, cus):
  """plan_march3d (csrc/sfm_mesh.hip) restated for one T: (ntx, nty, run, grid), or None
  where no tile of T threads holds three columns (txh * 3 <= T)."""
  b = int(np.prod(shape[1:-3], dtype=np.int64))
  z, y, x = shape[-3:]
  best = None
  for ntx in range(1, x + 1):
    cxw = -(-x // ntx)
    txh = cxw + 2
    if txh * 3 > t:
      continue
    rows = t // txh
    nty = (y + rows - 2) // (rows - 1)
    if best is None or ntx * nty < best[0] * best[1]:
      best = (ntx, nty)
    if cxw <= 8:
      break
  if best is None:
    return None
  per_cu = max(1, 160 * 1024 // (36 * t * 4))
  slots = min(cus * per_cu, 1024)
  planes = b * best[0] * best[1] * z
  run = zc if zc > 0 else max(-(-planes // slots), min(8, z))
  if -(-planes // run) > 1024:
    run = -(-planes // 1024)
  return best + (run, -(-planes // run))


def _vol_shape_can_take(path, shape):
  """The planner's conditions restated: 256 nodes for mesh_small_kernel, txh * 3 <= T for
  the z-march; the generic link loop runs on the shapes that have a links case list."""
  if path == 'small':
    return int(np.prod(shape[1:])) <= 256
  if path == 'links':
    return shape in ref.VOL_LINK_SHAPES
  if path.startswith('march'):
    return _march_plan(int(path[5:].split('_')[0]), shape, 0, 256) is not None
  return True


def _vol_can_take(path, case):
  # (a 5-D state that removes drift does so per x column, which mesh_small_kernel does
  # not take)
  column_drift = case.x.ndim == 5 and case.cfg.remove_drift
  return _vol_shape_can_take(path, case.x.shape) and not (path == 'small' and column_drift)


def _expect_vol(path, case, info):
  assert info.persist_tile == 0 and not info.tiled, (path, case.name)
  assert bool(info.small) == (path == 'small'), (path, case.name)
  if not path.startswith('march'):
    assert info.march_t == 0, (path, case.name)
    return
  import torch
  t = int(path[5:].split('_')[0])
  cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
  want = _march_plan(t, case.x.shape, 2 if path.endswith('_zc2') else 0, cus)
  got = (info.march_ntx, info.march_nty, info.march_run, info.march_grid)
  assert info.march_t == t and got == want, (path, case.name, info.march_t, got, want)


def _paths(shape):
  """[(name, switches, links, expect)] of every integrator a shape can run on."""
  if shape[0] == 2:
    return [(p, PATHS[p], None, _expect_plan) for p in PATHS if _can_take(p, shape)]
  return [(p,) + VOL_PATHS[p] + (_expect_vol,) for p in VOL_PATHS
          if _vol_shape_can_take(p, shape)]


def _takes(path, case):
  if case.x.shape[0] == 3:
    return _vol_can_take(path, case)
  # (the plain persistent kernel is the path without _spec)
  return not path.endswith('_spec') or (case.cfg.fire and not case.cfg.remove_drift)


def _chunk(case, path, opts, expect):
  """One chunk on the device: ((x, v, a[, dt, alpha, n_pos, cap]), (e_kin, v_max))."""
  from sofima_amd import _dev, mesh
  cfg = _config(case)
  force = _mesh_force(case)
  dev = _dev.device()
  prev = None if case.prev is None else case.prev.copy()   # (the case's arrays are read-only)
  with _switches(opts):
    expect(path, case, mesh_plan(case.x.copy(), prev, cfg, force))
    x_t = _dev.as_device_f32(case.x.copy(), dev)
    v_t = _dev.as_device_f32(case.v.copy(), dev)
    prev_t = None if prev is None else _dev.as_device_f32(prev, dev)
    a_t, fire, stats = mesh._run_chunk(x_t, v_t, prev_t, cfg, case.force_cap, case.dt0,
                                       case.alpha0, mesh._resolve_force(force))
  out = tuple(t.cpu().numpy() for t in (x_t, v_t, a_t))
  if cfg.fire:
    out += (f32(fire.dt), f32(fire.alpha), int(fire.n_pos), f32(fire.cap))
  return out, (f32(stats.e_kin), f32(stats.v_max))


_BASE = {}


def _base(case):
  """A case on the per-node kernels (advance_kernel / integrate_kernel), once."""
  if case.name not in _BASE:
    path = 'multi' if case.x.shape[0] == 2 else 'per_node'
    expect = _expect_plan if case.x.shape[0] == 2 else _expect_vol
    _BASE[case.name] = _chunk(case, path, {}, expect)[0]
  return _BASE[case.name]


class _Worst:
  """The largest device error per quantity, printed for information."""

  def __init__(self, what):
    self.what, self.u = what, {}

  def add(self, **kw):
    for k, v in kw.items():
      self.u[k] = max(self.u.get(k, 0.0), v)

  def show(self, ran):
    print('%s: %d cases, worst %s' % (self.what, ran,
                                      ', '.join('%s %.3g' % kv for kv in sorted(self.u.items()))))


def _check_chunk(case, path, opts, expect, worst, bitwise):
  """One case on one path: the state against float64 (or bit for bit against the
  per-node kernels), the scalars equal, the statistics within their bounds."""
  got, (e_kin, v_max) = _chunk(case, path, opts, expect)
  if bitwise and not case.cfg.remove_drift:
    base = _base(case)
    for i, key in enumerate('xva'):
      assert np.array_equal(got[i], base[i]), (path, case.name, key,
                                               ref.units(got[i], base[i], np.abs(base[i]).max()))
    assert tuple(got[3:]) == tuple(base[3:]), (path, case.name, got[3:], base[3:])
  u = ref.check_step(got, case, path)
  ue, uv = ref.check_case_stats(e_kin, v_max, case, path)
  worst.add(**u, e_kin_of_bound=ue, v_max_of_bound=uv)


# ---------------------------------------------------------------------------
# volumetric first steps
# ---------------------------------------------------------------------------
_VOL = [(s, p) for s in ref.VOL_SHAPES for p in VOL_PATHS if _vol_shape_can_take(p, s)]
_ids = lambda params: ['%s-%s' % ('x'.join(map(str, s)), p) for s, p in params]


@pytest.mark.parametrize('shape,path', _VOL, ids=_ids(_VOL))
def test_first_steps_volumetric_paths(gpu, shape, path):
  """One to three steps of damped Verlet and of FIRE (downhill, started uphill, with
  drift removal -- global on a 4-D state, per x column on a 5-D one), with prev, with a
  NaN row in prev and without, on one volumetric integrator.  The per-node kernels and
  every drift-removing case within 4 K_S of float64 with equal scalars; the generic link
  loop too (the reference adds the links in the order given, so a permuted set is another
  float32 sum than the default one: its own float64 statement is the reference); every
  other path bit for bit the per-node result.  Statistics within their bounds."""
  opts, links = VOL_PATHS[path]
  worst = _Worst(f'{path} {shape}')
  ran = 0
  for case in ref.step_cases_vol(shape, links):
    if not _vol_can_take(path, case):
      continue
    _check_chunk(case, path, opts, _expect_vol, worst, path not in ('per_node', 'links'))
    ran += 1
  worst.show(ran)
  column_drift = path == 'small' and len(shape) == 5
  assert ran >= (54 if column_drift else 72)


_LARGE = [(s, p) for s in ref.LARGE_SHAPES if s[0] == 3
          for p in ('per_node', 'march256', 'march256_zc2', 'march512', 'march1024')] + \
         [(s, p) for s in ref.LARGE_SHAPES if s[0] == 2 for p in ('multi', 'tiled', 'tiled_packed')]


@pytest.mark.parametrize('shape,path', _LARGE, ids=_ids(_LARGE))
def test_fire_step_pair_on_large_meshes(gpu, shape, path):
  """Two FIRE steps, without and with drift removal, on 540 and 2080 rows of 100-node
  columns (drift_cols_kernel with 17 and with 64 chunks) and past kMaxBlocks * kBlock
  nodes (grid-stride step kernels, 1024 rows of partial sums)."""
  if shape[0] == 2:
    assert _can_take(path, shape[:1] + shape[-3:])
    opts, expect = PATHS[path], _expect_plan
  else:
    opts, expect = VOL_PATHS[path][0], _expect_vol
  worst = _Worst(f'{path} {shape}')
  cases = ref.step_cases_large(shape)
  for case in cases:
    _check_chunk(case, path, opts, expect, worst, path not in ('per_node', 'multi'))
  worst.show(len(cases))
  assert [c.cfg.remove_drift for c in cases] == [False, True]


# ---------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------
_INPLANE_CHUNK = [(s, p) for s in ref.CHUNK_SHAPES if s[0] == 2 for p in PATHS if _can_take(p, s)]


@pytest.mark.parametrize('shape,path', _INPLANE_CHUNK, ids=_ids(_INPLANE_CHUNK))
def test_chunk_statistics_inplane(gpu, shape, path):
  """e_kin and v_max of a chunk of one to three steps on every in-plane integrator
  (finish_kernel + stats_kernel, persist_write_back, behind mesh_small_kernel): formed
  after the last step's gate and drift, exactly 0 for a chunk that ends uphill."""
  worst = _Worst(f'{path} {shape}')
  ran = zeros = 0
  for case in ref.step_cases_2d(shape):
    if not _takes(path, case):
      continue
    _check_chunk(case, path, PATHS[path], _expect_plan, worst, path != 'multi')
    zeros += ref.step_refs(case)[0][1].any() == 0
    ran += 1
  worst.show(ran)
  assert ran >= 36 and zeros >= 6


_ALL_CHUNK = [(s, p[0]) for s in ref.CHUNK_SHAPES for p in _paths(s)]


def _path_of(shape, name):
  return next(p for p in _paths(shape) if p[0] == name)


@pytest.mark.parametrize('shape,path', _ALL_CHUNK, ids=_ids(_ALL_CHUNK))
def test_relax_mesh_single_chunk(gpu, shape, path):
  """The public relax_mesh with max_iters == num_iters: one chunk from v = 0; t, the one
  e_kin within its bound, the positions those of the chunk."""
  from sofima_amd import mesh
  _, opts, links, expect = _path_of(shape, path)
  cases = [ref.step_case(shape, kind, pk, n, False, links)
           for kind in ('verlet', 'fire_down', 'fire_drift') for pk in ('prev', 'none')
           for n in (1, 3)]
  ran = 0
  for case in cases:
    if not _takes(path, case):
      continue
    prev = None if case.prev is None else case.prev.copy()
    with _switches(opts):
      expect(path, case, mesh_plan(case.x.copy(), prev, _config(case), _mesh_force(case)))
      x, e_kin, t = mesh.relax_mesh(case.x.copy(), prev, _config(case), _mesh_force(case))
    want, scales = ref.step_refs(case)
    assert t == case.n and len(e_kin) == 1, (path, case.name, t, e_kin)
    e_want, _, tol_e, _ = ref.stat_bounds(want[1], scales['v'])
    assert np.isfinite(e_kin[0]) and abs(e_kin[0] - e_want) <= tol_e, \
        (path, case.name, e_kin[0], e_want, tol_e)
    u = ref.units(np.array(x), want[0], scales['x'])
    assert u <= ref.DEV_FACTOR * ref.K_S['x'], (path, case.name, u)
    ran += 1
  assert ran >= (4 if path.endswith('_spec') else 8)


@pytest.mark.parametrize('shape,path', _ALL_CHUNK, ids=_ids(_ALL_CHUNK))
def test_v_max_keeps_a_nan_velocity(gpu, shape, path):
  """A NaN velocity (reachable from relax_mesh once squares overflow float32: a / |a|
  with |a| = inf is 0, times |v| = inf) makes v_max and e_kin NaN like the reference's
  jnp.max / jnp.sum, wherever the node sits in the reduction."""
  import dataclasses
  _, opts, links, expect = _path_of(shape, path)
  case = ref.step_case(shape, 'verlet', 'prev', 1, False, links)
  nodes = int(np.prod(shape[1:]))
  for node in (0, nodes // 2, nodes - 1):
    v = case.v.copy()
    v.reshape(shape[0], -1)[1, node] = np.nan
    _, (e_kin, v_max) = _chunk(dataclasses.replace(case, v=v), path, opts, expect)
    assert np.isnan(v_max) and np.isnan(e_kin), (path, node, e_kin, v_max)


# ---------------------------------------------------------------------------
# carry-over between chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('shape,path', _ALL_CHUNK, ids=_ids(_ALL_CHUNK))
def test_second_chunk(gpu, shape, path):
  """velocity_verlet started as a second chunk (fire_dt and fire_alpha grown twice, the
  cap at 1.5, a downhill velocity): n_pos restarts at 0, the first force is taken with
  the carried cap, and dt is limited by dt_max * config.dt = 0.39, not by the carried
  dt (0.3993)."""
  from sofima_amd import mesh
  _, opts, links, expect = _path_of(shape, path)
  worst = _Worst(f'{path} {shape}')
  cases = ref.second_chunk_cases(shape, links)
  for case in cases:
    cfg, force = _config(case), _mesh_force(case)
    with _switches(opts):
      expect(path, case, mesh_plan(case.x.copy(), case.prev.copy(), cfg, force))
      out = mesh.velocity_verlet(case.x.copy(), case.v.copy(), case.prev.copy(), cfg,
                                 force_cap=case.force_cap, fire_dt=case.dt0,
                                 fire_alpha=case.alpha0, mesh_force=force)
    got = tuple(np.array(t) for t in out[:3]) + tuple(out[3:])
    assert got[3] == f32(1.3 * 0.3) and got[5] == case.n, (path, case.name, got[3:])
    worst.add(**ref.check_step(got, case, path))
  worst.show(len(cases))
  assert len(cases) == 8


@pytest.mark.parametrize('shape,path', _ALL_CHUNK, ids=_ids(_ALL_CHUNK))
def test_cap_raise(gpu, shape, path):
  """relax_mesh with one step per chunk and a stop_v_max nothing exceeds: the chunk loop
  raises the cap 1 -> 1.5 -> 2 and stops on the cap after the third chunk (max_iters 3)
  or on max_iters after the second; t, the number of chunks, every e_kin and the final
  positions against the reference's loop, and -- driving mesh._relax_loop by hand --
  the dt, alpha and cap every chunk starts with and returns."""
  from sofima_amd import _dev, mesh
  _, opts, links, expect = _path_of(shape, path)
  cases = ref.cap_raise_cases(shape, links)
  for case in cases:
    cfg, force = _config(case), _mesh_force(case)
    with _switches(opts):
      expect(path, case, mesh_plan(case.x.copy(), case.prev.copy(), cfg, force))
      x, e_kin, t = mesh.relax_mesh(case.x.copy(), case.prev.copy(), cfg, force)
      ref.check_relax(np.array(x), e_kin, t, case, path)

      dev = _dev.device()
      x_t = _dev.as_device_f32(case.x.copy(), dev)
      v_t = _dev.as_device_f32(case.v.copy(), dev)
      prev_t = _dev.as_device_f32(case.prev.copy(), dev)
      starts, ends, v_maxes = [], [], []

      def run_chunk(dt, alpha, cap):
        starts.append((dt, alpha, cap))
        _, fire, stats = mesh._run_chunk(x_t, v_t, prev_t, cfg, cap, dt, alpha,
                                         mesh._resolve_force(force))
        ends.append((f32(fire.dt), f32(fire.alpha), int(fire.n_pos), f32(fire.cap)))
        v_maxes.append(float(stats.v_max))
        return ends[-1] + (float(stats.e_kin), float(stats.v_max))

      e_kin2, t2 = mesh._relax_loop(cfg, run_chunk)
    assert e_kin2 == e_kin and t2 == t, (path, case.name)
    ref.check_relax(x_t.cpu().numpy(), e_kin2, t2, case, path, starts, ends)
    assert np.array_equal(x_t.cpu().numpy(), np.array(x)), (path, case.name)
    for ch, v_max in zip(ref.relax_refs(case)[0], v_maxes):
      ref.check_stats(ch[4], v_max, ch[1], ch[6]['v'], (path, case.name))
  assert len(cases) == 4
