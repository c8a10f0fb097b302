"""Edge tests for the spring-mesh kernels: the spring law element-wise and the first
one to three steps of every integrator, against tests/mesh_ref64.py (the float64
statement of the operation and its float32 form; pinned on the CPU by
tests/test_mesh_ref64.py).

Forces: |got - float64| <= 4 K_F 2^-24 S element-wise, the NaN / zero patterns, and
bit equality with the float32 form (the kernels promise the reference's operation
order without contraction; NumPy's float32 sqrt and / are correctly rounded like
sfm_sqrt / sfm_div).  Steps: the multi-launch path within 4 K_S of float64 with equal
FIRE scalars; every other path bit-identical to it (same floats per node, FIRE reads
the sign of the power only), with drift removal (the sums enter the state) within
4 K_S of float64.  Every path-specific test asserts through sfm_debug_mesh_plan that
the path it names is the one the planner takes.
"""
import contextlib
import dataclasses
import functools

import numpy as np
import pytest

from tests import mesh_ref64 as ref
from tests.util import mesh_plan

pytestmark = pytest.mark.gpu

_FORCE_NAMES = [c.name for c in ref.force_cases()]


# ---------------------------------------------------------------------------
# forces
# ---------------------------------------------------------------------------
def _device_force(c, poo):
  from sofima_amd import mesh
  x = c.x.copy()                    # (the case's array is read-only)
  if c.ncomp == 2:
    return np.array(mesh.inplane_force(x, c.k, c.stride, poo))
  links = mesh.MESH_LINK_DIRECTIONS if c.links is None else c.links
  return np.array(mesh.elastic_mesh_3d(x, c.k, c.stride, poo, links=links))


@pytest.mark.parametrize('name', _FORCE_NAMES)
def test_force_case(gpu, name):
  """force_kernel (in-plane loop, unrolled default-link stencil, generic link loop)
  on one case of mesh_ref64.force_cases(), both prefer_orig_order values."""
  c = ref.force_case(name)
  for poo in (False, True):
    got = _device_force(c, poo)
    u = ref.check_force(got, name, poo)
    print(f'{name} poo={int(poo)}: {u:.3g} units of 2^-24 S (allowed {4 * ref.K_F:.3g})')
    if c.ncomp == 2 and c.x.shape[-2:] == (1, 1):
      assert got.view(np.uint32).max() == 0, name        # +0 in every bit


def test_negated_link_is_the_same_springs(gpu):
  """A link and its negation name the same springs (the two ends swap roles, d changes
  sign): each force is within the bound of the statement, so the two agree within
  twice the bound."""
  for i in range(13):
    for poo in (False, True):
      pos = _device_force(ref.force_case(f'link_{i}_pos'), poo)
      neg = _device_force(ref.force_case(f'link_{i}_neg'), poo)
      S = ref.force_refs(f'link_{i}_pos', poo)[1]
      assert ref.units(neg, pos, S[None]) <= 2 * ref.DEV_FACTOR * ref.K_F, (i, poo)
      assert np.array_equal(neg == 0, pos == 0)


def test_zero_link_adds_exactly_nothing(gpu):
  """The reference accepts a (0, 0, 0) link (mesh.py:241-245; rest 0, k_eff = inf, every
  term NaN -> 0): beside (1, 0, 0) it leaves that link's force bit for bit."""
  for poo in (False, True):
    pair = _device_force(ref.force_case('links_zero_beside_x'), poo)
    alone = _device_force(ref.force_case('link_0_pos'), poo)
    assert np.array_equal(pair.view(np.uint32), alone.view(np.uint32))


# ---------------------------------------------------------------------------
# first steps
# ---------------------------------------------------------------------------
_OFF = {'SFM_MESH_PERSISTENT': 0, 'SFM_MESH_SMALL': 0, 'SFM_MESH_TILED': 0, 'SFM_MESH_PACK': 0,
        'SFM_MESH_SPECULATE': 0, 'SFM_MESH_MARCH3D': 0}
PATHS = {
    'multi': {},
    'small': {'SFM_MESH_SMALL': 1, 'SFM_MESH_TILED': 1},
    'tiled': {'SFM_MESH_TILED': 1},
    'tiled_packed': {'SFM_MESH_TILED': 1, 'SFM_MESH_PACK': 1},
    'persist16': {'SFM_MESH_PERSISTENT': 1, 'SFM_MESH_TILE': 16},
    'persist16_spec': {'SFM_MESH_PERSISTENT': 1, 'SFM_MESH_TILE': 16, 'SFM_MESH_SPECULATE': 1},
    'persist32': {'SFM_MESH_PERSISTENT': 1, 'SFM_MESH_TILE': 32},
    'persist32_spec': {'SFM_MESH_PERSISTENT': 1, 'SFM_MESH_TILE': 32, 'SFM_MESH_SPECULATE': 1},
}


@contextlib.contextmanager
def _switches(opts):
  from sofima_amd import _abi
  with contextlib.ExitStack() as stack:
    for k, v in {**_OFF, **opts}.items():
      stack.enter_context(_abi.option(k, v))
    yield


def _can_take(path, shape):
  """The planner's thresholds (plan_chunk / plan_tiles in csrc/sfm_mesh.hip), restated:
  256 nodes for mesh_small_kernel, X >= 40 and Y >= 4 for the tiled step, a last tile
  column of at most 30 nodes over at least two tile rows for packing."""
  z, y, x = shape[1:]
  if path == 'small':
    return z * y * x <= 256
  if path in ('tiled', 'tiled_packed'):
    tiled = x >= 40 and y >= 4
    rem = x % 62
    return tiled and (path == 'tiled' or (rem and rem + 2 <= 32 and -(-y // 16) >= 2))
  return True


def _expect_plan(path, case, info):
  """Asserts that `info` names `path`; skips where only the device rules it out."""
  spec = case.cfg.fire and not case.cfg.remove_drift
  if path.startswith('persist'):
    t = int(path[7:9])
    if info.persist_tile != t:
      import torch
      z, y, x = case.x.shape[1:]
      nw = z * -(-y // t) * -(-x // t)
      cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
      assert nw > min(cus, 256), (path, case.name, info.persist_tile)
      pytest.skip(f'{nw} workgroups of tile {t} do not fit the {cus} CUs of this device')
    assert bool(info.persist_spec) == (path.endswith('_spec') and spec), (path, case.name)
    return
  assert info.persist_tile == 0 and info.march_t == 0, (path, case.name)
  assert bool(info.small) == (path == 'small'), (path, case.name)
  assert bool(info.tiled) == path.startswith('tiled'), (path, case.name)
  if path.startswith('tiled'):
    assert info.fused and bool(info.packed) == (path == 'tiled_packed'), (path, case.name)


def _config(case):
  from sofima_amd import mesh
  return mesh.IntegrationConfig(**dataclasses.asdict(case.cfg))


def _mesh_force(case):
  from sofima_amd import mesh
  if case.x.shape[0] == 2:
    return mesh.inplane_force
  if case.links is None:
    return mesh.elastic_mesh_3d
  return functools.partial(mesh.elastic_mesh_3d, links=case.links)


def _run(case, path, opts=None, expect=_expect_plan):
  from sofima_amd import mesh
  cfg = _config(case)
  force = _mesh_force(case)
  prev = None if case.prev is None else case.prev.copy()   # (the case's arrays are read-only)
  with _switches(PATHS[path] if opts is None else opts):
    expect(path, case, mesh_plan(case.x.copy(), prev, cfg, force))
    out = mesh.velocity_verlet(case.x.copy(), case.v.copy(), prev, cfg, case.force_cap,
                               mesh_force=force)
  return tuple(np.array(t) for t in out[:3]) + tuple(out[3:])


_MULTI = {}


def _multi(case):
  """The multi-launch (advance_kernel / integrate_kernel) result of a case, once."""
  if case.name not in _MULTI:
    _MULTI[case.name] = _run(case, 'multi')
  return _MULTI[case.name]


def _check_vs_float64(got, case, what):
  # x, v, a within DEV_FACTOR x K_S; dt, alpha, n_pos, cap compared with ==
  ref.check_step(got, case, what)
  assert len(got) == (7 if case.cfg.fire else 3)


_SHAPE_PATHS = [(s, p) for s in ref.STEP_SHAPES_2D for p in PATHS if _can_take(p, s)]


@pytest.mark.parametrize('shape,path', _SHAPE_PATHS,
                         ids=['%s-%s' % ('x'.join(map(str, s)), p) for s, p in _SHAPE_PATHS])
def test_first_steps_inplane(gpu, shape, path):
  """One to three steps of damped Verlet and of FIRE (downhill with every scalar moving,
  started uphill, with drift removal), with prev, with a NaN row in prev and without,
  on one in-plane integrator."""
  ran = 0
  for case in ref.step_cases_2d(shape):
    speculates = case.cfg.fire and not case.cfg.remove_drift
    if path.endswith('_spec') and not speculates:
      continue                      # the plain persistent kernel: the path without _spec
    got = _run(case, path)
    ran += 1
    if path == 'multi' or case.cfg.remove_drift:
      _check_vs_float64(got, case, path)
      continue
    base = _multi(case)
    for i, key in enumerate('xva'):
      assert np.array_equal(got[i], base[i]), (path, case.name, key)
    assert tuple(got[3:]) == tuple(base[3:]), (path, case.name)
  assert ran >= 36


_VOL_PATHS = {
    'per_node': ({}, None),
    'small': ({'SFM_MESH_SMALL': 1}, None),
    'links': ({}, ref.STEP_LINKS_3D),
}


@pytest.mark.parametrize('path', list(_VOL_PATHS))
@pytest.mark.parametrize('shape', ref.DEGENERATE_3D, ids=lambda s: 'x'.join(map(str, s)))
def test_first_steps_volumetric(gpu, shape, path):
  """The degenerate volumes through one and two steps on integrate_kernel<3> (unrolled
  default-link stencil), on mesh_small_kernel, and through the generic link loop with a
  permuted 13-link set."""
  opts, links = _VOL_PATHS[path]

  def expect(_, case, info):
    assert info.persist_tile == 0 and info.march_t == 0 and not info.tiled, case.name
    assert bool(info.small) == (path == 'small'), case.name

  for case in ref.step_cases_3d(shape, links):
    _check_vs_float64(_run(case, path, opts, expect), case, path)
