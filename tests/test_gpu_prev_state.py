"""processor_mesh.prev_state / relax_sections on the device: the fused compose
and average kernel bit for bit against the separately pinned compose_maps_fast,
mask_irregular on float64 against NumPy, and both against what the reference's
RelaxMesh.get_prev_state / run_relaxation produced (tests/golden/prev_state.npz)."""
import numpy as np
import pytest
from scipy import ndimage

from tests import prev_state_ref as ref

CASES = ('fwd', 'bwd')
SHAPES = [(19, 70), (1, 1), (1, 65), (130, 3)]


@pytest.fixture(scope='module')
def fixture(golden):
  return golden('prev_state')


# ---------------------------------------------------------------------------
# sfm_prev_state
# ---------------------------------------------------------------------------
def _smooth(rng, shape, amp):
  sig = [0] + [min(2.0, s / 4) for s in shape[1:]]
  return (ndimage.gaussian_filter(rng.standard_normal(shape), sig) * amp +
          rng.standard_normal(shape) * 0.5).astype(np.float32)


def _compose_inputs(shape, k, seed):
  """k flows ([c, y, x], every third one with 3 channels) and their tables of
  (look-back, reference mesh [2, y, x])."""
  rng = np.random.default_rng(seed)
  n = shape[0] * shape[1]

  def sprinkle(a, frac, value):
    a.reshape(a.shape[0], -1)[:, rng.random(n) < frac] = value

  def mesh():
    m = _smooth(rng, (2,) + shape, 30.0)
    sprinkle(m[:1], 0.05, np.nan)                # a NaN component / node
    sprinkle(m, 0.05, np.nan)
    sprinkle(m, 0.03, np.inf)
    sprinkle(m[1:], 0.03, -np.inf)
    return m

  flows, tables = [], []
  for j in range(k):
    c = 3 if j % 3 == 0 else 2
    f = _smooth(rng, (c,) + shape, 45.0)         # about a node spacing: taps move
    sprinkle(f[:2], 0.1, np.nan)
    sprinkle(f[:1], 0.03, np.inf)
    sprinkle(f[1:2], 0.03, -np.inf)
    sprinkle(f[:2], 0.03, 1e6)                   # far outside: mode nearest clamps
    f[:2].reshape(2, -1)[:, rng.random(n) < 0.05] = 0.0   # on a node: weight 0 meets inf
    if c == 2:
      tables.append([(j + 1, mesh())])
    else:
      offsets = [1, 2, 3] if j == 0 else list(range(-8, 0)) + list(range(1, 9))
      # look-backs in the table, and what names no section: 0, NaN, a fraction, inf,
      # an offset that is not in the table
      pool = np.array(offsets + [0, np.nan, 1.5, np.inf, 20], np.float32)
      f[2] = rng.choice(pool, size=shape)
      tables.append([(dz, mesh()) for dz in offsets])
    flows.append(f)
  return flows, tables


def _compose_average_numpy(flows, tables, stride):
  """processor/mesh.py:170-236, 248-277, 331-371 with map_utils.compose_maps_fast
  of this package, one call per (flow, offset)."""
  from sofima_amd import map_utils
  shape = flows[0].shape[1:]

  def compose(flow2, mesh):
    return np.array(map_utils.compose_maps_fast(flow2[:, None], (0, 0), stride, mesh[:, None],
                                                (0, 0), stride))[:, 0]

  prev = np.zeros((2,) + shape)
  count = np.zeros(shape, np.int32)
  for flow, table in zip(flows, tables):
    if flow.shape[0] == 2:
      ref_mesh = compose(flow, table[0][1])
      assert ref_mesh.dtype == np.float32
    else:
      ref_mesh = np.full((2,) + shape, np.nan)
      for dz, mesh in table:
        m = flow[2] == dz
        curr = flow[:2].copy()
        curr[0][~m] = np.nan
        curr[1][~m] = np.nan
        curr = compose(curr, mesh)
        ref_mesh[0][m] = curr[0][m]
        ref_mesh[1][m] = curr[1][m]
    count += np.isfinite(ref_mesh[0]).astype(np.int32)
    np.nan_to_num(ref_mesh, copy=False)
    prev += ref_mesh
  count = count.astype(np.float32)
  count[count == 0] = np.nan
  with np.errstate(over='ignore', invalid='ignore'):
    return prev / count[np.newaxis], count


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1, 3, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_compose_average_bit_for_bit(gpu, shape, k):
  from sofima_amd import processor_mesh
  stride = (40.0, 32.0)                          # y, x as compose_maps_fast reads them
  flows, tables = _compose_inputs(shape, k, seed=100 * k + shape[0])
  with np.errstate(all='ignore'):
    want, count = _compose_average_numpy(flows, tables, stride)
  got = processor_mesh.compose_average(flows, tables, stride).cpu().numpy()
  assert got.dtype == np.float64 and got.shape == want.shape
  if shape[0] * shape[1] > 100:                  # the inputs reach every branch
    assert np.isnan(count).any() and (k == 1 or np.nanmax(count) >= 2)
    assert np.isfinite(want).any() and (np.abs(want[np.isfinite(want)]) > 1e30).any()
  np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.gpu
def test_compose_average_reads_strided_planes(gpu):
  """Section planes of [c, nz, y, x] volumes are read where they lie: the
  descriptor points into the volumes with their channel stride, nothing is
  copied, and the result is that of the same planes handed over on their own."""
  import torch
  from sofima_amd import processor_mesh
  shape = (19, 70)
  n, nz = shape[0] * shape[1], 3
  flows, tables = _compose_inputs(shape, 3, seed=7)
  want = processor_mesh.compose_average(flows, tables, 40.0).cpu().numpy()
  vols = [torch.from_numpy(np.stack([np.zeros_like(f), f, np.ones_like(f)], 1)).to(gpu)
          for f in flows]
  hist = [[(dz, torch.from_numpy(np.stack([m, m + 1, m + 2], 1)).to(gpu)[:, 0]) for dz, m in t]
          for t in tables]
  views = [v[:, 1] for v in vols]
  assert not any(v.is_contiguous() for v in views)
  d, keep, _ = processor_mesh._prev_state_desc(views, hist, 40.0, gpu)
  for f, (view, table) in enumerate(zip(views, hist)):
    assert d.flows[f].flow == view.data_ptr()
    assert d.flows[f].flow_channel_stride == nz * n
    assert d.flows[f].mesh_channel_stride == nz * n
    for k, (_, m) in enumerate(table):
      assert d.flows[f].mesh[k] == m.data_ptr()
  assert {t.data_ptr() for t in keep} == (
      {v.data_ptr() for v in views} | {m.data_ptr() for t in hist for _, m in t})
  got = processor_mesh.compose_average(views, hist, 40.0).cpu().numpy()
  np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
  # planes that are not dense are copied, once
  sparse = [v[:, :, :, ::2] for v in (torch.zeros((2, 1, 19, 140), device=gpu),)]
  d, keep, _ = processor_mesh._prev_state_desc(
      [sparse[0][:, 0]], [[(1, torch.zeros((2,) + shape, device=gpu))]], 40.0, gpu)
  assert d.flows[0].flow == keep[0].data_ptr() != sparse[0].data_ptr()
  assert d.flows[0].flow_channel_stride == n


# ---------------------------------------------------------------------------
# sfm_mask_irregular_f64
# ---------------------------------------------------------------------------
def _check_irregular_f64(gpu, m, stride, **kw):
  import torch
  from sofima_amd import map_utils
  want = m.copy()
  want_bad = ref.mask_irregular_np(want, stride, **kw)
  t = torch.from_numpy(m.copy()).to(gpu)
  bad, n_valid = map_utils.mask_irregular_f64(t, stride, **kw)
  np.testing.assert_array_equal(bad.cpu().numpy().astype(bool), want_bad)
  np.testing.assert_array_equal(t.cpu().numpy().view(np.uint64)[~np.isnan(want)],
                                want.view(np.uint64)[~np.isnan(want)])
  np.testing.assert_array_equal(np.isnan(t.cpu().numpy()), np.isnan(want))
  assert int(n_valid.item()) == int((~np.isnan(want)).any(axis=0).sum())
  return want_bad


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_mask_irregular_f64_equals_numpy(gpu, shape):
  rng = np.random.default_rng(shape[1])
  stride = (40.0, 32.0)
  n = shape[0] * shape[1]
  for iters in (0, 1, 2):
    m = ndimage.gaussian_filter(rng.standard_normal((2,) + shape), (0, 1, 1)) * 60
    m += rng.standard_normal(m.shape) * 3
    m.reshape(2, -1)[:, rng.random(n) < 0.05] = np.nan
    m[:1].reshape(1, -1)[:, rng.random(n) < 0.03] = np.nan       # one component only
    m.reshape(2, -1)[:, rng.random(n) < 0.02] = np.inf
    bad = _check_irregular_f64(gpu, m, stride, frac=0.5, max_frac=1.4, dilation_iters=iters)
    _check_irregular_f64(gpu, m, stride, frac=0.7, dilation_iters=iters)
    if n > 100 and iters == 0:                   # both outcomes occur before dilation
      assert bad.any() and not bad.all()
  _check_irregular_f64(gpu, np.full((2,) + shape, np.nan), stride, frac=0.5)   # n_valid 0


@pytest.mark.gpu
def test_mask_irregular_f64_does_not_narrow(gpu):
  """A difference whose sum with the stride sits 1e-9 below frac * stride is a
  fold in float64 and none once the map is narrowed to float32."""
  stride, frac = (40.0, 40.0), 0.5
  m = np.zeros((2, 5, 67))
  m[0, 2, 65] = -(20.0 + 1e-9)                    # x: 40 + diff = 20 - 1e-9 < 20
  m[0, 2, 66] = m[0, 2, 65]
  m[1, 3, 10] = -(20.0 + 1e-9)                    # y, one row up
  m[1, 4, 10] = m[1, 3, 10]
  narrowed = m.astype(np.float32).astype(np.float64)
  assert not ref.mask_irregular_np(narrowed.copy(), stride, frac, dilation_iters=0).any()
  bad = _check_irregular_f64(gpu, m, stride, frac=frac, dilation_iters=0)
  assert bad[2, 64] and bad[2, 10] and bad.sum() == 2


# ---------------------------------------------------------------------------
# prev_state and relax_sections against the reference's records
# ---------------------------------------------------------------------------
def _masked(history, mask):
  if mask is None:
    return None
  h = history.copy()
  h[:, mask] = np.nan
  return h


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_prev_state_vs_reference(gpu, fixture, name):
  """prev_state against the reference's get_prev_state: NaN pattern equal, values
  within the composition tolerance of test_compose_maps_fast_golden (rtol 1e-5,
  atol 2e-5).  The composition interpolates absolute coordinates of up to
  69 * 40 = 2760, where a float32 ulp (2.4e-4) is beyond that bound: it holds
  because the fixture was generated with the stand-in's lattice in float32,
  as JAX's is, so both sides round alike.  The figures are printed per
  section before the assertions.
  """
  from sofima_amd import processor_mesh
  case = ref.Case(fixture, name)
  flows = case.flow_volumes()
  history = case.history()
  results = []
  for z in case.sections:
    got = processor_mesh.prev_state(
        z, flows, history, case.cfg['stride'], block_starts=case.block_starts,
        backward=case.backward, sections_to_skip=case.skip,
        masked_history=_masked(history, case.mask), mesh_min_frac=case.min_frac,
        mesh_max_frac=case.max_frac)
    if not case.has_prev(z):
      assert got is None
      continue
    want = case.rec(z, 'prev')
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape
    both = ~np.isnan(got) & ~np.isnan(want)
    err = np.abs(got[both] - want[both])
    print(f'prev_state {name} z={z}: NaN pattern equal {np.array_equal(np.isnan(got), np.isnan(want))}, '
          f'max |got - want| {err.max():.3e}, beyond rtol 1e-5 / atol 2e-5: '
          f'{int((err > 2e-5 + 1e-5 * np.abs(want[both])).sum())} of {err.size}')
    results.append((got, want))
  assert len(results) >= 3
  for got, want in results:
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
  for got, want in results:
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=1e-5, atol=2e-5)


def _block_start(case, z):
  starts = case.block_starts
  return min(s for s in starts if s >= z) if case.backward else max(s for s in starts if s <= z)


def _driver_kwargs(case):
  return dict(block_starts=case.block_starts, backward=case.backward,
              sections_to_skip=case.skip, mask=case.mask, mesh_min_frac=case.min_frac,
              mesh_max_frac=case.max_frac)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_relax_sections_one_at_a_time_vs_reference(gpu, fixture, name):
  """Every section solved on its own against the reference's own history."""
  from sofima_amd import processor_mesh
  case = ref.Case(fixture, name)
  flows, cfg, history = case.flow_volumes(), case.integration_config(), case.history()
  for z in case.sections:
    first = _block_start(case, z)
    meshes, statuses, steps, energies = processor_mesh.relax_sections(
        flows, cfg, solved=history, sections=[first] if first == z else [first, z],
        **_driver_kwargs(case))
    assert int(statuses[z]) == int(case.rec(z, 'status')), z
    assert steps[z] == int(case.rec(z, 'steps')), z
    want = case.rec(z, 'x')[:, 0]
    got = meshes[:, z]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    scale = np.nanmax(np.abs(want))
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), atol=2e-3 * scale)
    np.testing.assert_allclose(energies[z], case.rec(z, 'ekin'), rtol=1e-3, atol=1e-6)
    others = [s for s in range(history.shape[1]) if s not in (z, first)]
    np.testing.assert_array_equal(meshes[:, others].view(np.uint32),
                                  history[:, others].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_relax_sections_chained_equals_section_by_section(gpu, fixture, name):
  """The device hand-off: one call over all sections == the driver called per
  section and fed its own outputs through `solved`, bit for bit."""
  from sofima_amd import processor_mesh
  case = ref.Case(fixture, name)
  flows, cfg = case.flow_volumes(), case.integration_config()
  kw = _driver_kwargs(case)
  meshes, statuses, steps, energies = processor_mesh.relax_sections(
      flows, cfg, sections=case.sections, **kw)
  assert meshes.dtype == np.float32 and meshes.shape == case.history().shape
  assert [int(statuses[z]) for z in case.sections] == [int(case.rec(z, 'status'))
                                                      for z in case.sections]
  assert [steps[z] for z in case.sections] == [int(case.rec(z, 'steps')) for z in case.sections]
  solved = np.zeros_like(meshes)
  for z in case.sections:
    first = _block_start(case, z)
    m, st, sp, en = processor_mesh.relax_sections(
        flows, cfg, solved=solved, sections=[first] if first == z else [first, z], **kw)
    assert (int(st[z]), sp[z], en[z]) == (int(statuses[z]), steps[z], energies[z])
    solved[:, z] = m[:, z]
  np.testing.assert_array_equal(solved.view(np.uint32), meshes.view(np.uint32))
  if not case.backward:                          # all sections, in the default order
    again, _, _, _ = processor_mesh.relax_sections(flows, cfg, **kw)
    np.testing.assert_array_equal(again.view(np.uint32), meshes.view(np.uint32))
