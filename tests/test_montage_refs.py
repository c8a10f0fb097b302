"""CPU checks of the reference side of tests/test_gpu_montage_edges.py: what the
GPU tests assume about their oracles, their float64 references and their
cases is itself asserted here, without a GPU, over the SAME cases."""
import numpy as np
import pytest

from oracle import stitch_oracle
from tests import test_gpu_montage_edges as edges

f32 = np.float32


# ---------------------------------------------------------------------------
# target mesh
# ---------------------------------------------------------------------------
def test_target_oracle_stays_inside_the_derived_bound():
  """The float32 oracle against target64 under (T + 4) 2^-24 M on every case,
  NaN / inf patterns equal outside `near`, `near` under its cap."""
  worst = {}
  for name in edges.target_cases():
    want32 = edges.target_refs(name)[0]
    nd = want32.shape[0]
    _, d64, atol = edges.check_target(want32, name)
    worst[name] = d64 / atol * ((4 if nd == 2 else 8) + 4)
  print({k: round(v, 2) for k, v in worst.items()})       # units of 2^-24 M
  assert max(worst.values()) > 0.5                         # the bound is not idle


def test_target64_reproduces_the_goldens(golden):
  g = golden('montage')
  stride = tuple(float(v) for v in g['stride'])
  for xin, want in ((g['x'], g['tg0']), (g['xs'], g['tg1'])):
    got, near, big = edges.target64(g['nbors'], xin, g['fx'], g['fy'], stride)
    assert near.sum() <= max(2, 1e-3 * near.size)
    keep = np.broadcast_to(~near, got.shape)
    np.testing.assert_array_equal(np.isnan(got)[keep], np.isnan(want)[keep])
    fin = np.isfinite(got) & np.isfinite(want)
    assert fin.sum() > 100
    assert np.abs(got[fin] - want[fin]).max() <= edges.target_atol(2, big)
  g = golden('montage3d')
  stride = tuple(float(v) for v in g['stride'])
  got, near, big = edges.target64(g['nbors'], g['x'], g['fx'], g['fy'], stride)
  assert near.sum() <= max(2, 1e-3 * near.size)
  keep = np.broadcast_to(~near, got.shape)
  np.testing.assert_array_equal(np.isnan(got)[keep], np.isnan(g['tg'])[keep])
  fin = np.isfinite(got) & np.isfinite(g['tg'])
  assert fin.sum() > 100
  assert np.abs(got[fin] - g['tg'][fin]).max() <= edges.target_atol(3, big)


def _stats(name):
  c = edges.target_cases()[name]
  s = {}
  with np.errstate(all='ignore'):
    edges.target64(c['nbors'], c['x'], c['fx'], c['fy'], c['stride'], stats=s)
  return s


def test_target_cases_cover_what_they_claim():
  cases = edges.target_cases()
  assert tuple(sorted(cases)) == edges.TARGET_CASE_NAMES
  stats = {name: _stats(name) for name in cases}
  # padded flows: fx and fy differ in shape and count and reach beyond every
  # recorded size by 1 .. 4 nodes; some pastes run past the mesh and are cropped
  for name, c in cases.items():
    assert c['fx'].shape[2:] != c['fy'].shape[2:] and c['fx'].shape[1] != c['fy'].shape[1], name
    nd = c['x'].shape[0]
    for rows in c['nbors']:
      for nb in rows:
        if nb[0] == -1:
          continue
        flow = c['fx'] if nb[7] == 0 else c['fy']
        rec = (nb[3], nb[4]) if nb[7] == 0 else (nb[4], nb[3])
        assert all(1 <= s - r for s, r in zip(flow.shape[-2:], rec)), name
        assert min(rec) >= 1 and all(r <= m for r, m in zip(rec, c['x'].shape[-2:])), name
        pad = flow[(slice(None), nb[1]) + (slice(None),) * (nd - 2) + (slice(rec[0], None),)]
        assert np.isnan(pad).all(), name
        if nd == 3:
          assert nb[9] <= c['x'].shape[2] and flow.shape[2] > nb[9], name
  assert sum(s['cropped'] for s in stats.values()) > 20
  assert all(stats[n]['cropped'] > 0 for n in ('g22_15x31', 'g22_16x16', 'g22_17x33',
                                               'vol21_z0', 'vol12_zpos'))
  # an earlier update survives in one component only
  assert stats['nonfinite_x']['survive_one'] > 0
  # a NaN in one flow component makes the whole update NaN (the query is NaN)
  assert stats['g22_17x33_nan']['survive_one'] == 0
  # queries out of range on both sides of both axes, and exactly on the last node
  assert stats['large_amp']['out'] == {(0, 'lo'), (0, 'hi'), (1, 'lo'), (1, 'hi')}
  assert stats['zero_flow']['last'] > 10 and not stats['zero_flow']['out']
  want32 = edges.target_refs('zero_flow')[0]
  assert np.isnan(want32[:, 1, :10, 4]).all() and np.isfinite(want32[:, 1, :10, :4]).all()
  # every sign combination
  signs = set().union(*(s['signs'] for s in stats.values() if len(s['signs_z']) == 0))
  assert signs == {(o, m, d) for o in (-1, 0, 1) for m in (-1, 1) for d in (0, 1)}
  signs3 = set().union(*(s['signs'] for s in stats.values() if s['signs_z']))
  assert signs3 >= {(o, m, 0) for o in (-1, 0, 1) for m in (-1, 1)} and \
      {d for _, _, d in signs3} == {0, 1}
  signs_z = set().union(*(s['signs_z'] for s in stats.values()))
  assert signs_z == {(o, m) for o in (-1, 0, 1) for m in (-1, 1)}
  # four -1 rows; -1 rows before valid ones
  assert stats['isolated_tile']['all_nan_tiles'] == 1
  assert (cases['isolated_tile']['nbors'][2, :, 0] == -1).all()
  assert all(s['minus_before_valid'] > 0 for s in stats.values())
  # mesh sizes, strides, volumetric shapes
  shapes = {c['x'].shape[2:] for c in cases.values()}
  assert shapes >= {(15, 31), (16, 16), (17, 33), (5, 40), (40, 5), (4, 9, 18), (1, 6, 17)}
  assert {c['stride'] for c in cases.values()} == {(20., 20.), (16., 10.5), (8., 16., 20.)}
  for name in edges.PREV_FN_CASES:      # wide enough for the tiled integrator
    assert cases[name]['x'].shape[-1] >= 40 and cases[name]['x'].shape[-2] >= 4
    assert np.isfinite(cases[name]['x']).all()
  # a volumetric mesh of one section gets no finite target at all
  assert np.isnan(edges.target_refs('vol21_thin')[0]).all()
  assert np.isfinite(edges.target_refs('vol21_z0')[0]).any()
  # NaN and both infinities among the nodes of x, in single components
  x = cases['nonfinite_x']['x']
  assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
  assert (np.isnan(x[0]) != np.isnan(x[1])).any()


# ---------------------------------------------------------------------------
# tile mesh force
# ---------------------------------------------------------------------------
def test_tile_force_oracle_stays_inside_the_derived_bound():
  worst = 0.0
  for ncomp, nz, ny, nx in edges.tile_force_params():
    oracle = stitch_oracle.elastic_tile_mesh if ncomp == 2 else stitch_oracle.elastic_tile_mesh_3d
    for variant in edges.TILE_VARIANTS:
      x, cx, cy = edges.tile_force_case(ncomp, nz, ny, nx, variant)
      with np.errstate(all='ignore'):
        got = oracle(x, cx, cy)
      worst = max(worst, edges.check_tile_force(got, x, cx, cy, f'{(ncomp, nz, ny, nx)} {variant}'))
  print(f'float32 oracle uses {worst:.3f} of the bound')
  assert 0.05 < worst <= 1.0


def test_tile_force_cases_cover_what_they_claim():
  x, cx, cy = edges.tile_force_case(2, 3, 17, 19, 'missing')
  assert np.isnan(cx).all(axis=0).any() and np.isnan(cy).all(axis=0).any()
  x, cx, cy = edges.tile_force_case(3, 1, 17, 19, 'inf')
  assert (cx == np.inf).any() and (cx == -np.inf).any() and (cy == -np.inf).any()
  x, cx, cy = edges.tile_force_case(3, 3, 17, 19, 'x_nonfinite')
  assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any()
  # terms at +-FLT_MAX that cancel exactly, and that add up to +-inf
  x, cx, cy = edges.tile_force_case(2, 1, 17, 19, 'saturated')
  with np.errstate(all='ignore'):
    f = stitch_oracle.elastic_tile_mesh(x, cx, cy)
  _, _, sat = edges.tile_force64(x, cx, cy)
  assert (sat & (f == 0)).any() and (sat & np.isinf(f)).any() and not np.isnan(f).any()
  # the two accumulation orders differ in the last bit on plain data
  x, cx, cy = edges.tile_force_case(2, 1, 17, 19, 'plain')
  a = stitch_oracle._tile_force(x, cx, cy, ((0, 'x'), (1, 'y'), (0, 'y'), (1, 'x')))
  b = stitch_oracle._tile_force(x, cx, cy, ((0, 'x'), (1, 'x'), (0, 'y'), (1, 'y')))
  assert (a[1] != b[1]).any() and (a[0] == b[0]).all()


# ---------------------------------------------------------------------------
# range mask
# ---------------------------------------------------------------------------
def test_range_limit_forms_are_not_vacuous():
  """For each limit form the fix is about, the reference's mask differs from
  the mask computed with the limit rounded to float32 first."""
  assert float(f32(0.7)) < 0.7
  hit = {}
  for img, limit in edges.f32_limit_cases():
    if isinstance(limit, np.float64) and float(f32(limit)) < float(limit):
      want = stitch_oracle.range_mask(img, limit, 3)
      hit[float(limit)] = bool((want != stitch_oracle.range_mask(img, f32(limit), 3)).any())
      # a Python float of the same value compares in float32
      np.testing.assert_array_equal(stitch_oracle.range_mask(img, float(limit), 3),
                                    stitch_oracle.range_mask(img, f32(limit), 3))
  assert hit and all(hit.values()), hit
  img, limit = edges.u16_limit_case()
  assert isinstance(limit, float) and float(f32(limit)) == 3.0
  want = stitch_oracle.range_mask(img, limit, 3)
  assert (want != stitch_oracle.range_mask(img, f32(limit), 3)).any()


def test_range_limit_reproduces_numpy_comparisons():
  import torch
  from sofima_amd.stitch_rigid import _given_dtype, _range_limit
  assert _given_dtype(torch.zeros(2, dtype=torch.bfloat16)) == np.float32   # no NumPy name
  assert _given_dtype(torch.zeros(2, dtype=torch.uint8)) == np.uint8
  assert _given_dtype(np.zeros(2, np.uint16)) == np.uint16
  vals = {np.dtype(np.float32): np.array(edges._around_all((0.7, 0.1, 3.0, 40.3)), f32),
          np.dtype(np.uint8): np.arange(256, dtype=np.uint8),
          np.dtype(np.uint16): np.array([0, 2, 3, 4, 255, 256, 65534, 65535], np.uint16)}
  limits = [0.7, 0.1, 3.0000001, 40.3, -1, 0, 3, 255, 256, 65535, 65536, 1000, 25.5]
  for dtype, v in vals.items():
    for value in limits:
      for form, cast in edges.LIMIT_FORMS.items():
        if form in ('int', 'int64') and value != int(value):
          continue
        t = cast(value)
        d = _range_limit(dtype, t)
        assert isinstance(d, float)
        np.testing.assert_array_equal(v.astype(np.float64) < d, v < t,
                                      err_msg=f'{dtype} {t!r} {form}')


def test_scipy_rank_filters_with_nan_depend_on_the_scan_order():
  """Why NaN pixels are left out: the filters of an image and of its mirror
  image disagree where a window holds a NaN."""
  from scipy import ndimage
  rng = np.random.default_rng(0)
  img = rng.random((9, 11)).astype(f32)
  img[4, 5] = np.nan
  a = ndimage.maximum_filter(img, 3)
  b = ndimage.maximum_filter(img[::-1, ::-1], 3)[::-1, ::-1]
  same = (a == b) | (np.isnan(a) & np.isnan(b))
  clean = ndimage.maximum_filter(np.nan_to_num(img), 3)
  clean_b = ndimage.maximum_filter(np.nan_to_num(img)[::-1, ::-1], 3)[::-1, ::-1]
  np.testing.assert_array_equal(clean, clean_b)     # without NaN it is symmetric
  assert not same.all()
