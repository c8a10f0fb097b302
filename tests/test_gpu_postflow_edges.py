"""Edge tests of the small kernels between flow estimation and rendering (-m gpu):
map_utils.mask_irregular, map_utils.compose_maps_fast, flow_utils.clean_flow and
warp.warp_subvolume at the shapes, special values and thresholds where kernels
go wrong.

The case builders and the float64 references live at module level and need no
GPU: tests/test_postflow_refs.py runs the reference-side claims (the float32
oracle stays inside the derived compose bound, the threshold list is not
vacuous, the warp tie exclusion stays under its cap) on the CPU over the SAME
cases.
"""
import itertools
import types

import numpy as np
import pytest

from oracle import flow_utils_oracle, maps_oracle, warp_oracle
from tests.refs64 import around as _around, compose64, compose_atol, sample64 as _sample64, \
    smooth as _smooth

gpu_test = pytest.mark.gpu
f32 = np.float32


# ---------------------------------------------------------------------------
# mask_irregular
# ---------------------------------------------------------------------------
IRREG_STRIDES = ((25.0, 25.0), (31.5, 30.25), (20.0, 16.0), (10.0, 12.0), (40.0, 37.0))
IRREG_FRACS = (0.15, 0.25, 0.3, 0.45, 0.6, 0.8)


def irregular_params():
  """(stride xy, frac, max_frac): every stride with every frac, max_frac the
  default 2 - frac and, alternating, an explicit one above 1."""
  out = []
  for i, (stride, frac) in enumerate(itertools.product(IRREG_STRIDES, IRREG_FRACS)):
    out.append((stride, frac, None))
    out.append((stride, frac, (1.1, 1.35, 1.7)[i % 3]))
  return out


def threshold_differences(s, frac, max_frac):
  """float32 neighbour differences d for which d + s sits on frac * s or
  max_frac * s, or float32 ulps beside it: around the limit formed in double
  and around the one formed in float32 (they differ for some (s, frac))."""
  if max_frac is None:
    max_frac = 2 - frac
  ds = []
  for f in (frac, max_frac):
    for limit in (f * s, float(f32(f) * f32(s))):
      ds += _around(limit - s)
  return np.array(sorted(set(float(d) for d in ds)), f32)


def threshold_map(stride, frac, max_frac, axis, dtype, based=False):
  """[2, y, x] map: one row (axis 'x') or column (axis 'y') per difference of
  threshold_differences, holding (0, d, d), so that the difference d is exact
  in float32 and in float64.  `based`: rows (b, b (+) d, b (+) d) with float32
  sums instead -- float32 maps only, where the reference subtracts in float32
  like the kernel."""
  s = stride[0] if axis == 'x' else stride[1]
  d = threshold_differences(s, frac, max_frac)
  line = np.zeros((len(d), 3), f32)
  if based:
    b = f32(np.random.default_rng(len(d)).uniform(-40, 40, len(d)))
    line[:, 0] = b
    line[:, 1] = line[:, 2] = b + d
  else:
    line[:, 1] = line[:, 2] = d
  m = np.zeros((2,) + line.shape, f32)
  if axis == 'x':
    m[0] = line
  else:
    m = np.zeros((2,) + line.T.shape, f32)
    m[1] = line.T
  return m.astype(dtype)


def check_irregular(coord_map, stride, **kw):
  """Returned mask and in-place masked map == the reference's statements."""
  from sofima_amd import map_utils
  with np.errstate(all='ignore'):
    want_map, want_bad = maps_oracle.mask_irregular(coord_map, stride, **kw)
  got_map = coord_map.copy()
  got_bad = map_utils.mask_irregular(got_map, stride, **kw)
  msg = f'shape {coord_map.shape} {coord_map.dtype} stride {stride} {kw}'
  assert got_bad.dtype == bool and got_bad.shape == want_bad.shape, msg
  np.testing.assert_array_equal(got_bad, want_bad, err_msg=msg)
  np.testing.assert_array_equal(got_map, want_map, err_msg=msg)
  return want_bad


@gpu_test
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_mask_irregular_thresholds(gpu, dtype):
  """Neighbour differences exactly on a limit and float32 ulps beside it.  The
  reference adds the float64 stride scalar to the float32 differences and
  compares with frac * stride in double; a kernel that forms the limits or
  the sum in float32 masks a different set (it did, in every combination).
  float64 maps hold float32-representable values with exact differences, so
  narrowing them changes nothing."""
  masked = kept = 0
  for stride, frac, max_frac in irregular_params():
    for axis in 'xy':
      m = threshold_map(stride, frac, max_frac, axis, dtype)
      bad = check_irregular(m, stride, frac=frac, max_frac=max_frac, dilation_iters=0)
      masked += int(bad.sum())
      kept += int((~bad).sum())
      if dtype == np.float32:
        m = threshold_map(stride, frac, max_frac, axis, dtype, based=True)
        check_irregular(m, stride, frac=frac, max_frac=max_frac, dilation_iters=0)
  assert masked > 100 and kept > 100


def irregular_field(rng, shape, stride, rough=0.5):
  """Relative map whose neighbour distances straddle [0.3, 1.7] * stride."""
  m = rng.standard_normal((2,) + tuple(shape)) * rough * min(stride)
  return m.astype(f32)


@gpu_test
def test_mask_irregular_shapes_and_dilation(gpu):
  rng = np.random.default_rng(71)
  stride = (20.0, 16.0)
  for shape in ((1, 37), (41, 1), (1, 1), (2, 2), (4, 3), (19, 23)):
    for iters in (0, 1, 2, 5):
      m = irregular_field(rng, shape, stride)
      check_irregular(m, stride, frac=0.3, dilation_iters=iters)
      check_irregular(m, stride, frac=0.6, max_frac=1.2, dilation_iters=iters)
  # a single bad node in a small map: 5 dilations cover the whole map
  m = np.zeros((2, 4, 3), f32)
  m[0, 1, 1] = 30
  bad = check_irregular(m, stride, frac=0.25, dilation_iters=5)
  assert bad.all()


@gpu_test
def test_mask_irregular_nan_and_inf_nodes(gpu):
  """Comparisons with NaN are false: a NaN node is not bad by itself, an inf
  node is (inf > limit) unless its difference is inf - inf = NaN."""
  rng = np.random.default_rng(72)
  stride = (31.5, 30.25)
  m = irregular_field(rng, (33, 29), stride, rough=0.2)
  m[0, 3, 4] = np.nan
  m[1, 10, 10:13] = np.nan
  m[0, 20, 5] = np.inf
  m[1, 21, 7] = -np.inf
  m[0, 25, 8:10] = np.inf        # inf - inf between the two
  m[:, 32, 28] = np.nan
  m[:, 0, 0] = np.inf
  for iters in (0, 1, 2):
    bad = check_irregular(m, stride, frac=0.25, dilation_iters=iters)
    assert 0 < bad.sum() < bad.size


@gpu_test
def test_mask_irregular_large_map(gpu):
  """2^20 + nodes over many workgroups; bad nodes in the first and last rows
  and in both corners of each."""
  stride = (20.0, 16.0)
  rng = np.random.default_rng(73)
  m = (rng.standard_normal((2, 1031, 1021)) * 0.5).astype(f32)
  for y, x in ((0, 0), (0, 1020), (1030, 0), (1030, 1020), (0, 511), (1030, 700),
               (1, 3), (1029, 1019), (500, 500)):
    m[:, y, x] += 40
  assert m[0].size >= 2**20
  bad = check_irregular(m, stride, frac=0.25, dilation_iters=0)
  # a node is judged by the distance to its +x / +y neighbour: the very last
  # node has neither, its two neighbours are bad instead
  assert bad[0, 0] and bad[0, 1020] and bad[1030, 0] and bad[1030, 1019] and bad[1029, 1020]
  assert not bad[1030, 1020] and 9 <= bad.sum() < 40
  bad = check_irregular(m, stride, frac=0.25, dilation_iters=2)
  assert bad[0, 0] and bad[0, 1020] and bad[1030, 0] and bad[1030, 1020]
  assert 9 * 9 <= bad.sum() < 1000


@gpu_test
def test_mask_irregular_device_tensor_in_place(gpu):
  import torch
  from sofima_amd import map_utils
  rng = np.random.default_rng(74)
  stride = (25.0, 25.0)
  m = irregular_field(rng, (45, 52), stride)
  with np.errstate(all='ignore'):
    want_map, want_bad = maps_oracle.mask_irregular(m, stride, 0.3, dilation_iters=1)
  t = torch.from_numpy(m.copy()).to(gpu)
  ptr = t.data_ptr()
  bad = map_utils.mask_irregular(t, stride, 0.3, dilation_iters=1)
  assert t.data_ptr() == ptr
  np.testing.assert_array_equal(bad, want_bad)
  np.testing.assert_array_equal(t.cpu().numpy(), want_map)
  assert 0 < bad.sum() < bad.size


# ---------------------------------------------------------------------------
# compose_maps_fast
# ---------------------------------------------------------------------------
def _maps(rng, dim, shape1, shape2, amp1, amp2):
  m1 = np.stack([_smooth(rng, shape1, amp1) for _ in range(dim)]).astype(f32)
  m2 = np.stack([_smooth(rng, shape2, amp2) for _ in range(dim)]).astype(f32)
  return m1, m2


def compose_cases():
  """{name: dict(map1, start1, stride1, map2, start2, stride2)}.  Strides are
  dyadic and starts integral, so both lattices are exact in float32; map2
  stretches by far less than 2x per node."""
  cases = {}
  rng = np.random.default_rng(81)
  # more than 4096 x 256 nodes: the grid cap and the stride loop both run
  m1, m2 = _maps(rng, 2, (1, 1100, 1000), (1, 565, 515), 30.0, 6.0)
  cases['big'] = dict(map1=m1, start1=(0, 3, 5), stride1=10.5, map2=m2, start2=(0, 0, 0),
                      stride2=20.25)
  m1, m2 = _maps(rng, 2, (3, 37, 53), (5, 70, 90), 25.0, 8.0)
  cases['more_sections_in_map2'] = dict(map1=m1, start1=(0, 2, 1), stride1=31.5, map2=m2,
                                        start2=(0, 0, 0), stride2=20.25)
  m1, m2 = _maps(rng, 2, (2, 1, 17), (2, 6, 40), 10.0, 4.0)
  cases['map1_y1'] = dict(map1=m1, start1=(0, 2, 3), stride1=16.0, map2=m2, start2=(0, 0, 0),
                          stride2=8.0)
  m1, m2 = _maps(rng, 2, (1, 13, 1), (1, 30, 9), 10.0, 4.0)
  cases['map1_x1'] = dict(map1=m1, start1=(0, 1, 2), stride1=(16.0, 12.0), map2=m2,
                          start2=(0, 0, 0), stride2=(8.0, 12.0))
  m1, m2 = _maps(rng, 2, (1, 9, 11), (1, 1, 25), 3.0, 4.0)
  cases['map2_y1'] = dict(map1=m1, start1=(0, 0, 0), stride1=8.0, map2=m2, start2=(0, 0, 0),
                          stride2=8.0)
  m1, m2 = _maps(rng, 2, (1, 9, 11), (1, 21, 1), 3.0, 4.0)
  cases['map2_x1'] = dict(map1=m1, start1=(0, 0, 0), stride1=8.0, map2=m2, start2=(0, 0, 0),
                          stride2=8.0)
  m1, m2 = _maps(rng, 3, (1, 1, 7), (4, 5, 12), 6.0, 3.0)
  cases['vol_1_1_7'] = dict(map1=m1, start1=(1, 2, 1), stride1=(8.0, 10.5, 12.25), map2=m2,
                            start2=(0, 0, 0), stride2=(4.5, 20.25, 9.0))
  m1, m2 = _maps(rng, 3, (9, 1, 1), (12, 4, 5), 6.0, 3.0)
  cases['vol_9_1_1'] = dict(map1=m1, start1=(0, 1, 2), stride1=(8.0, 10.5, 12.25), map2=m2,
                            start2=(0, 0, 0), stride2=(7.5, 20.25, 9.0))
  m1, m2 = _maps(rng, 3, (1, 1, 7), (1, 1, 9), 6.0, 3.0)
  cases['vol_thin_both'] = dict(map1=m1, start1=(0, 0, 1), stride1=10.5, map2=m2,
                                start2=(0, 0, 0), stride2=10.5)
  # starts: negative, around 1e5 (equal on both sides), and map2 1e4 nodes later
  # (M = 2e5; the other way round the queries leave map2 by 1e4 cells and the
  # lattice of map1, not M, sets the scale of the rounding: outside the bound)
  m1, m2 = _maps(rng, 2, (2, 40, 44), (2, 70, 75), 25.0, 8.0)
  for name, a, b in (('starts_small', (0, 4, 6), (0, 1, 2)),
                     ('starts_negative', (0, -33, -41), (0, -36, -45)),
                     ('starts_1e5', (0, 100004, 100006), (0, 100001, 100002)),
                     ('starts_map2_1e4_later', (0, 3, 5), (0, 10003, 2))):
    cases[name] = dict(map1=m1, start1=a, stride1=31.5, map2=m2, start2=b, stride2=20.25)
  # NaN holes in map1 (queries stay inside map2)
  m1, m2 = _maps(rng, 2, (2, 30, 33), (2, 80, 80), 6.0, 5.0)
  m1[0, 0, 3, 4] = np.nan
  m1[1, 0, 10, 10:14] = np.nan
  m1[:, 1, 20:23, 5] = np.nan
  m1[:, 1, 0, 0] = np.nan
  m1[:, 0, 29, 32] = np.nan
  cases['nan_in_map1'] = dict(map1=m1, start1=(0, 12, 14), stride1=16.0, map2=m2,
                              start2=(0, 0, 0), stride2=16.0)
  # NaN holes in map2; map1 = 0 on equal lattices puts every query ON a node:
  # the upper corners carry weight 0 and still poison
  m1 = np.zeros((2, 1, 24, 24), f32)
  m1[:, 0, 12:] = _maps(rng, 2, (1, 12, 24), (1, 1, 1), 5.0, 1.0)[0][:, 0]
  m2 = _maps(rng, 2, (1, 1, 1), (1, 30, 30), 1.0, 5.0)[1]
  m2[0, 0, 5, 6] = np.nan
  m2[1, 0, 9, 9:12] = np.nan
  m2[:, 0, 20:22, 20:22] = np.nan
  cases['nan_in_map2'] = dict(map1=m1, start1=(0, 0, 0), stride1=16.0, map2=m2,
                              start2=(0, 0, 0), stride2=16.0)
  # queries up to 10 cells outside map2 on every side, and exactly on its last
  # node (m1 = dyadic shifts on equal lattices)
  m1 = np.zeros((2, 1, 30, 30), f32)
  m1[0, 0, :, :8] = -16 * 12.0
  m1[1, 0, :8, :] = -16 * 11.0
  m1[:, 0, 10:16, 10:16] += _maps(rng, 2, (1, 6, 6), (1, 1, 1), 7.0, 1.0)[0][:, 0]
  m2 = _maps(rng, 2, (1, 1, 1), (1, 20, 20), 1.0, 5.0)[1]
  cases['outside_and_last_node'] = dict(map1=m1, start1=(0, 0, 0), stride1=16.0, map2=m2,
                                        start2=(0, 0, 0), stride2=16.0)
  return cases


def compose_sweep_case(seed):
  """One of the 12 seeded geometries of the random sweep (2-D and 3-D)."""
  rng = np.random.default_rng(9000 + seed)
  dim = 2 + seed % 2
  strides = (4.5, 8.0, 10.5, 12.25, 16.0, 20.25, 31.5)
  pick = lambda: tuple(float(rng.choice(strides)) for _ in range(dim))
  if dim == 2:
    z = int(rng.integers(1, 4))
    shape1 = (z,) + tuple(int(v) for v in rng.integers(1, 41, 2))
    sections2 = (z + int(rng.integers(0, 3)),)       # map2 may have more sections
  else:
    shape1 = tuple(int(v) for v in rng.integers(1, 13, 3))
    sections2 = ()
  st1, st2 = pick(), pick()
  base = rng.integers(-50, 51, 3)
  start1 = tuple(int(v) for v in base + rng.integers(0, 4, 3))
  start2 = tuple(int(v) for v in base + rng.integers(0, 4, 3))
  # map2 covers 0.7 .. 1.3 of map1's extent per axis: queries leave it on some
  # sides, and M stays the scale of every coordinate involved
  shape2 = sections2 + tuple(max(1, int(np.ceil((n + 3) * a / b * rng.uniform(0.7, 1.3))))
                             for n, a, b in zip(shape1[-dim:], st1, st2))
  m1, m2 = _maps(rng, dim, shape1, shape2, float(rng.uniform(1, 40)),
                 0.3 * min(st2))
  for m in (m1, m2):
    if rng.random() < 0.6:
      hole = rng.random(m.shape[1:]) < 0.03
      m[:, hole] = np.nan
  return dict(map1=m1, start1=start1, stride1=st1, map2=m2, start2=start2, stride2=st2)


def describe_compose(case, mode):
  return (f"map1 {case['map1'].shape} start {case['start1']} stride {case['stride1']}, "
          f"map2 {case['map2'].shape} start {case['start2']} stride {case['stride2']}, {mode}")


def check_compose(got, case, mode, float32_reference=None):
  """`got` against (a) the float32 oracle and (b) the float64 reference."""
  msg = describe_compose(case, mode)
  got = np.asarray(got)
  dim = case['map1'].shape[0]
  want64, near, big = compose64(mode=mode, **case)
  atol = compose_atol(dim, big)
  assert got.shape == want64.shape and got.dtype == np.float32, msg
  if float32_reference is None:
    float32_reference = maps_oracle.compose_maps_fast(mode=mode, **case)
  # (a) float32, in JAX's operation order
  np.testing.assert_array_equal(np.isnan(got), np.isnan(float32_reference), err_msg=msg)
  np.testing.assert_allclose(got, float32_reference, rtol=1e-5, atol=atol, err_msg=msg)
  # (b) float64 from the definition; the NaN pattern is compared wherever the
  # choice of the cell does not hang on float32 rounding of the query
  assert near.sum() <= max(2, 1e-3 * near.size), f'{msg}: {int(near.sum())} queries next to a node'
  keep = np.broadcast_to(~near, got.shape)
  np.testing.assert_array_equal(np.isnan(got)[keep], np.isnan(want64)[keep], err_msg=msg)
  fin = np.isfinite(got) & np.isfinite(want64)
  err = float(np.abs(got[fin] - want64[fin]).max()) if fin.any() else 0.0
  assert err <= atol, f'{msg}: |got - float64| = {err:.4g} > {atol:.4g} (M = {big:.6g})'
  return err, atol, want64


def _run_compose(case, mode):
  from sofima_amd import map_utils
  return np.array(map_utils.compose_maps_fast(
      case['map1'], case['start1'], case['stride1'], case['map2'], case['start2'],
      case['stride2'], mode=mode))


@gpu_test
@pytest.mark.parametrize('mode', ['nearest', 'constant'])
def test_compose_grid_cap_and_stride_loop(gpu, mode):
  """1.1 M nodes: 4096 workgroups of 256 threads cover 4096 * 256 nodes per
  pass, the rest is reached by the stride loop."""
  case = compose_cases()['big']
  got = _run_compose(case, mode)
  err, atol, want64 = check_compose(got, case, mode)
  n = got[0].size
  assert n > 4096 * 256
  for c in range(2):
    for k in (0, 4096 * 256 - 1, 4096 * 256, n - 1):
      g, w = got[c].flat[k], want64[c].flat[k]
      assert np.isnan(g) == np.isnan(w), (c, k)
      if mode == 'nearest':
        assert np.isfinite(g) and abs(g - w) <= atol, (c, k, g, w)
  if mode == 'constant':   # some queries leave map2
    assert 0 < np.isnan(got).mean() < 0.5
  print(f'compose big {mode}: |got - f64| = {err:.3g}, allowed {atol:.3g}')


@gpu_test
@pytest.mark.parametrize('mode', ['nearest', 'constant'])
def test_compose_shapes_starts_and_holes(gpu, mode):
  cases = compose_cases()
  res = {}
  for name, case in cases.items():
    if name == 'big':
      continue
    res[name] = _run_compose(case, mode)
    check_compose(res[name], case, mode)
  # only start - min(start1, start2) enters: equal shifts of both starts, large
  # or negative, change nothing at all
  np.testing.assert_array_equal(res['starts_1e5'], res['starts_small'])
  np.testing.assert_array_equal(res['starts_negative'], res['starts_small'])
  # NaN holes in map1: NaN exactly there (all queries lie inside map2)
  m1 = cases['nan_in_map1']['map1']
  hole = np.isnan(m1).any(axis=0)
  assert hole.sum() > 5
  np.testing.assert_array_equal(np.isnan(res['nan_in_map1']),
                                np.broadcast_to(hole, m1.shape))
  # NaN nodes of map2: a query ON node (5, 5) has the NaN node (5, 6) as a
  # corner of weight 0 and is NaN in both modes; channel 1 is not
  got = res['nan_in_map2']
  assert np.isnan(got[0, 0, 5, 5]) and np.isnan(got[0, 0, 5, 6]) and np.isnan(got[0, 0, 4, 6])
  assert np.isfinite(got[1, 0, 5, 5]) and np.isfinite(got[0, 0, 5, 7])
  # outside map2 and on its last node
  got = res['outside_and_last_node']
  if mode == 'constant':
    assert np.isnan(got[:, 0, 19:, :]).all() and np.isnan(got[:, 0, :, 19:]).all()
    assert np.isnan(got[:, 0, :8, :]).all() and np.isnan(got[:, 0, :, :8]).all()
    assert np.isfinite(got[:, 0, 8:19, 8:19]).all()
  else:
    assert np.isfinite(got).all()
    m2 = cases['outside_and_last_node']['map2']
    # clamped: the last node's displacement carried outwards
    np.testing.assert_allclose(got[0, 0, 19, 25], m2[0, 0, 19, 19] - 6 * 16.0, rtol=0,
                               atol=1e-4)


@gpu_test
def test_compose_fewer_sections_in_map2_is_an_error(gpu):
  from sofima_amd import _abi, map_utils
  rng = np.random.default_rng(82)
  m1, m2 = _maps(rng, 2, (3, 8, 9), (2, 12, 12), 3.0, 3.0)
  with pytest.raises(_abi.SofimaAmdError, match='fewer sections'):
    map_utils.compose_maps_fast(m1, (0, 0, 0), 8.0, m2, (0, 0, 0), 8.0)


@gpu_test
@pytest.mark.parametrize('seed', range(12))
def test_compose_random_sweep(gpu, seed):
  case = compose_sweep_case(seed)
  for mode in ('nearest', 'constant'):
    check_compose(_run_compose(case, mode), case, mode)


# ---------------------------------------------------------------------------
# clean_flow
# ---------------------------------------------------------------------------
def flow_field_like(rng, shape, dim, spread=3.0):
  """[c, z, y, x] float32 flow: vectors, then (c = dim + 2) sharpness and ratio."""
  c = shape[0]
  f = (rng.standard_normal(shape) * spread).astype(f32)
  if c == dim + 2:
    f[dim] = rng.uniform(0.5, 4.0, shape[1:]).astype(f32)
    f[dim + 1] = rng.uniform(0.0, 3.0, shape[1:]).astype(f32)
    f[dim + 1][rng.random(shape[1:]) < 0.1] = 0.0      # ratio 0: exempt
  return f


def check_clean(flow, params, dim):
  from sofima_amd import flow_utils
  with np.errstate(all='ignore'):
    want = flow_utils_oracle.clean_flow(flow, *params, dim=dim)
  got = np.asarray(flow_utils.clean_flow(flow, *params, dim=dim))
  msg = f'flow {flow.shape} params {params!r} dim {dim}'
  assert got.dtype == np.float32 and got.shape == want.shape, msg
  np.testing.assert_array_equal(got, want, err_msg=msg)   # NaNs in the same places
  return want


@gpu_test
def test_clean_flow_degenerate_axes(gpu):
  """Length-1 and length-2 axes: the reflect boundary of the window folds onto
  the few samples there are."""
  rng = np.random.default_rng(91)
  shapes = (((4, 1, 1, 1), 2), ((4, 1, 1, 9), 2), ((4, 3, 2, 2), 2), ((4, 1, 2, 1), 2),
            ((5, 1, 1, 1), 3), ((5, 2, 1, 7), 3), ((5, 4, 5, 1), 3), ((5, 2, 2, 2), 3),
            ((5, 1, 6, 5), 3))
  nan_seen = kept = 0
  for shape, dim in shapes:
    for rep in range(6):
      flow = flow_field_like(rng, shape, dim)
      for params in ((1.4, 1.6, 4.0, 1.5), (0.0, 0.0, 0.0, 0.7), (1.0, 1.0, 2.5, 0.0)):
        for f in (flow, flow[:dim]):                     # channels dim + 2 and dim
          want = check_clean(f, params, dim)
          nan_seen += int(np.isnan(want).sum())
          kept += int(np.isfinite(want).sum())
  assert nan_seen > 50 and kept > 50


@gpu_test
def test_clean_flow_2d_window_stays_in_its_section(gpu):
  """dim = 2 over several z sections whose levels differ by far more than the
  deviation limit: a window reaching across z would see another median."""
  rng = np.random.default_rng(92)
  flow = flow_field_like(rng, (4, 5, 7, 9), 2, spread=0.5)
  flow[:2] += (np.arange(5, dtype=f32) * 100).reshape(1, 5, 1, 1)
  want = check_clean(flow, (0.0, 0.0, 0.0, 1.0), 2)
  assert 0 < np.isnan(want).mean() < 0.6
  check_clean(flow[:2], (0.0, 0.0, 0.0, 1.0), 2)
  # the same field as a volume: the 3 x 3 x 3 window does reach across z
  vol = np.concatenate([flow[:2], flow[:1], flow[2:]])
  check_clean(vol, (0.0, 0.0, 0.0, 1.0), 3)


@gpu_test
def test_clean_flow_thresholds_off(gpu):
  """Each threshold at 0 and negative, alone and combined (3^4 settings)."""
  rng = np.random.default_rng(93)
  flow = flow_field_like(rng, (4, 2, 11, 13), 2)
  on = (1.4, 1.6, 4.0, 1.5)
  counts = set()
  for setting in itertools.product(range(3), repeat=4):
    params = tuple((on[i], 0.0, -1.0 - i)[s] for i, s in enumerate(setting))
    want = check_clean(flow, params, 2)
    counts.add(int(np.isnan(want[0]).sum()))
  assert len(counts) > 8       # the settings do filter differently
  flow3 = flow_field_like(rng, (5, 3, 6, 7), 3)
  for params in ((1.4, 1.6, 4.0, 1.5), (0, 0, 0, 0), (-1, 1.6, -2, 1.5), (1.4, -1, 4.0, -3)):
    check_clean(flow3, params, 3)


@gpu_test
def test_clean_flow_inf_and_nan_in_every_channel(gpu):
  """np.nan_to_num turns +-inf into +-FLT_MAX and NaN into 0 inside the median;
  NaN compares false everywhere."""
  for dim, shape in ((2, (4, 2, 9, 10)), (3, (5, 4, 6, 7))):
    rng = np.random.default_rng(94 + dim)
    for ch in range(shape[0]):
      for value in (np.inf, -np.inf, np.nan):
        flow = flow_field_like(rng, shape, dim)
        pos = rng.random(shape[1:]) < 0.12
        flow[ch][pos] = value
        flow[ch, 0, 0, 0] = value
        flow[ch, -1, -1, -1] = value
        for params in ((1.4, 1.6, 4.0, 1.5), (0.0, 0.0, 0.0, 1.5), (0.0, 0.0, 1e38, 3e38)):
          check_clean(flow, params, dim)
          check_clean(flow[:dim], params, dim)
    # everything special at once
    flow = flow_field_like(rng, shape, dim)
    flow[rng.random(shape) < 0.1] = np.inf
    flow[rng.random(shape) < 0.1] = -np.inf
    flow[rng.random(shape) < 0.1] = np.nan
    check_clean(flow, (1.4, 1.6, 4.0, 1.5), dim)
    check_clean(flow, (0.0, 0.0, 0.0, 1.5), dim)


def _ulps(v):
  return [float(x) for x in _around(v)]


@gpu_test
def test_clean_flow_values_exactly_at_a_limit(gpu):
  """All four comparisons are strict and made in float32: a value equal to its
  limit passes, one ulp beyond fails."""
  ratio, sharp, mag, dev = 1.5, 1.25, 8.0, 2.0           # float32-representable
  flow = np.zeros((4, 1, 12, 15), f32)
  flow[2] = 3.0
  flow[3] = 2.0
  for i, v in enumerate(_ulps(ratio) + [0.0, -0.0]):
    flow[3, 0, 0, i] = v
    flow[3, 0, 1, i] = -v
  for i, v in enumerate(_ulps(sharp)):
    flow[2, 0, 2, i] = v
    flow[2, 0, 3, i] = -v
  for i, v in enumerate(_ulps(mag)):
    flow[0, 0, 5, 2 * i] = v               # isolated: also a deviation from median 0
    flow[1, 0, 7, 2 * i] = -v
  for i, v in enumerate(_ulps(dev)):
    flow[1, 0, 9, 2 * i] = v
    flow[0, 0, 11, 2 * i] = -v
  want = check_clean(flow, (ratio, sharp, mag, dev), 2)
  assert np.isnan(want[0, 0, 0, :2]).all() and not np.isnan(want[0, 0, 0, 2:7]).any()
  assert np.isnan(want[0, 0, 2, :2]).all() and not np.isnan(want[0, 0, 2, 2:5]).any()
  want = check_clean(flow, (ratio, sharp, mag, 0.0), 2)
  assert not np.isnan(want[0, 0, 5, 0:6:2]).any() and np.isnan(want[0, 0, 5, 6:10:2]).all()
  want = check_clean(flow, (ratio, sharp, 0.0, dev), 2)
  assert not np.isnan(want[0, 0, 9, 0:6:2]).any() and np.isnan(want[0, 0, 9, 6:10:2]).all()


@gpu_test
def test_clean_flow_median_ties(gpu):
  """Windows of few distinct values: the median is one of many equal samples."""
  rng = np.random.default_rng(96)
  for dim, shape in ((2, (4, 3, 17, 19)), (3, (5, 5, 9, 8))):
    for levels in (2, 3):
      flow = flow_field_like(rng, shape, dim)
      flow[:dim] = rng.integers(0, levels, (dim,) + shape[1:]).astype(f32)
      flow[:dim][:, rng.random(shape[1:]) < 0.05] = np.nan     # NaN -> 0 in the median
      for d in (0.5, 1.0, 1.5):
        want = check_clean(flow, (0.0, 0.0, 0.0, d), dim)
      check_clean(flow, (1.4, 1.6, 1.0, 1.0), dim)
  assert np.isnan(want).any()


@gpu_test
@pytest.mark.parametrize('form', [float, np.float64, np.float32])
def test_clean_flow_threshold_forms(gpu, form):
  """A Python number (or float32 scalar) is compared in float32, a float64
  scalar in float64 (NEP 50).  0.7 rounds DOWN to float32 and 0.1 rounds UP, so
  an entry equal to the float32 rounding is `< 0.7` and `> 0.1` in double
  only."""
  ratio, sharp, mag, dev = form(0.7), form(0.7), form(0.1), form(0.1)
  flow = np.zeros((4, 1, 12, 15), f32)
  flow[2] = 3.0
  flow[3] = 2.0
  for i, v in enumerate(_ulps(0.7)):
    flow[3, 0, 0, i] = v
    flow[2, 0, 2, i] = -v
  for i, v in enumerate(_ulps(0.1)):
    flow[0, 0, 5, 2 * i] = v
    flow[1, 0, 9, 2 * i] = -v
  assert float(f32(0.7)) < 0.7 and float(f32(0.1)) > 0.1
  w_all = check_clean(flow, (ratio, sharp, mag, dev), 2)
  w_mag = check_clean(flow, (0.0, 0.0, mag, 0.0), 2)
  w_dev = check_clean(flow[:2], (0.0, 0.0, 0.0, dev), 2)
  w_q = check_clean(flow, (ratio, sharp, 0.0, 0.0), 2)
  # the entry AT the float32 rounding (index 2 of _ulps) is where the forms part
  in_double = form is np.float64
  assert np.isnan(w_q[0, 0, 0, 2]) == in_double and np.isnan(w_q[0, 0, 2, 2]) == in_double
  assert np.isnan(w_mag[0, 0, 5, 4]) == in_double
  assert np.isnan(w_dev[1, 0, 9, 4]) == in_double
  assert np.isnan(w_all).any() and np.isfinite(w_all).any()
  # a positive limit that float32 rounds to 0 still switches its test on
  tiny = form(1e-60) if form is not np.float32 else np.float32(1e-45)
  check_clean(flow, (0.0, 0.0, tiny, 0.0), 2)
  check_clean(flow, (0.0, 0.0, 0.0, tiny), 2)


@gpu_test
def test_clean_flow_large_field(gpu):
  rng = np.random.default_rng(97)
  flow = flow_field_like(rng, (4, 1, 1024, 1031), 2)
  flow[:, 0, 0, 0] = (9.0, 0.0, 3.0, 2.0)
  flow[:, 0, -1, -1] = (0.0, -9.0, 3.0, 2.0)
  assert flow[0].size >= 2**20
  want = check_clean(flow, (1.4, 1.6, 8.0, 5.0), 2)
  assert np.isnan(want[0, 0, 0, 0]) and np.isnan(want[0, 0, -1, -1])
  assert 0.3 < np.isnan(want[0]).mean() < 0.9


# ---------------------------------------------------------------------------
# warp_subvolume
# ---------------------------------------------------------------------------
def _kernel_weights(kind, t, taps):
  """[len(taps), ...] weights of the samples at integer offsets `taps` from
  floor(q), t = q - floor(q), from the kernels' definitions, in double."""
  s = np.stack([np.abs(t - k) for k in taps])      # distance of the query to each sample
  if kind == 'linear':
    return np.clip(1.0 - s, 0.0, None)
  if kind == 'cubic':                             # cubic convolution, a = -0.75
    a = -0.75
    near = ((a + 2.0) * s - (a + 3.0)) * s * s + 1.0
    far = ((a * s - 5.0 * a) * s + 8.0 * a) * s - 4.0 * a
    return np.where(s <= 1.0, near, np.where(s < 2.0, far, 0.0))
  w = np.sinc(s) * np.sinc(s / 4.0)               # Lanczos, a = 4
  w = np.where(s < 4.0, w, 0.0)
  return w / w.sum(axis=0)


_TAPS = {'linear': (0, 1), 'cubic': (-1, 0, 1, 2), 'lanczos': (-3, -2, -1, 0, 1, 2, 3, 4)}


def resample64(img, qx, qy, kind):
  """img[y, x] resampled at (qx, qy) in double: 'nearest' (round half to even),
  'linear', 'cubic' (4 taps at -1 .. 2) or 'lanczos' (8 taps at -3 .. 4,
  sinc(t) sinc(t / 4), normalised per axis).  Samples outside the image count
  as 0; integer images are clipped to their range (and not rounded)."""
  img = np.asarray(img)
  h, w = img.shape
  src = img.astype(np.float64)

  def px(y, x):
    ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    return np.where(ok, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0.0)

  if kind == 'nearest':
    return px(np.rint(qy).astype(np.int64), np.rint(qx).astype(np.int64))
  x0, y0 = np.floor(qx), np.floor(qy)
  taps = _TAPS[kind]
  wx = _kernel_weights(kind, qx - x0, taps)
  wy = _kernel_weights(kind, qy - y0, taps)
  x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
  acc = np.zeros(qx.shape, np.float64)
  for j, ky in enumerate(taps):
    row = np.zeros(qx.shape, np.float64)
    for i, kx in enumerate(taps):
      row = row + wx[i] * px(y0 + ky, x0 + kx)
    acc = acc + wy[j] * row
  if img.dtype.kind in 'ui':
    info = np.iinfo(img.dtype)
    acc = np.clip(acc, info.min, info.max)
  return acc


def dense_coordinates(coord_map_z, map_start, img_start, out_start, out_size, stride, offset):
  """Source coordinates (x, y) in the image's frame for every output pixel of
  one section, as the kernel is documented to use them: the map's nodes made
  absolute in the MAP's dtype (node index * stride, then the box shift, each
  added in place), interpolated bilinearly -- extrapolating beyond the outer
  nodes -- in double at the pixel's position in node units, cast to float32."""
  nodes = np.array(coord_map_z, copy=True)             # [2, my, mx]
  if nodes.dtype != np.float64:
    nodes = nodes.astype(f32)
  my, mx = nodes.shape[1:]
  jy, jx = np.mgrid[:my, :mx]
  nodes[0] += jx * stride
  nodes[1] += jy * stride
  nodes += (np.asarray(map_start[:2], np.float64) * stride - np.asarray(img_start[:2]) +
            offset).reshape(2, 1, 1)
  nodes = nodes.astype(np.float64)
  py, px = np.mgrid[:out_size[1], :out_size[0]].astype(np.float64)
  gy = (py - (map_start[1] * stride - out_start[1] + offset)) / stride
  gx = (px - (map_start[0] * stride - out_start[0] + offset)) / stride
  i = np.clip(np.floor(gy), 0, my - 2).astype(np.int64)
  j = np.clip(np.floor(gx), 0, mx - 2).astype(np.int64)
  t, u = gy - i, gx - j
  dense = []
  for c in (0, 1):
    v = nodes[c]
    dense.append(((1.0 - t) * (1.0 - u) * v[i, j] + (1.0 - t) * u * v[i, j + 1] +
                  t * (1.0 - u) * v[i + 1, j] + t * u * v[i + 1, j + 1]).astype(f32))
  return dense[0].astype(np.float64), dense[1].astype(np.float64)


def quantise(q, kind):
  """(coordinates the resampling uses, ties): table kernels round half-to-even
  to 1 / 32 pixel, nearest neighbour to the pixel.  `ties`: within 2^-10 of a
  rounding tie, where another (equally valid) operation order of the dense-map
  interpolation may land on the other side.  An EXACT tie of the float32
  coordinate is not left out: half-to-even decides it, and above 1024 pixels,
  where float32 resolves 2^-8 of a 1 / 32 step, one pixel in 256 is one."""
  scale = 1.0 if kind == 'nearest' else 32.0
  frac = q * scale - np.floor(q * scale)
  ties = (np.abs(frac - 0.5) < 2.0**-10) & (frac != 0.5)
  return np.rint(q * scale) / scale, ties


WARP_MAX_TIES = 0.005     # share of a case's pixels that may be left out


def warp_reference(case, kind):
  """(want [c, z, y, x] float64, compared [z, y, x] bool) for a warp case."""
  img, cm = case['image'], case['coord_map']
  (img_start, _), (map_start, _) = case['image_box'], case['map_box']
  out_start, out_size = case['out_box']
  want = np.zeros((img.shape[0], out_size[2], out_size[1], out_size[0]), np.float64)
  compared = np.ones(want.shape[1:], bool)
  for z in range(img.shape[1]):
    if np.all(np.isnan(cm[:, z])):
      continue                                   # skipped section: stays 0
    qx, qy = dense_coordinates(cm[:, z], map_start, img_start, out_start, out_size,
                               case['stride'], case.get('offset', 0.0))
    qx, tx = quantise(qx, kind)
    qy, ty = quantise(qy, kind)
    compared[z] = ~(tx | ty)
    for c in range(img.shape[0]):
      want[c, z] = resample64(img[c, z], qx, qy, kind)
  return want, compared


def _texture(rng, shape, dtype):
  from tests.util import em_texture
  img = em_texture(rng, shape).astype(dtype)
  if dtype == np.uint16:
    img = img * np.uint16(211) + rng.integers(0, 211, shape).astype(np.uint16)
  elif dtype == np.float32:
    img = img * f32(0.37) - f32(20.0) + rng.random(shape, dtype=f32)
  return img


def _smooth_map(rng, z, my, mx, amp):
  """[2, z, my, mx] smooth sub-pixel displacements with irrational-looking
  offsets (no dyadic values, so rounding ties are as rare as chance)."""
  yy, xx = np.mgrid[:my, :mx]
  cm = np.zeros((2, z, my, mx))
  for k in range(z):
    cm[0, k] = amp * np.sin(yy / 2.7 + 0.31 * k) + 0.237 * xx + np.pi / 7 + \
        rng.standard_normal((my, mx)) * 0.4
    cm[1, k] = amp * 0.8 * np.cos(xx / 3.3 + 0.17 * k) - 0.173 * yy + np.e / 5 + \
        rng.standard_normal((my, mx)) * 0.4
  return cm


def warp_case(name, dtype=np.uint8, map_dtype=np.float32):
  """Named warp geometries.  Boxes are (start xyz, size xyz)."""
  rng = np.random.default_rng(sum(map(ord, name)))
  if name == 'overhang':
    # 2 channels x 3 sections (one skipped), non-integer stride, offset != 0; the
    # output box hangs over every image border by more than the Lanczos support
    # and the map (7 x 8 nodes) is smaller than the output: both extrapolation
    # sides are used
    img = _texture(rng, (2, 3, 120, 150), dtype)
    cm = _smooth_map(rng, 3, 7, 8, 3.0)
    cm[:, 1] = np.nan
    return dict(image=img, image_box=((5, 8, 0), (150, 120, 3)), coord_map=cm.astype(map_dtype),
                map_box=((1, 1, 0), (8, 7, 3)), stride=15.5,
                out_box=((-9, -6, 0), (182, 151, 3)), offset=2.25)
  if name == 'far_outside':
    img = _texture(rng, (1, 1, 90, 100), dtype)
    cm = _smooth_map(rng, 1, 6, 7, 2.0)
    # the right part and the top rows read hundreds of pixels outside: 0 (the
    # float32 coordinates there are still finer than 1 / 32 pixel by 2^-10)
    cm[0, 0, :, 4:] += 400.0 + 17.0 / 3
    cm[1, 0, :2, :] -= 700.0 + 1.0 / 7
    return dict(image=img, image_box=((0, 0, 0), (100, 90, 1)), coord_map=cm.astype(map_dtype),
                map_box=((0, 0, 0), (7, 6, 1)), stride=16.0, out_box=((0, 0, 0), (100, 90, 1)))
  if name == 'map_2x2':
    img = _texture(rng, (1, 2, 70, 80), dtype)
    cm = _smooth_map(rng, 2, 2, 2, 1.5)
    return dict(image=img, image_box=((0, 0, 0), (80, 70, 2)), coord_map=cm.astype(map_dtype),
                map_box=((1, 1, 0), (2, 2, 2)), stride=24.5, out_box=((-5, -4, 0), (92, 81, 2)),
                offset=-1.5)
  if name == 'one_pixel_wide':
    img = _texture(rng, (1, 1, 97, 5), dtype)[..., 2:3]
    cm = _smooth_map(rng, 1, 9, 4, 0.6)
    cm[0] = cm[0] * 0.05 + np.sqrt(3) / 7   # the 1-pixel column (x = 10) stays in the output
    cm[1] += 0.61 * np.arange(4)              # sheared: rows do not share one sub-pixel phase
    return dict(image=np.ascontiguousarray(img), image_box=((10, 0, 0), (1, 97, 1)),
                coord_map=cm.astype(map_dtype), map_box=((0, 0, 0), (4, 9, 1)), stride=12.0,
                out_box=((-10, -3, 0), (41, 103, 1)), offset=10.0)
  if name == 'large':
    img = _texture(rng, (1, 1, 2048, 2100), dtype)
    cm = _smooth_map(rng, 1, 34, 35, 4.0)
    return dict(image=img, image_box=((0, 0, 0), (2100, 2048, 1)),
                coord_map=cm.astype(map_dtype), map_box=((0, 0, 0), (35, 34, 1)), stride=63.5,
                out_box=((-4, -3, 0), (2110, 2056, 1)))
  raise KeyError(name)


def _ns(box):
  return types.SimpleNamespace(start=np.array(box[0]), size=np.array(box[1]))


def run_warp(case, interp):
  from sofima_amd import warp
  return warp.warp_subvolume(case['image'], _ns(case['image_box']), case['coord_map'],
                             _ns(case['map_box']), case['stride'], _ns(case['out_box']), interp,
                             offset=case.get('offset', 0.0))


# float32 images: largest |result - resample64| / max|image| of the OpenCV
# restatement (float32 weight tables, float32 accumulation) over all float32
# cases of this file, measured on the CPU (tests/test_postflow_refs.py asserts
# it): 4.06e-7, recorded as 4.1e-7.  The kernel may sum in another order:
# margin 4 x.
WARP_F32_MEASURED = 4.1e-7
WARP_F32_R = 4 * WARP_F32_MEASURED


def check_warp(got, case, interp, label='', r_limit=WARP_F32_R):
  """`got` ([c, z, y, x]) against the float64 resampling reference."""
  kind = 'lanczos' if interp is None else interp
  img = case['image']
  want, compared = warp_reference(case, kind)
  msg = f'{label} {img.dtype} {kind} map {case["coord_map"].dtype}'
  assert got.shape == want.shape and got.dtype == img.dtype, msg
  left_out = 1.0 - compared.mean()
  assert left_out <= WARP_MAX_TIES, f'{msg}: {left_out:.4%} of the pixels are rounding ties'
  keep = np.broadcast_to(compared, want.shape)
  diff = np.abs(got.astype(np.float64) - want)[keep]
  if kind == 'nearest':
    assert diff.max() == 0, f'{msg}: {int((diff > 0).sum())} pixels differ'
  elif img.dtype.kind in 'ui':
    # 15-bit weight tables: the ks^2 rounding errors add up to < 0.01 count
    assert diff.max() <= 1.0, f'{msg}: max |diff| {diff.max():.4f} counts'
    share = (diff <= 0.51).mean()
    assert share >= 0.999, f'{msg}: only {share:.5%} within 0.51 counts'
  else:
    r = diff.max() / np.abs(img).max()
    assert r <= r_limit, f'{msg}: |diff| / max|img| = {r:.3g} > {r_limit:.3g}'
    return float(r), left_out
  return float(diff.max()), left_out


@gpu_test
@pytest.mark.parametrize('map_dtype', [np.float32, np.float64])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize('interp', ['nearest', 'linear', 'cubic', None])
def test_warp_vs_float64_resampling(gpu, dtype, interp, map_dtype):
  """Tap geometry, kernels, zero border and the 1 / 32-pixel coordinate
  quantisation against the analytic reference: overhanging output box, map
  smaller than the output, skipped section, offset, fractional stride,
  channels and sections."""
  case = warp_case('overhang', dtype, map_dtype)
  got = run_warp(case, interp)
  check_warp(got, case, interp, 'overhang')
  assert not got[:, 1].any()                        # the NaN section is left zero
  assert got[:, 0].std() > 1 and got[:, 2].std() > 1
  assert not got[:, :, :, 0].any()                  # beyond the image and the kernel support


@gpu_test
@pytest.mark.parametrize('name', ['far_outside', 'map_2x2', 'one_pixel_wide'])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
def test_warp_geometries(gpu, name, dtype):
  for interp, map_dtype in (('linear', np.float32), ('cubic', np.float64), (None, np.float32),
                            ('nearest', np.float64)):
    case = warp_case(name, dtype, map_dtype)
    got = run_warp(case, interp)
    check_warp(got, case, interp, name)
    assert got.any()
    if name == 'far_outside':
      assert not got[0, 0, :, 70:].any() and not got[0, 0, :20, :].any()
      assert got[0, 0, 40:, :50].any()


@gpu_test
def test_warp_large_image(gpu):
  case = warp_case('large', np.uint8, np.float32)
  assert min(case['image'].shape[2:]) >= 2048
  got = run_warp(case, 'cubic')
  worst, left_out = check_warp(got, case, 'cubic', 'large')
  print(f'warp large: max |diff| {worst:.4f} counts, {left_out:.4%} ties left out')
  assert got.std() > 10


@gpu_test
def test_warp_uint64_labels(gpu):
  """Labels above 2^40: nearest neighbour on the ids, exactly the label at the
  rounded (half to even) coordinate."""
  case = warp_case('overhang', np.uint8, np.float64)
  ids = np.array([0, 3, 2**40 + 5, 2**41 + 1, 2**63 + 11, 77, 2**40 + 6, 12345678901234],
                 np.uint64)
  index = case['image'] // 32                      # 0 .. 7; outside the image: 0 -> label 0
  labels = dict(case, image=ids[index])
  got = run_warp(labels, None)
  assert got.dtype == np.uint64
  # the reference resamples in double: it picks the small index, not the label
  want, compared = warp_reference(dict(case, image=index), 'nearest')
  want = ids[want.astype(np.int64)]
  keep = np.broadcast_to(compared, want.shape)
  assert 1.0 - compared.mean() <= WARP_MAX_TIES
  np.testing.assert_array_equal(got[keep], want[keep])
  assert (got > 2**40).any() and (got == 0).any() and not got[:, 1].any()


@gpu_test
@pytest.mark.parametrize('interp', ['nearest', 'linear', None])
def test_warp_nan_nodes_inside_a_section(gpu, interp):
  """NaN nodes inside a used section have no analytic meaning: the contract is
  OpenCV's -- a NaN coordinate rounds to INT_MIN (cvRound), which reads outside
  the image -- so this case is compared with the oracle only."""
  for dtype in (np.uint8, np.float32):
    case = warp_case('overhang', dtype, np.float32)
    case['coord_map'] = case['coord_map'].copy()
    case['coord_map'][0, 0, 2:4, 3] = np.nan
    case['coord_map'][1, 2, 5, 5:7] = np.nan
    got = run_warp(case, interp)
    want = warp_oracle.warp_subvolume(case['image'], case['image_box'], case['coord_map'],
                                      case['map_box'], case['stride'], case['out_box'], interp,
                                      offset=case['offset'])
    if dtype == np.float32:
      np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-4)
    else:
      np.testing.assert_array_equal(got, want)
    assert got[:, 0].any()
