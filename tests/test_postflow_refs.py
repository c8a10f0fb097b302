"""CPU checks of the reference side of tests/test_gpu_postflow_edges.py: what the
GPU tests assume about their oracles, their float64 references and their
cases is itself asserted here, without a GPU, over the SAME cases."""
import numpy as np
import pytest

from oracle import flow_utils_oracle, maps_oracle, warp_oracle
from tests import test_gpu_postflow_edges as edges

f32 = np.float32


# ---------------------------------------------------------------------------
# mask_irregular
# ---------------------------------------------------------------------------
def test_irregular_threshold_list_is_not_vacuous():
  """For at least a quarter of the (stride, frac, max_frac) combinations a
  limit formed in float32 differs from the one formed in double."""
  params = edges.irregular_params()
  for need in ((25.0, 25.0), (31.5, 30.25), (20.0, 16.0), (10.0, 12.0)):
    for frac in (0.15, 0.25, 0.3, 0.45, 0.6, 0.8):
      assert (need, frac, None) in params
  differ = 0
  for stride, frac, max_frac in params:
    fr = (frac, 2 - frac if max_frac is None else max_frac)
    differ += any(f32(f * s) != f32(f) * f32(s) for f in fr for s in stride)
  assert differ >= len(params) / 4, (differ, len(params))


def _float32_arithmetic_mask(m, stride, frac, max_frac):
  """mask_irregular with the limits AND the sum formed in float32 (what NumPy
  1.x's value-based casting did; no dilation)."""
  m = np.asarray(m, f32)
  if max_frac is None:
    max_frac = 2 - frac
  sx, sy = f32(stride[0]), f32(stride[1])
  dx = np.pad(np.diff(m[0], axis=-1), [[0, 0], [0, 1]]) + sx
  dy = np.pad(np.diff(m[1], axis=-2), [[0, 1], [0, 0]]) + sy
  lo, hi = f32(frac), f32(max_frac)
  return (dx < lo * sx) | (dy < lo * sy) | (dx > hi * sx) | (dy > hi * sy)


def test_irregular_threshold_inputs_tell_the_arithmetics_apart():
  """The threshold maps separate float32 arithmetic from the reference's (sum
  and comparison in double) in every combination, so a kernel that rounds the
  limits or the sum cannot pass; float32 and float64 maps give one mask."""
  told = total = 0
  for stride, frac, max_frac in edges.irregular_params():
    hit = False
    for axis in 'xy':
      m = edges.threshold_map(stride, frac, max_frac, axis, np.float32)
      _, want = maps_oracle.mask_irregular(m, stride, frac, max_frac, dilation_iters=0)
      _, want64 = maps_oracle.mask_irregular(m.astype(np.float64), stride, frac, max_frac,
                                             dilation_iters=0)
      np.testing.assert_array_equal(want, want64)
      assert want.any() and not want.all()
      hit |= bool((_float32_arithmetic_mask(m, stride, frac, max_frac) != want).any())
    told += hit
    total += 1
  assert told == total, (told, total)


# ---------------------------------------------------------------------------
# compose_maps_fast
# ---------------------------------------------------------------------------
def _oracle_in_bound(case, mode):
  got = maps_oracle.compose_maps_fast(mode=mode, **case)
  err, atol, _ = edges.check_compose(got, case, mode, float32_reference=got)
  return err / atol * 7 if case['map1'].shape[0] == 2 else err / atol * 11


@pytest.mark.parametrize('mode', ['nearest', 'constant'])
def test_compose_oracle_stays_inside_the_derived_bound(mode):
  """The float32 oracle against the float64 reference under
  (T + 3) 2^-24 M on every case of the GPU tests."""
  worst = {}
  for name, case in edges.compose_cases().items():
    worst[name] = _oracle_in_bound(case, mode)
  for seed in range(12):
    worst[f'sweep{seed}'] = _oracle_in_bound(edges.compose_sweep_case(seed), mode)
  print({k: round(v, 2) for k, v in worst.items()})     # units of 2^-24 M
  assert max(worst.values()) > 0.5                       # the bound is not idle


def test_compose_cases_cover_what_they_claim():
  cases = edges.compose_cases()
  assert cases['big']['map1'][0].size > 4096 * 256
  assert cases['more_sections_in_map2']['map2'].shape[1] > \
      cases['more_sections_in_map2']['map1'].shape[1]
  dims = {edges.compose_sweep_case(s)['map1'].shape[0] for s in range(12)}
  assert dims == {2, 3}
  # map2 stretches by far less than 2x per node
  for name, case in cases.items():
    m2, st = case['map2'], np.broadcast_to(case['stride2'], (case['map2'].shape[0],))
    for c in range(m2.shape[0]):
      ax = m2.ndim - 1 - c
      if m2.shape[ax] > 1:
        with np.errstate(invalid='ignore'):
          g = np.abs(np.diff(m2[c], axis=ax - 1))
        assert np.nanmax(g) < st[::-1][c], name


def test_compose64_on_a_known_answer():
  """Translation by whole nodes: the composition of two constant shifts."""
  m1 = np.zeros((2, 1, 6, 7), f32)
  m1[0] = 16.0
  m2 = np.zeros((2, 1, 9, 10), f32)
  m2[1] = -3.0
  out, near, big = edges.compose64(m1, (0, 0, 0), 16.0, m2, (0, 0, 0), 16.0, 'nearest')
  assert not near.any() and big == 9 * 16.0
  np.testing.assert_array_equal(out[0], 16.0)
  np.testing.assert_array_equal(out[1], -3.0)
  out = edges.compose64(m1, (0, 0, 0), 16.0, m2[..., :7], (0, 0, 0), 16.0, 'constant')[0]
  assert np.isnan(out[:, 0, :, 5:]).all() and np.isfinite(out[:, 0, :, :5]).all()


# ---------------------------------------------------------------------------
# clean_flow
# ---------------------------------------------------------------------------
def test_clean_flow_threshold_forms_differ_in_the_reference():
  """0.7 rounds down and 0.1 rounds up to float32, so the reference itself
  answers differently for a Python number and a float64 scalar at an entry
  equal to the float32 rounding."""
  assert float(f32(0.7)) < 0.7 and float(f32(0.1)) > 0.1
  flow = np.zeros((4, 1, 3, 3), f32)
  flow[2] = 3.0
  flow[3, 0, 1, 1] = f32(0.7)
  flow[3, 0, 0, 0] = 2.0
  a = flow_utils_oracle.clean_flow(flow, 0.7, 0.0, 0.0, 0.0)
  b = flow_utils_oracle.clean_flow(flow, np.float64(0.7), 0.0, 0.0, 0.0)
  assert not np.isnan(a[0, 0, 1, 1]) and np.isnan(b[0, 0, 1, 1])
  flow[0, 0, 0, 2] = f32(0.1)
  a = flow_utils_oracle.clean_flow(flow, 0.0, 0.0, 0.1, 0.0)
  b = flow_utils_oracle.clean_flow(flow, 0.0, 0.0, np.float64(0.1), 0.0)
  assert not np.isnan(a[0, 0, 0, 2]) and np.isnan(b[0, 0, 0, 2])


def test_f32_threshold_reproduces_numpy_comparisons():
  from sofima_amd.flow_utils import _f32_threshold
  x = np.array(edges._around(0.7) + edges._around(0.1), f32)
  for t in (0.7, 0.1, np.float64(0.7), np.float64(0.1), f32(0.7), f32(0.1), 1, np.int64(1)):
    d = _f32_threshold(t)
    np.testing.assert_array_equal(x.astype(np.float64) > d, x > t)
    np.testing.assert_array_equal(x.astype(np.float64) < d, x < t)


# ---------------------------------------------------------------------------
# warp_subvolume
# ---------------------------------------------------------------------------
def test_resample64_kernels_from_their_definitions():
  t = np.linspace(0, 1, 33)[:-1]
  for kind, taps in edges._TAPS.items():
    w = edges._kernel_weights(kind, t, taps)
    np.testing.assert_allclose(w.sum(axis=0), 1.0, atol=1e-12 if kind != 'cubic' else 1e-12)
    assert w[taps.index(0), 0] == 1.0 and np.abs(w[:, 0]).sum() == 1.0   # interpolating
  # cubic convolution, a = -0.75, at t = 1 / 2: (-3, 19, 19, -3) / 32
  np.testing.assert_allclose(edges._kernel_weights('cubic', np.array([0.5]), (-1, 0, 1, 2))[:, 0],
                             np.array([-3, 19, 19, -3]) / 32.0, atol=1e-15)
  img = np.arange(30, dtype=np.float32).reshape(5, 6) ** 2
  qy, qx = np.mgrid[:5, :6].astype(np.float64)
  for kind in ('nearest', 'linear', 'cubic', 'lanczos'):
    np.testing.assert_allclose(edges.resample64(img, qx, qy, kind), img, atol=1e-9)
  # outside counts as 0; half-way between two pixels
  np.testing.assert_allclose(
      edges.resample64(img, np.array([5.5, 2.5]), np.array([0.0, 1.0]), 'linear'),
      [img[0, 5] / 2, (img[1, 2] + img[1, 3]) / 2])


_WARP_RUNS = [(n, d, k, m) for n in ('overhang', 'far_outside', 'map_2x2', 'one_pixel_wide')
              for d in (np.uint8, np.uint16, np.float32)
              for k, m in (('nearest', np.float64), ('linear', np.float32),
                           ('cubic', np.float64), (None, np.float32))]


def test_warp_oracle_meets_the_conditions_asked_of_the_kernel():
  """The OpenCV restatement against resample64 on the cases of the GPU tests:
  integer images within 1 count (0.51 at 99.9 %), float32 images within the
  measured r WITHOUT the margin, ties under the cap."""
  worst_r = 0.0
  for name, dtype, interp, map_dtype in _WARP_RUNS:
    case = edges.warp_case(name, dtype, map_dtype)
    got = warp_oracle.warp_subvolume(case['image'], case['image_box'], case['coord_map'],
                                     case['map_box'], case['stride'], case['out_box'], interp,
                                     offset=case.get('offset', 0.0))
    worst, _ = edges.check_warp(got, case, interp, name, r_limit=edges.WARP_F32_MEASURED)
    if dtype == np.float32 and interp != 'nearest':
      worst_r = max(worst_r, worst)
  print(f'float32 images: oracle within {worst_r:.3g} of max|img|')
  assert worst_r > edges.WARP_F32_MEASURED / 4          # the recorded figure is current


@pytest.mark.parametrize('map_dtype', [np.float32, np.float64])
def test_warp_tie_exclusion_share_is_below_its_cap(map_dtype):
  shares = {}
  for name in ('overhang', 'far_outside', 'map_2x2', 'one_pixel_wide', 'large'):
    case = edges.warp_case(name, np.uint8, map_dtype)
    for kind in ('nearest', 'linear'):
      for z in range(case['image'].shape[1]):
        if np.all(np.isnan(case['coord_map'][:, z])):
          continue
        qx, qy = edges.dense_coordinates(
            case['coord_map'][:, z], case['map_box'][0], case['image_box'][0],
            case['out_box'][0], case['out_box'][1], case['stride'], case.get('offset', 0.0))
        ties = edges.quantise(qx, kind)[1] | edges.quantise(qy, kind)[1]
        shares[name, kind, z] = float(ties.mean())
  print({k: round(v, 5) for k, v in shares.items()})
  assert max(shares.values()) <= edges.WARP_MAX_TIES, shares


def test_dense_coordinates_match_the_oracles_interpolator():
  """The test's own bilinear (extrapolating) interpolation == SciPy's
  RegularGridInterpolator, the reference's call, to double rounding."""
  from scipy import interpolate
  case = edges.warp_case('overhang', np.uint8, np.float64)
  qx, qy = edges.dense_coordinates(case['coord_map'][:, 0], case['map_box'][0],
                                   case['image_box'][0], case['out_box'][0],
                                   case['out_box'][1], case['stride'], case['offset'])
  cm, stride, off = case['coord_map'], case['stride'], case['offset']
  my, mx = cm.shape[2:]
  jy, jx = np.mgrid[:my, :mx]
  nodes = cm[:, 0].copy()
  nodes[0] += jx * stride + (case['map_box'][0][0] * stride - case['image_box'][0][0] + off)
  nodes[1] += jy * stride + (case['map_box'][0][1] * stride - case['image_box'][0][1] + off)
  gy = (np.arange(my) + case['map_box'][0][1]) * stride - case['out_box'][0][1] + off
  gx = (np.arange(mx) + case['map_box'][0][0]) * stride - case['out_box'][0][0] + off
  oy, ox = np.mgrid[:case['out_box'][1][1], :case['out_box'][1][0]]
  for c, q in ((0, qx), (1, qy)):
    want = interpolate.RegularGridInterpolator((gy, gx), nodes[c], bounds_error=False,
                                               fill_value=None)((oy, ox))
    np.testing.assert_allclose(q, want, rtol=0, atol=2e-5)   # q went through float32
