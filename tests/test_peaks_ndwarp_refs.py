"""CPU side of tests/test_gpu_peaks_ndwarp_edges.py: the references and the
cases, checked without a GPU over the SAME case builders (tests/refs64.py).

Peak search: `peaks64`, written from the definition (peak list, strike set,
clipped sharpness window), equals the vectorised oracle bit for bit wherever
the oracle is defined, and the cases reach the branches they name (candidate
counts around the list capacity, the widths and sizes around the kernels'
switches, NaN rows that couple into their neighbours).

ndimage_warp: what SciPy does with a NaN coordinate and with the zero-weight
tap beyond the last sample, stated as assertions on
scipy.ndimage.map_coordinates, and the non-vacuity of the cases built on it.
"""
import numpy as np
import pytest
from scipy import ndimage

from oracle import flow_oracle, warp_oracle
from tests import refs64
from tests.refs64 import NDWARP_CASE_GROUPS, PEAKS_CASE_GROUPS, peak_mask64, peaks64

f32 = np.float32


def assert_same_bits(got, want, name=''):
  """Equal shape and dtype, identical NaN pattern, every other element equal in
  its bits (so -0.0 is not 0.0)."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, name
  nan = np.isnan(want)
  np.testing.assert_array_equal(np.isnan(got), nan, err_msg=name)
  np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32), err_msg=name)


def _oracle(c):
  with np.errstate(invalid='ignore'):
    return flow_oracle.batched_peaks(c['img'], c['center'], c['min_distance'],
                                     c['threshold_rel'], c['radius'])


def _ref(c, **kw):
  return peaks64(c['img'], c['center'], c['min_distance'], c['threshold_rel'], c['radius'], **kw)


def _case(group, name):
  return next(c for c in PEAKS_CASE_GROUPS[group]() if c['name'] == name)


# ---------------------------------------------------------------------------
# peaks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('group', list(PEAKS_CASE_GROUPS))
def test_peaks64_equals_oracle(group):
  """All dim + 2 columns bit-equal, identical NaN patterns, on every case where
  the oracle is defined: every case but the surfaces smaller than the
  sharpness window, and exactly those."""
  cases = PEAKS_CASE_GROUPS[group]()
  assert len({c['name'] for c in cases}) == len(cases)
  for c in cases:
    sp = c['img'].shape[1:]
    rad = [c['radius']] * len(sp) if np.ndim(c['radius']) == 0 else c['radius']
    fits = all(2 * r + 1 <= a for r, a in zip(rad, sp))
    assert fits == c['oracle'], c['name']
    if c['oracle']:
      assert_same_bits(_ref(c), _oracle(c), c['name'])


def test_peaks64_group_is_a_batch_of_its_own():
  """`group`: the strike set is that of each run of `group` surfaces."""
  c = _case('coupling', 'couple_batch9')
  want = np.concatenate([
      flow_oracle.batched_peaks(c['img'][g:g + 4], c['center'], 2, 0.1, 5) for g in (0, 4, 8)])
  assert_same_bits(_ref(c, group=4), want)
  assert not np.array_equal(_ref(c, group=4), _ref(c), equal_nan=True)


def test_capacity_cases_count_exactly():
  """Surfaces 1 and 4 hold exactly 2047 / 2048 / 2049 peaks, the others fewer
  than the capacity: one list of the first four overflows at 2049, none below."""
  seen = set()
  for c in PEAKS_CASE_GROUPS['capacity']():
    n = int(c['name'][3:7])
    seen.add(n)
    assert c['img'].shape == (5, 64, 70) and c['min_distance'] == 0
    counts = peak_mask64(c['img'], 0, c['threshold_rel']).reshape(5, -1).sum(axis=1)
    assert list(counts) == [300, n, 700, 1500, n], c['name']
    vals = c['img'][1][c['img'][1] > 0]
    assert (len(np.unique(vals)) == n) == c['name'].endswith('distinct')
  assert seen == {2047, 2048, 2049}


def test_sweep_cases_cover_the_switches():
  shapes = {c['img'].shape[1:] for c in PEAKS_CASE_GROUPS['sweep']()}
  for w in (1, 63, 64, 65, 128, 129, 256, 257, 300):
    for h in (1, 3, 4, 5, 33):
      assert (h, w) in shapes
  sizes = {int(np.prod(s)) for s in shapes}
  assert {2**18 - 1, 2**18} <= sizes and (64, 64, 64) in shapes
  # peaks on the border: the first peak of every surface with more than one row
  # and column lies in a corner or on the first / last row or column
  for c in PEAKS_CASE_GROUPS['sweep']():
    h, w = c['img'].shape[-2:]
    out = _ref(c)
    y = out[:, 1] + c['center'][-2]
    x = out[:, 0] + c['center'][-1]
    assert (np.isin(y, (0, h - 1)) | np.isin(x, (0, w - 1))).all(), c['name']


def test_threshold_cases_straddle_the_product():
  """Of the five elements around threshold_rel x max, the product itself and
  the two below it are no peaks ('>' is strict), the two above are."""
  for t in (0.3, 0.5, 0.7):
    c = _case('threshold', f'thr_{t}')
    counts = peak_mask64(c['img'], 2, t).reshape(5, -1).sum(axis=1)
    assert list(counts) == [1, 1, 1, 2, 2]
    assert c['img'][2, 10, 11] == f32(t) * c['img'][2, 3, 4]
  c = _case('threshold', 'constant_50x50_t0.5')
  assert (peak_mask64(c['img'], 2, 0.5).reshape(5, -1).sum(axis=1) == 2500).all()   # > capacity
  for name in ('thr_rel_1.0', 'negative_8x9_t0.0', 'zero_50x50_t0.5'):
    assert np.isnan(_ref(_case('threshold', name))).all()


@pytest.mark.parametrize('tag', ['40x37', '512x512'])
def test_special_value_cases_say_what_they_claim(tag):
  out = _ref(_case('special', f'nan_couples_{tag}'))
  assert np.isnan(out[0]).all() and np.isfinite(out[1:]).all()
  # index 0, the NaN row's first-peak index, is struck: surface 1 has nothing
  # left and reads its un-struck element 0 (3.0), surface 2 falls to its third
  # peak (2.5) -- without the NaN row it would be 4 / 3 as well
  assert out[1, 3] == f32(4) / f32(3) and out[2, 3] == f32(4) / f32(2.5)
  c = _case('special', f'nan_couples_{tag}')
  assert peaks64(c['img'][1:], c['center'], 2, 0.5, 5)[1, 3] == f32(4) / f32(3)
  out = _ref(_case('special', f'nan_places_{tag}'))
  assert np.isnan(out[:3]).all() and np.isfinite(out[3]).all()
  for t in (0.5, 0.0):
    out = _ref(_case('special', f'posinf_{tag}_t{t}'))
    assert np.isfinite(out[0]).all() and np.isnan(out[1:]).all()
  out = _ref(_case('special', f'neginf_{tag}'))
  assert out[0, 2] == 32 and np.isnan(out[3]).all()
  assert (out[1:3, 2] == 0).all() and np.signbit(out[1:3, 2]).all()
  out = _ref(_case('special', f'window_min_{tag}'))
  assert out[0, 2] == np.inf and out[1, 2] == -np.inf and out[2, 2] == f32(4) / f32(-0.75)


def test_coupling_cases_say_what_they_claim():
  out = _ref(_case('coupling', 'couple_first_second'))
  assert out[1, 3] == 4.0      # 8 / 2: the 7 at A's first-peak index is struck
  assert out[0, 3] == 0.0 and out[2, 3] == 0.0
  out = _ref(_case('coupling', 'couple_index0'))
  assert out[1, 3] == 3.0 and out[2, 3] == 0.0
  assert {c['img'].shape[0] for c in PEAKS_CASE_GROUPS['coupling']()} >= {1, 4, 5, 9}


def test_negative_parameters_raise_before_any_device_work():
  """No GPU here: the ValueError comes before the device is touched."""
  from sofima_amd import flow_field
  img = np.zeros((1, 8, 8), f32)
  for kw in (dict(min_distance=-1), dict(peak_radius=-1), dict(peak_radius=(2, -3))):
    args = dict(min_distance=2, peak_radius=5)
    args.update(kw)
    with pytest.raises(ValueError):
      flow_field._batched_peaks(img, (4, 4), args['min_distance'], 0.5, args['peak_radius'])


def test_sfm_peaks_rejects_negative_parameters():
  """SFM_ERR_INVALID from the C entry, before the surface or the workspace is
  looked at (so no device is needed); the unused z radius of 2-D surfaces is
  not checked."""
  import ctypes as C
  from sofima_amd import _abi
  lib = _abi.load()
  out = (C.c_float * 8)()

  def call(min_distance, radius):
    d = _abi.SfmPeaksDesc()
    d.ndim, d.batch = 2, 2
    d.shape = (C.c_int32 * 3)(1, 8, 9)
    d.center_offset = (C.c_float * 3)(0, 4, 4)
    d.min_distance = min_distance
    d.threshold_rel = 0.5
    d.peak_radius = (C.c_int32 * 3)(*radius)
    d.surface = 0x1000      # never dereferenced: every call here fails before
    return lib.sfm_peaks(C.byref(d), C.cast(out, C.c_void_p)), lib.sfm_last_error()

  for m, r in ((-1, (0, 5, 5)), (2, (0, -1, 5)), (2, (0, 5, -2))):
    rc, msg = call(m, r)
    assert rc == -1 and b'must be >= 0' in msg        # SFM_ERR_INVALID
  rc, msg = call(2, (-1, 5, 5))
  assert rc == -3 and b'workspace' in msg             # valid: stops at the missing workspace


# ---------------------------------------------------------------------------
# ndimage_warp
# ---------------------------------------------------------------------------
def _warp_oracle(c, cmap=None):
  return warp_oracle.ndimage_warp(c['image'], c['cmap'] if cmap is None else cmap, c['stride'],
                                  **refs64.ndwarp_oracle_args(c))


def test_scipy_nan_coordinate_is_outside():
  img = np.arange(1, 26, dtype=f32).reshape(5, 5)
  for order in (0, 1):
    for coords in ([[np.nan], [1.0]], [[1.0], [np.nan]], [[np.nan], [np.nan]]):
      assert ndimage.map_coordinates(img, coords, order=order)[0] == 0.0
    for dtype in (np.uint8, np.uint16):
      assert ndimage.map_coordinates(img.astype(dtype), [[np.nan], [1.0]], order=order)[0] == 0


def test_scipy_reads_the_tap_beyond_the_end_mirrored():
  """Coordinate exactly on the last sample: the zero-weight tap is read from
  len - 2 (0 x inf = NaN), not from len - 1 (a clamp), not skipped; an axis of
  one sample reads itself."""
  base = np.arange(1, 26, dtype=f32).reshape(5, 5)
  for val in (np.inf, -np.inf, np.nan):
    img = base.copy()
    img[3, :] = val
    assert np.isnan(ndimage.map_coordinates(img, [[4.0], [1.0]], order=1)[0])
    img = base.copy()
    img[:, 3] = val
    assert np.isnan(ndimage.map_coordinates(img, [[1.0], [4.0]], order=1)[0])
    assert ndimage.map_coordinates(img, [[1.0], [4.0]], order=0)[0] == base[1, 4]
    img = base.copy()
    img[4, :] = val     # the last sample itself non-finite elsewhere on the row: untouched
    assert ndimage.map_coordinates(img, [[3.0], [1.0]], order=1)[0] != base[3, 1]   # tap 4, weight 0
  assert ndimage.map_coordinates(base[:1], [[0.0], [2.0]], order=1)[0] == base[0, 2]
  assert ndimage.map_coordinates(base[:1, :1], [[0.0], [0.0]], order=1)[0] == base[0, 0]


@pytest.mark.parametrize('dim', [2, 3])
@pytest.mark.parametrize('kind', refs64.NDWARP_NONFINITE_KINDS)
def test_nonfinite_map_cases_are_not_vacuous(dim, kind):
  """The oracle's float32 output holds no NaN (a non-finite dense coordinate
  gives 0), and at least 5 % of the voxels differ from the clean map's."""
  clean, bad, shape, stride = refs64.ndwarp_nonfinite_map(dim, kind)
  img = refs64._image(np.random.default_rng(0), shape, f32)
  for order in (0, 1):
    a = warp_oracle.ndimage_warp(img, bad, stride, order=order)
    b = warp_oracle.ndimage_warp(img, clean, stride, order=order)
    assert not np.isnan(a).any()
    hit = a != b
    assert hit.mean() >= 0.05, hit.mean()
    assert (a[hit] == 0).all() and hit.mean() < 0.9


def test_edge_tap_cases_reach_the_tap():
  for c in NDWARP_CASE_GROUPS['edge_tap']():
    name, out = c['name'], _warp_oracle(c)
    dim = c['image'].ndim
    if name.startswith('map_'):
      axis = int(name.split('_ax')[1][0])
      last = np.take(out, -1 if '_hi_' in name else 0, axis=axis)
      assert not last.any(), name            # the row exactly on the outermost node: all 0
      assert (c['image'] != 0).all() and out.any()
      # the far side of the map is untouched
      assert np.take(out, 0 if '_hi_' in name else -1, axis=axis).any(), name
    else:
      axis = int(name.split('_ax')[1][0])
      assert c['order'] == 1 and c['image'].dtype == f32
      last = np.take(out, -1 if '_hi_' in name else 0, axis=axis)
      assert np.isnan(last).all(), name      # 0 x inf from the tap beyond / at index 1
      keep = np.take(out, 0 if '_hi_' in name else -1, axis=axis)
      np.testing.assert_array_equal(keep, np.take(c['image'], 0 if '_hi_' in name else -1, axis=axis))
    assert dim in (2, 3)


def test_boundary_cases_sit_on_their_targets():
  targets = refs64.ndwarp_boundary_targets(6)
  assert targets[0] == 0 and np.signbit(targets[1]) and targets[2] < 0 and targets[5] == 5
  assert targets[6] > 5 > targets[7]
  for k in (0.5, 2.5, 4.5):
    assert {f32(k), np.nextafter(f32(k), f32(0)), np.nextafter(f32(k), f32(9))} <= set(targets)
  for c in NDWARP_CASE_GROUPS['boundary']():
    dim = c['image'].ndim
    axis = int(c['name'].split('_ax')[1][0])
    src = warp_oracle.ndimage_abs_map(c['cmap'], c['stride'], (1.0,) * 3)
    row0 = np.take(src[dim - 1 - axis], 0, axis=axis)
    other = (axis + 1) % dim
    line = np.moveaxis(row0, other - (other > axis), 0).reshape(len(targets), -1)[:, 0]
    np.testing.assert_array_equal(line, np.where(targets == 0, 0, targets).astype(np.float64))
    out = _warp_oracle(c)
    assert out.any() and not out.all()


def test_rounding_cases_round_as_claimed():
  for c in NDWARP_CASE_GROUPS['rounding']():
    if c['order'] != 1 or c['image'].dtype == f32:
      continue
    out = _warp_oracle(c)
    lo, hi = int(c['image'][..., 0].max()), int(c['image'][..., 1].max())
    # k + 0.5 goes up, the float32 below it stays
    assert (out[..., 0, 0] == hi).all() and (out[..., 1, 0] == lo).all(), c['name']
    assert (out[..., 1] == hi).all()


def test_shape_cases_produce_output():
  seen = set()
  for c in NDWARP_CASE_GROUPS['shapes']():
    out = _warp_oracle(c)
    seen.add(out.size)
    assert out.dtype == c['image'].dtype
    assert out.any(), c['name']
  assert {1, 255, 256, 257} <= seen and max(seen) > 1024
