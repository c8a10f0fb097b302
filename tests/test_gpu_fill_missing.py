"""map_utils.fill_missing on the device (-m gpu): sfm_fill_missing_nearest.

Everything is bits: the kernels move channel values, they compute none.  The
expectation is tests/fill_missing_ref.py, the brute-force statement that
tests/test_fill_missing_ref.py pins to the reference's results wherever the
nearest valid node is unique; the device must equal it everywhere, ties included.
"""
import numpy as np
import pytest
import torch

from sofima_amd import map_utils
from sofima_amd import processor_warp
from sofima_amd._dev import DeviceArray
from tests import render3d_ref
from tests.fill_missing_ref import bits, cases, fill_missing_ref

pytestmark = pytest.mark.gpu

NEAREST = dict(extrapolate=True, interpolate_first=False)


def check(m, **kw):
  """Device == statement, bit for bit; the input is not written."""
  before = m.copy()
  got = map_utils.fill_missing(m, **kw)
  assert isinstance(got, DeviceArray)
  got = np.asarray(got)
  np.testing.assert_array_equal(bits(m), bits(before))
  want = fill_missing_ref(m, **kw)
  assert got.dtype == m.dtype and got.shape == m.shape
  np.testing.assert_array_equal(bits(got), bits(want))
  return got


def field(rng, shape, dtype=np.float32):
  return rng.uniform(-30.0, 30.0, shape).astype(dtype)


def test_fixture_cases(gpu, golden):
  for c in cases(golden('fill_missing')):
    got = check(c['map'], **c['kw'])
    # ... so the reference's result on every node it settles
    settled = np.broadcast_to(~(c['filled'] & ~c['unique']), got.shape)
    np.testing.assert_array_equal(bits(got)[settled], bits(c['out'])[settled], err_msg=c['name'])


@pytest.mark.parametrize('nx', [70, 130])
def test_lines_across_waves_one_far_node(gpu, nx):
  """The largest distances: one valid node in the far corner of a row that spans two
  and three 64-lane chunks."""
  rng = np.random.default_rng(nx)
  for corner in ((4, nx - 1), (0, 0), (4, 0), (2, 64)):
    m = np.full((2, 1, 5, nx), np.nan, np.float32)
    m[(slice(None), 0) + corner] = field(rng, 2)
    got = check(m, **NEAREST)
    assert (got == got[(slice(None), 0) + corner].reshape(2, 1, 1, 1)).all()
  # valid nodes on both sides of the chunk borders, gaps across them
  m = field(rng, (2, 1, 5, nx))
  m[:, 0, :, 3:nx - 2] = np.nan
  m[:, 0, 1, 63] = 1.0
  m[:, 0, 3, 64] = 2.0
  check(m, **NEAREST)


def test_long_z(gpu):
  rng = np.random.default_rng(1)
  m = np.full((3, 33, 5, 4), np.nan, np.float64)
  m[:, 32, 4, 3] = field(rng, 3)
  got = check(m, **NEAREST)
  assert (got == m[:, 32, 4, 3].reshape(3, 1, 1, 1)).all()
  m[:, 0, 0, 0] = field(rng, 3)
  m[:, 16, 2, 1] = field(rng, 3)
  check(m, **NEAREST)
  m = field(rng, (3, 33, 5, 4), np.float32)
  m[:, rng.uniform(size=(33, 5, 4)) < 0.9] = np.nan
  check(m, **NEAREST)


def test_axes_of_length_one(gpu):
  rng = np.random.default_rng(2)
  m = np.full((3, 1, 1, 1), np.nan, np.float32)
  assert np.isnan(check(m, **NEAREST)).all()
  assert not check(m, invalid_to_zero=True, **NEAREST).any()
  m[1:] = 4.0                                 # still invalid: channel 0 is NaN
  assert np.isnan(check(m, **NEAREST)).all()
  for shape in ((3, 2, 3, 70), (2, 4, 1, 9), (3, 1, 7, 1), (2, 1, 1, 66)):
    m = field(rng, shape)
    m[:, rng.uniform(size=shape[1:]) < 0.8] = np.nan
    m[:, 0, 0, 0] = 1.0
    check(m, **NEAREST)


@pytest.mark.parametrize('axis', [1, 2, 3])
def test_axis_at_its_limit(gpu, axis):
  """16384 nodes on one axis, the valid nodes at its ends: the largest squared
  distance the 32-bit keys must hold next to the "no source" mark."""
  shape = [3, 1, 1, 1]
  shape[axis] = 16384
  m = np.full(shape, np.nan, np.float32)
  far = [slice(None), 0, 0, 0]
  far[axis] = 16383
  m[tuple(far)] = (1.0, 2.0, 3.0)
  got = check(m, **NEAREST)
  assert (got == np.array([1.0, 2.0, 3.0], np.float32).reshape(3, 1, 1, 1)).all()
  near = list(far)
  near[axis] = 0
  m[tuple(near)] = (4.0, 5.0, 6.0)
  got = np.moveaxis(check(m, **NEAREST), axis, 1).reshape(3, -1)
  # 8191 is as far from node 0 as 8192 is from node 16383; 8191.5 is no node: no tie
  assert (got[0, :8192] == 4.0).all() and (got[0, 8192:] == 1.0).all()


def test_tie_rule_on_a_checkerboard(gpu):
  """Every filled node has 2 to 4 equidistant valid neighbours: the lowest C-order
  index wins -- the node above if there is one, else the node to the left, ..."""
  rng = np.random.default_rng(3)
  y, x = np.mgrid[:8, :9]
  m = field(rng, (2, 1, 8, 9))
  m[:, 0, (y + x) % 2 == 1] = np.nan
  got = check(m, **NEAREST)
  np.testing.assert_array_equal(got[:, 0, 3, 4], m[:, 0, 2, 4])    # inside: the node above
  np.testing.assert_array_equal(got[:, 0, 0, 3], m[:, 0, 0, 2])    # top row: the node to the left
  np.testing.assert_array_equal(got[:, 0, 5, 0], m[:, 0, 4, 0])
  # 3-D: z before y before x
  z, y, x = np.mgrid[:4, :5, :6]
  m = field(rng, (3, 4, 5, 6), np.float64)
  m[:, (z + y + x) % 2 == 1] = np.nan
  got = check(m, **NEAREST)
  np.testing.assert_array_equal(got[:, 2, 2, 3], m[:, 1, 2, 3])
  np.testing.assert_array_equal(got[:, 0, 2, 3], m[:, 0, 1, 3])
  np.testing.assert_array_equal(got[:, 0, 0, 3], m[:, 0, 0, 2])


def test_slices_are_independent(gpu):
  rng = np.random.default_rng(4)
  m = field(rng, (2, 5, 9, 11))
  m[:, rng.uniform(size=(5, 9, 11)) < 0.85] = np.nan
  m[:, 3] = np.nan
  got = check(m, **NEAREST)
  perm = np.array([3, 0, 4, 2, 1])
  np.testing.assert_array_equal(bits(check(np.ascontiguousarray(m[:, perm]), **NEAREST)),
                                bits(got[:, perm]))
  # a 3-channel map is one volume: the empty slice 3 is filled from its neighbours
  m3 = np.concatenate([m, m[:1]])
  assert np.isfinite(check(m3, **NEAREST)).all()


def test_inf_and_all_invalid_semantics(gpu):
  rng = np.random.default_rng(5)
  # inf makes a node invalid; slice 1 holds inf but no NaN and is filled all the same
  m = field(rng, (2, 3, 6, 7))
  m[:, 0, 1:5, 2:6] = np.nan
  m[0, 0, 0, 0] = np.inf
  m[1, 1, 2, 3] = -np.inf
  m[:, 2] = np.inf                              # no valid node, no NaN
  got = check(m, **NEAREST)
  assert np.isfinite(got[:, :2]).all() and np.isnan(got[:, 2]).all()
  np.testing.assert_array_equal(got[:, 1, 2, 3], m[:, 1, 1, 3])
  got = check(m, invalid_to_zero=True, **NEAREST)
  assert np.isfinite(got[:, :2]).all() and not got[:, 2].any()
  # without extrapolate only the invalid_to_zero rule applies
  got = check(m, invalid_to_zero=True, interpolate_first=False)
  np.testing.assert_array_equal(bits(got[:, :2]), bits(m[:, :2]))
  assert not got[:, 2].any()
  np.testing.assert_array_equal(bits(check(m, interpolate_first=False)), bits(m))
  # the NaN-free map comes back unchanged, inf and all, whatever the keywords
  whole = field(rng, (3, 2, 3, 4), np.float64)
  whole[1, 0, 1, 1] = np.inf
  whole[:, 1] = -np.inf
  for kw in (NEAREST, dict(invalid_to_zero=True, **NEAREST), {}, dict(extrapolate=True)):
    np.testing.assert_array_equal(bits(check(whole, **kw)), bits(whole))


def test_interpolate_first_raises_on_nan(gpu):
  rng = np.random.default_rng(6)
  m = field(rng, (2, 1, 4, 5))
  np.testing.assert_array_equal(bits(np.asarray(map_utils.fill_missing(m))), bits(m))
  m[0, 0, 1, 1] = np.nan
  with pytest.raises(NotImplementedError, match='interpolate_first=False'):
    map_utils.fill_missing(m)                   # the default arguments
  with pytest.raises(NotImplementedError, match='Qhull'):
    map_utils.fill_missing(m, extrapolate=True, invalid_to_zero=True, interpolate_first=True)


def test_argument_checks(gpu):
  with pytest.raises(ValueError):
    map_utils.fill_missing(np.zeros((4, 1, 2, 2), np.float32))
  with pytest.raises(ValueError):
    map_utils.fill_missing(np.zeros((2, 2, 2), np.float32))
  with pytest.raises(TypeError):
    map_utils.fill_missing(np.zeros((2, 1, 2, 2), np.int32))
  with pytest.raises(TypeError):
    map_utils.fill_missing(torch.zeros((2, 1, 2, 2), dtype=torch.float16, device=gpu))
  with pytest.raises(ValueError, match='16384'):
    map_utils.fill_missing(torch.zeros((2, 1, 1, 16385), dtype=torch.float32, device=gpu),
                           **NEAREST)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_dtypes_and_residency(gpu, dtype):
  rng = np.random.default_rng(7)
  m = field(rng, (2, 2, 13, 67), dtype)
  m[:, rng.uniform(size=(2, 13, 67)) < 0.9] = np.nan
  m[1, 0, 0, 0] = np.nan                        # one channel only, payload kept apart
  want = check(m, **NEAREST)
  t = torch.from_numpy(m).to(gpu)
  kept = t.clone()
  for arg in (t, DeviceArray(t)):
    a = map_utils.fill_missing(arg, **NEAREST)
    b = map_utils.fill_missing(arg, **NEAREST)
    assert a.tensor.is_cuda and a.tensor.dtype == t.dtype
    assert a.tensor.data_ptr() != t.data_ptr()
    np.testing.assert_array_equal(bits(np.asarray(a)), bits(want))
    np.testing.assert_array_equal(bits(np.asarray(b)), bits(want))
  int_t = torch.int32 if dtype == np.float32 else torch.int64
  assert torch.equal(t.view(int_t), kept.view(int_t))


def test_fill_inverted_renders_like_maps_filled_one_by_one(gpu, golden):
  sc = render3d_ref.scenes(golden('render3d'))[0]
  holed = {}
  for i, (tg_box, inv) in sc['inverted'].items():
    inv = inv.copy()
    assert inv.shape[0] == 3 and min(inv.shape[1:]) >= 3
    inv[:, :, 0] = np.nan                       # part of the shell that invert_map leaves
    inv[:, :, :, -1] = np.nan
    inv[1, inv.shape[1] // 2, 1, 1] = np.nan
    holed[i] = (tg_box, inv)
  filled = processor_warp.fill_inverted(holed)
  one_by_one = {}
  for i, (tg_box, inv) in holed.items():
    assert isinstance(filled[i][1], DeviceArray) and filled[i][1].dtype == np.float64
    np.testing.assert_array_equal(filled[i][0].start, tg_box.start)
    np.testing.assert_array_equal(filled[i][0].size, tg_box.size)
    m = map_utils.fill_missing(inv, **NEAREST)
    np.testing.assert_array_equal(bits(np.asarray(filled[i][1])), bits(fill_missing_ref(inv, **NEAREST)))
    assert np.isfinite(np.asarray(m)).all()
    one_by_one[i] = (tg_box, m)
  args = (sc['tiles'], sc['meshes'], sc['tile_idx_to_xy'])
  kw = dict(offset=sc['offset'], margin=sc['margin'], order=sc['order'])
  ra = processor_warp.TileRenderer(*args, filled, sc['stride'], **kw)
  rb = processor_warp.TileRenderer(*args, one_by_one, sc['stride'], **kw)
  _, b, _, _ = sc['requests'][0]
  got = ra.render(b)
  np.testing.assert_array_equal(got, rb.render(b))
  assert got.any()
