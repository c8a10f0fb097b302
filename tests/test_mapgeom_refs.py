"""The NumPy statement of the map geometry helpers (tests/mapgeom_ref.py) against
the reference's own output (tests/golden/mapgeom.npz), and proof that the
fixture holds what the GPU tests rely on: NaN holes, points outside the grid,
an all-NaN channel, a NaN map that inner_box refuses."""
import numpy as np
import pytest

from tests import mapgeom_ref as ref

GOLD = ref.load_golden()
GEO = {r['name']: r for r in GOLD['geo']}
AFF = {r['name']: r for r in GOLD['aff']}
PTS = {r['name']: r for r in GOLD['pts']}


def bits_equal(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', list(GEO))
def test_shift_is_bit_exact(name):
  rec = GEO[name]
  stride, box = ref.py_stride(rec['stride']), ref.geo_box(rec)
  before = rec['map'].copy()
  assert bits_equal(ref.to_absolute(rec['map'], stride, box), rec['abs'])
  assert bits_equal(ref.to_relative(rec['abs'], stride, box), rec['rel'])
  assert bits_equal(rec['map'], before)


@pytest.mark.parametrize('name', [n for n, r in GEO.items() if int(r['hasbox'])])
def test_boxes_are_exact(name):
  rec = GEO[name]
  stride, box = ref.py_stride(rec['stride']), ref.geo_box(rec)
  tl = ref.py_stride(rec['target_len'])
  if int(rec['outer_err']):
    with pytest.raises(ValueError):
      ref.outer_box(rec['map'], box, stride, tl)
  else:
    ob = ref.outer_box(rec['map'], box, stride, tl)
    assert np.array_equal(ob.start, rec['outer_start'])
    assert np.array_equal(ob.size, rec['outer_size'])
  if 'inner_start' in rec:
    ib = ref.inner_box(rec['map'], box, stride)
    assert np.array_equal(np.asarray(ib.start, np.float64), rec['inner_start'])
    assert np.array_equal(np.asarray(ib.size, np.float64), rec['inner_size'])
  else:
    assert np.isnan(rec['map']).any()
    with pytest.raises(NotImplementedError, match='fill_missing'):
      ref.inner_box(rec['map'], box, stride)


def test_box_size_mismatch_raises():
  rec = GEO['c2_f32_scalar']
  bad = ref.Box(rec['start'], rec['size'] + 1)
  with pytest.raises(ValueError, match='mismatch with coord map'):
    ref.to_absolute(rec['map'], 40, bad)
  with pytest.raises(ValueError, match='mismatch with coord map'):
    ref.to_relative(rec['map'], 40, bad)


@pytest.mark.parametrize('name', list(AFF))
def test_affine_within_the_dot_product_bound(name):
  rec = AFF[name]
  box = ref.Box(rec['start'], rec['size'])
  stride = ref.py_stride(rec['stride'])
  got = ref.make_affine_map(rec['matrix'], box, stride)
  assert got.dtype == np.float64 and got.shape == rec['out'].shape
  assert np.all(np.abs(got - rec['out']) <= ref.affine_bound(rec['matrix'], box, stride))


@pytest.mark.parametrize('name', list(PTS))
def test_points_meet_the_cap(name):
  rec = PTS[name]
  box = ref.Box(rec['start'], rec['map'].shape[1:][::-1])
  stride = ref.py_scalar(rec['stride'])
  got = ref.warp_points(rec['points'], rec['map'], box, stride)
  if np.issubdtype(got.dtype, np.integer):
    f32 = ref.warp_points_f32(rec['points'], rec['map'], box, stride)
    assert ref.check_points_int(got, rec['out'], f32) == 0
  else:
    ref.check_points_float(got, rec['out'])


def test_fixture_is_not_vacuous():
  holes = GEO['c2_f32_holes']
  assert np.isnan(holes['map']).any() and not np.isnan(holes['map']).all()
  assert np.isnan(holes['abs']).sum() == np.isnan(holes['map']).sum()
  assert int(holes['outer_err']) == 0
  assert int(GEO['c2_f32_all_nan_channel']['outer_err']) == 1
  assert {r['map'].shape[0] for r in GEO.values()} == {2, 3}
  assert {r['map'].dtype for r in GEO.values()} == {np.dtype('f4'), np.dtype('f8')}
  assert any((r['start'] < 0).any() for r in GEO.values())
  # the float32 rounding of the offset sum is visible somewhere
  big = GEO['c2_f32_large_coords']
  exact = big['map'][0].astype(np.float64) + ref._offsets(
      big['map'].shape[1:], (40, 40), ref.geo_box(big))[0]
  assert np.any(exact != big['abs'][0])
  # points lie outside the grid on every side, on nodes, and sections wrap
  rec = PTS['m32_float64']
  nz, ny, nx = rec['map'].shape[1:]
  s = float(rec['stride'])
  x = rec['points'][:, 0] / s - rec['start'][0]
  y = rec['points'][:, 1] / s - rec['start'][1]
  assert (x < 0).any() and (x > nx - 1).any() and (y < 0).any() and (y > ny - 1).any()
  assert ((x == np.round(x)) & (y == np.round(y))).sum() >= 10
  assert ((x == nx - 1) & (y == ny - 1)).any()
  assert (rec['points'][:, 2] < rec['start'][2]).any()
  assert {r['points'].dtype for r in PTS.values()} == {
      np.dtype('f4'), np.dtype('f8'), np.dtype('i4'), np.dtype('i8')}
  nan = PTS['nan_nodes_f32']
  assert np.isnan(nan['out'][:, :2]).any() and not np.isnan(nan['out'][:, :2]).all()


def test_points_section_rules():
  rec = PTS['m32_float32']
  box = ref.Box(rec['start'], rec['map'].shape[1:][::-1])
  p = rec['points'][:3].copy()
  p[0, 2] = rec['start'][2] + rec['map'].shape[1]          # one past the last section
  with pytest.raises(IndexError):
    ref.warp_points(p, rec['map'], box, 40)
  p[0, 2] = rec['start'][2] - rec['map'].shape[1] - 1
  with pytest.raises(IndexError):
    ref.warp_points(p, rec['map'], box, 40)
  with pytest.raises(ValueError):
    ref.warp_points(rec['points'][:3], rec['map'][:, :, :1], ref.Box(rec['start'], (7, 1, 3)), 40)
  empty = ref.warp_points(rec['points'][:0], rec['map'], box, 40)
  assert empty.shape == (0, 3) and empty.dtype == rec['points'].dtype
