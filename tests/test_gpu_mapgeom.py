"""map_utils.to_absolute / to_relative / outer_box / inner_box / make_affine_map
and warp.warp_points on the device: the reference's own output
(tests/golden/mapgeom.npz) and, on generated shapes that cross the kernels'
vector, wave and workgroup boundaries, the NumPy statement of tests/mapgeom_ref.py
(itself pinned to the reference by tests/test_mapgeom_refs.py)."""
import numpy as np
import pytest
import torch

from sofima_amd import map_utils, warp
from sofima_amd._dev import DeviceArray
from tests import mapgeom_ref as ref

pytestmark = pytest.mark.gpu

GOLD = ref.load_golden()
GEO = {r['name']: r for r in GOLD['geo']}
AFF = {r['name']: r for r in GOLD['aff']}
PTS = {r['name']: r for r in GOLD['pts']}


def bits_equal(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rand_map(seed, shape, dtype, amp=15.0, nan_frac=0.0):
  rng = np.random.default_rng(seed)
  m = rng.uniform(-amp, amp, shape).astype(dtype)
  if nan_frac:
    m[:, rng.random(shape[1:]) < nan_frac] = np.nan
    m[0][rng.random(shape[1:]) < nan_frac / 2] = np.nan   # one channel only
  return m


def box_of(shape, start):
  return ref.Box(start, shape[1:][::-1])


def strides_for(dim):
  return (30, 20.5, 10)[-dim:]


# -- to_absolute / to_relative -------------------------------------------------------
@pytest.mark.parametrize('name', list(GEO))
def test_shift_golden(name):
  rec = GEO[name]
  stride, box = ref.py_stride(rec['stride']), ref.geo_box(rec)
  before = rec['map'].copy()
  got = map_utils.to_absolute(rec['map'], stride, box)
  assert isinstance(got, DeviceArray)
  assert bits_equal(got, rec['abs'])
  assert bits_equal(map_utils.to_relative(got, stride, box), rec['rel'])
  assert bits_equal(rec['map'], before)


SHIFT_SHAPES = [(2, 1, 1, 1), (2, 3, 5, 7), (3, 4, 5, 6),
                (2, 2, 3, 1), (2, 2, 3, 3), (3, 2, 3, 4), (2, 2, 3, 5), (2, 2, 3, 257),
                (2, 1, 1, 1023), (3, 1, 1, 1024), (2, 1, 5, 205), (2, 1, 3, 341)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape', SHIFT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_shift_shapes(shape, dtype):
  """Vector body, scalar head and tail, channels that start off a 16-byte
  boundary (odd node counts), 256 k - 1 / 256 k / 256 k + 1 nodes."""
  dim = shape[0]
  m = rand_map(sum(shape), shape, dtype, nan_frac=0.05)
  stride = strides_for(dim)
  for box in (None, box_of(shape, (-7, 11, 2))):
    want = ref.to_absolute(m, stride, box)
    got = map_utils.to_absolute(m, stride, box)
    assert bits_equal(got, want)
    dev = map_utils.to_absolute(DeviceArray(torch.from_numpy(m).cuda()), stride, box)
    assert bits_equal(dev, got)
    # the round trip is NOT the identity in float32: compare with the statement
    assert bits_equal(map_utils.to_relative(got, stride, box),
                      ref.to_relative(want, stride, box))


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_shift_misaligned_device_input(dtype):
  """A contiguous device view that starts one element off the allocation."""
  shape = (2, 2, 5, 131)
  m = rand_map(1, shape, dtype)
  flat = torch.empty(m.size + 1, dtype=torch.from_numpy(m).dtype, device='cuda')
  flat[1:] = torch.from_numpy(m).cuda().reshape(-1)
  view = flat[1:].view(shape)
  assert view.is_contiguous() and view.data_ptr() % 16 != 0
  box = box_of(shape, (3, -5, 0))
  assert bits_equal(map_utils.to_absolute(view, 40, box), ref.to_absolute(m, 40, box))
  assert bits_equal(view.cpu().numpy(), m)
  assert bits_equal(map_utils.to_relative(DeviceArray(view), 40, box),
                    ref.to_relative(m, 40, box))


def test_shift_argument_errors():
  m = np.zeros((2, 2, 5, 7), np.float32)
  with pytest.raises(ValueError, match='mismatch with coord map'):
    map_utils.to_absolute(m, 40, ref.Box((0, 0, 0), (7, 6, 2)))
  with pytest.raises(ValueError, match='mismatch with coord map'):
    map_utils.to_relative(m, 40, (np.zeros(3, int), np.array([8, 5, 2])))
  # a (start, size) pair is a box too
  got = map_utils.to_absolute(m, 40, (np.array([1, 2, 3]), np.array([7, 5, 2])))
  assert bits_equal(got, ref.to_absolute(m, 40, ref.Box((1, 2, 3), (7, 5, 2))))


# -- outer_box / inner_box ---------------------------------------------------------
def same_box(got, start, size):
  return (np.array_equal(np.asarray(got.start), np.asarray(start)) and
          np.array_equal(np.asarray(got.size), np.asarray(size)))


@pytest.mark.parametrize('name', [n for n, r in GEO.items() if int(r['hasbox'])])
def test_boxes_golden(name):
  rec = GEO[name]
  stride, box = ref.py_stride(rec['stride']), ref.geo_box(rec)
  tl = ref.py_stride(rec['target_len'])
  if int(rec['outer_err']):
    with pytest.raises(ValueError):
      map_utils.outer_box(rec['map'], box, stride, tl)
  else:
    ob = map_utils.outer_box(rec['map'], box, stride, tl)
    assert isinstance(ob, ref.Box)
    assert same_box(ob, rec['outer_start'], rec['outer_size'])
  if 'inner_start' in rec:
    ib = map_utils.inner_box(rec['map'], box, stride)
    assert same_box(ib, rec['inner_start'], rec['inner_size'])
  else:
    with pytest.raises(NotImplementedError, match='fill_missing'):
      map_utils.inner_box(rec['map'], box, stride)


EXTENT_SHAPES = SHIFT_SHAPES[:8] + [(2, 2, 300, 517), (3, 9, 70, 131), (2, 1, 2, 70),
                                    (3, 5, 3, 64)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape', EXTENT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_outer_box_shapes(shape, dtype):
  dim = shape[0]
  stride = strides_for(dim)
  box = box_of(shape, (-400, 11, -3))          # negative absolute coordinates
  for seed, nan_frac in ((0, 0.0), (1, 0.2)):
    m = rand_map(seed + sum(shape), shape, dtype, amp=55.0, nan_frac=nan_frac)
    if nan_frac:
      m[:, 0, 0, 0] = 1.0                       # at least one valid node
    for tl in (None, 7, (16, 8, 4)[-dim:]):
      want = ref.outer_box(m, box, stride, tl)
      got = map_utils.outer_box(DeviceArray(torch.from_numpy(m).cuda()), box, stride, tl)
      assert same_box(got, want.start, want.size), (got, want)
  pair = map_utils.outer_box(m, (box.start, box.size), stride)
  want = ref.outer_box(m, box, stride)
  assert isinstance(pair, tuple) and pair[0].dtype.kind == 'i' and pair[1].dtype.kind == 'i'
  assert np.array_equal(pair[0], want.start) and np.array_equal(pair[1], want.size)


def test_outer_extents_are_the_statement_s():
  """The reduced scalars themselves, where the extreme sits in the last workgroup,
  the scalar tail or behind NaN."""
  shape = (2, 2, 300, 517)
  m = rand_map(3, shape, np.float32, nan_frac=0.1)
  m[0, 1, 299, 516] = 1e4
  m[1, 1, 299, 515] = -1e4
  box = box_of(shape, (5, 6, 0))
  res, dtype, _, _ = map_utils._extents(m, 40, box, 0)
  want = ref.outer_extents(m, 40, box)
  assert dtype == np.float32
  assert [np.float32(v) for v in res[:4]] == [want[0][0], want[0][1], want[1][0], want[1][1]]


def test_outer_box_all_nan_channel_raises():
  for shape in ((2, 2, 4, 5), (3, 2, 40, 70)):
    m = rand_map(0, shape, np.float32)
    m[shape[0] - 1] = np.nan
    with pytest.raises(ValueError, match='NaN'):
      map_utils.outer_box(m, box_of(shape, (0, 0, 0)), 40)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape', EXTENT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_inner_box_shapes(shape, dtype):
  dim = shape[0]
  stride = strides_for(dim)
  box = box_of(shape, (-400, 11, -3))
  m = rand_map(7 + sum(shape), shape, dtype, amp=9.0)
  want = ref.inner_box(m, box, stride)
  got = map_utils.inner_box(m, box, stride)
  assert isinstance(got, ref.Box)
  assert same_box(got, want.start, want.size), (got, want)
  res, _, _, _ = map_utils._extents(m, stride, box, 1)
  ext = ref.inner_extents(m, stride, box)
  assert [dtype(v) for v in res[:2 * dim]] == [v for pair in ext for v in pair]
  assert res[6] == 0
  # the deciding line is the last one of the last section
  m[:, -1, -1, :] += dtype(3.0)
  m[:, -1, :, -1] -= dtype(3.0)
  want = ref.inner_box(m, box, stride)
  assert same_box(map_utils.inner_box(DeviceArray(torch.from_numpy(m).cuda()), box, stride),
                  want.start, want.size)


@pytest.mark.parametrize('where', [(0, 0, 0, 0), (1, 1, 299, 516), (0, 1, 150, 63)])
def test_inner_box_nan_raises(where):
  shape = (2, 2, 300, 517)
  m = rand_map(5, shape, np.float32)
  m[where] = np.nan
  with pytest.raises(NotImplementedError, match='fill_missing'):
    map_utils.inner_box(m, box_of(shape, (0, 0, 0)), 40)
  m3 = rand_map(5, (3, 4, 5, 6), np.float64)
  m3[2, 3, 4, 5] = np.nan
  with pytest.raises(NotImplementedError, match='fill_missing'):
    map_utils.inner_box(m3, box_of(m3.shape, (0, 0, 0)), 40)


# -- make_affine_map ---------------------------------------------------------------
@pytest.mark.parametrize('name', list(AFF))
def test_affine_golden(name):
  rec = AFF[name]
  box = ref.Box(rec['start'], rec['size'])
  stride = ref.py_stride(rec['stride'])
  got = map_utils.make_affine_map(rec['matrix'], box, stride)
  assert isinstance(got, DeviceArray)
  got = np.asarray(got)
  assert got.dtype == np.float64 and got.shape == rec['out'].shape
  assert np.all(np.abs(got - rec['out']) <= ref.affine_bound(rec['matrix'], box, stride))


@pytest.mark.parametrize('size', [(1, 1, 1), (7, 5, 3), (257, 3, 2), (4, 5, 51), (64, 4, 1)],
                         ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['identity', 'translation', 'general'])
def test_affine_shapes(kind, size):
  """The kernel and the statement do the same IEEE operations in the same order
  (no contraction): equal bits, and inside the dot-product bound a fortiori."""
  rng = np.random.default_rng(len(kind) + sum(size))
  m = np.hstack([np.eye(3), np.zeros((3, 1))])
  if kind == 'translation':
    m[:, 3] = (3.25, -7.5, 11.0)
  elif kind == 'general':
    m = rng.uniform(-1.5, 1.5, (3, 4))
    m[:, 3] *= 40
  box = ref.Box((-13, 21, 5), size)
  for stride in (10, (2.5, 20, 40)):
    got = np.asarray(map_utils.make_affine_map(m, box, stride))
    want = ref.make_affine_map(m, box, stride)
    assert np.all(np.abs(got - want) <= ref.affine_bound(m, box, stride))
    assert bits_equal(got, want)
  if kind == 'identity':
    assert not got.any()


# -- warp_points -------------------------------------------------------------------
def cloud(seed, n, shape, start, stride, dtype, zs):
  """Points inside the grid, outside on every side, on nodes and on the last node."""
  rng = np.random.default_rng(seed)
  nz, ny, nx = shape[1:]
  x0, y0 = start[0] * stride, start[1] * stride
  w, h = (nx - 1) * stride, (ny - 1) * stride
  xy = rng.uniform([x0 - 0.7 * stride, y0 - 0.7 * stride],
                   [x0 + w + 0.7 * stride, y0 + h + 0.7 * stride], (n, 2))
  k = n // 4
  xy[:k] = rng.integers(0, [nx, ny], (k, 2)) * stride + [x0, y0]
  if n > 8:
    xy[k] = (x0 + w, y0 + h)
    xy[k + 1] = (x0 - 2.5 * stride, y0 + h + 3.25 * stride)
    xy[k + 2] = (x0 + w + 1.5 * stride, y0 - 1.25 * stride)
  p = np.concatenate([xy, rng.choice(zs, n)[:, None]], axis=1)
  return (np.round(p) if np.issubdtype(dtype, np.integer) else p).astype(dtype)


def check_points(points, m, box, stride):
  got = warp.warp_points(points, m, box, stride)
  want = ref.warp_points(points, m, box, stride)
  assert isinstance(got, np.ndarray) and got.dtype == points.dtype
  if np.issubdtype(points.dtype, np.integer):
    left_out = ref.check_points_int(got, want, ref.warp_points_f32(points, m, box, stride))
  else:
    left_out = ref.check_points_float(got, want)
  print(f'{len(points)} points: {left_out} off the exact value / left out')
  return got


@pytest.mark.parametrize('name', list(PTS))
def test_points_golden(name):
  rec = PTS[name]
  box = ref.Box(rec['start'], rec['map'].shape[1:][::-1])
  stride = ref.py_scalar(rec['stride'])
  before = rec['points'].copy()
  got = warp.warp_points(rec['points'], rec['map'], box, stride)
  assert bits_equal(rec['points'], before)
  if np.issubdtype(got.dtype, np.integer):
    ref.check_points_int(got, rec['out'],
                         ref.warp_points_f32(rec['points'], rec['map'], box, stride))
  else:
    ref.check_points_float(got, rec['out'])


@pytest.mark.parametrize('pdtype', [np.float32, np.float64, np.int32, np.int64],
                         ids=['pf32', 'pf64', 'pi32', 'pi64'])
@pytest.mark.parametrize('mdtype', [np.float32, np.float64], ids=['mf32', 'mf64'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 100000])
def test_points_counts_and_dtypes(n, mdtype, pdtype):
  shape = (2, 3, 6, 7)
  start = (5, -3, 10)
  m = rand_map(n, shape, mdtype)
  box = box_of(shape, start)
  pts = cloud(n + 1, n, shape, start, 40, pdtype, (10, 11, 12, 9, 8))   # 9, 8 wrap
  check_points(pts, m, box, 40)


@pytest.mark.parametrize('mdtype', [np.float32, np.float64], ids=['mf32', 'mf64'])
@pytest.mark.parametrize('shape', [(2, 1, 2, 2), (2, 2, 2, 9), (2, 2, 9, 2)],
                         ids=lambda s: 'x'.join(map(str, s)))
def test_points_small_maps(shape, mdtype):
  m = rand_map(2, shape, mdtype, amp=4.0)
  start = (-4, 2, -1)
  box = box_of(shape, start)
  for pdtype in (np.float64, np.int32):
    zs = [-1 + z for z in range(shape[1])] + [-2]
    check_points(cloud(3, 65, shape, start, 20.5, pdtype, zs), m, box, 20.5)


@pytest.mark.parametrize('pdtype', [np.float32, np.float64], ids=['pf32', 'pf64'])
@pytest.mark.parametrize('mdtype', [np.float32, np.float64], ids=['mf32', 'mf64'])
def test_points_nan_nodes(mdtype, pdtype):
  shape = (2, 3, 6, 7)
  m = rand_map(4, shape, mdtype)
  m[:, 0, 2:4, 2:5] = np.nan
  m[0, 1, 0, 0] = np.nan
  box = box_of(shape, (5, -3, 10))
  got = check_points(cloud(5, 500, shape, (5, -3, 10), 40, pdtype, (10, 11, 12)), m, box, 40)
  assert np.isnan(got[:, :2]).any() and not np.isnan(got[:, :2]).all()
  assert not np.isnan(got[:, 2]).any()


def test_points_input_kinds_and_empty():
  shape = (2, 3, 6, 7)
  m = rand_map(6, shape, np.float32)
  box = box_of(shape, (5, -3, 10))
  pts = cloud(7, 64, shape, (5, -3, 10), 40, np.float32, (10, 11))
  a = warp.warp_points(pts, m, box, 40)
  b = warp.warp_points(pts, DeviceArray(torch.from_numpy(m).cuda()), (box.start, box.size), 40)
  c = warp.warp_points(pts.tolist(), torch.from_numpy(m), box, 40.0)
  assert bits_equal(a, b) and np.array_equal(a.astype(np.float64), c)
  empty = warp.warp_points(pts[:0], m, box, 40)
  assert empty.shape == (0, 3) and empty.dtype == np.float32
  small = warp.warp_points(pts.astype(np.int16), m, box, 40)
  assert small.dtype == np.int16
  assert np.array_equal(small, ref.warp_points(pts.astype(np.int16), m, box, 40))


def test_points_errors():
  shape = (2, 3, 6, 7)
  m = rand_map(6, shape, np.float32)
  box = box_of(shape, (5, -3, 10))
  pts = cloud(7, 8, shape, (5, -3, 10), 40, np.float64, (10,))
  for z in (13, 6, 1e12):
    bad = pts.copy()
    bad[5, 2] = z
    with pytest.raises(IndexError):
      warp.warp_points(bad, m, box, 40)
  pts[5, 2] = 7.9           # int(-2.1) = -2 wraps; 12.9 is section 2
  pts[6, 2] = 12.9
  check_points(pts, m, box, 40)
  for bad_shape in ((2, 3, 1, 9), (2, 3, 9, 1)):
    with pytest.raises(ValueError, match='at least 2'):
      warp.warp_points(pts, np.zeros(bad_shape, np.float32), box_of(bad_shape, (0, 0, 10)), 40)
    with pytest.raises(ValueError, match='at least 2'):
      warp.warp_points(pts[:0], np.zeros(bad_shape, np.float32), box_of(bad_shape, (0, 0, 10)),
                       40)
