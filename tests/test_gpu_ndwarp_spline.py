"""Spline orders 2 to 5 on the device (-m gpu): the B-spline prefilter
(sfm_spline_prefilter), `spline_sample`, `warp.ndimage_warp(order=2..5)` and
`processor_warp.render` / `TileRenderer` with those orders.

The contract is the one of orders 0 and 1, bit for bit:
  * the reference's own output (tests/golden/ndimage_warp_spline.npz);
  * SciPy on the shapes where the kernels can go wrong, at coordinates on every
    edge of the sampler.  oracle.warp_oracle.ndimage_warp passes `order` through
    but computes float32 maps only, in which `len - 1 + 1e-9` does not exist: the
    edge coordinates come in float64 maps and go through map_coordinates twice
    in tests/ndwarp_spline_ref.py (`scipy_sampler`); the oracle serves the
    float32-map cases;
  * the coefficients themselves against tests/ndwarp_spline_ref.py, which
    tests/test_ndwarp_spline_ref.py pins to scipy.ndimage.spline_filter.
Integer images compare with array_equal, float32 images by their bits.

Orders 2 to 5 are opt-in (the switch SFM_SPLINE_ORDERS): every test of this module
runs with it set, except the one that checks the default.
"""
import types

import numpy as np
import pytest
import torch

from oracle import warp_oracle
from sofima_amd import _abi, _spline, processor_warp, warp
from tests import ndwarp_spline_ref as ref
from tests import render3d_ref
from tests.render3d_ref import box

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16, np.float32)
_ABI_DTYPE = {np.dtype(np.uint8): _abi.DTYPE_U8, np.dtype(np.uint16): _abi.DTYPE_U16,
              np.dtype(np.float32): _abi.DTYPE_F32}


def assert_same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    bits = np.uint32 if want.dtype == np.float32 else np.uint64
    differ = got.view(bits) != want.view(bits)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


@pytest.fixture(autouse=True)
def spline_orders(request):
  if request.node.name == 'test_orders_above_1_are_opt_in':
    yield
    return
  with _abi.option(_spline.OPTION, 1):
    yield


@pytest.fixture(scope='module')
def fixture(golden):
  return golden('ndimage_warp_spline')


@pytest.fixture(scope='module')
def scenes(golden):
  return render3d_ref.scenes(golden('render3d'))


def device_coeffs(img, order, dev):
  """The prefilter alone: float64 coefficients of a whole 2-D / 3-D array."""
  shape = (1,) * (3 - img.ndim) + img.shape
  view = img.view(np.int16) if img.dtype == np.uint16 else img
  t = torch.from_numpy(np.ascontiguousarray(view)).to(dev)
  ws, off = _spline.prefilter([(t.data_ptr(), shape, (shape[1] * shape[2], shape[2], 1))],
                              _ABI_DTYPE[img.dtype], order, dev)
  assert off == [0] and ws.dtype == torch.float64
  return ws.cpu().numpy()[:img.size].reshape(img.shape)


def warp_at(img, coords, order):
  """warp.ndimage_warp, and SciPy's map_coordinates twice, sampling `img` at
  `coords` [ndim, n]: a stride-1 float64 map as large as the output holds them as
  node values, which the order-1 step returns unchanged at the nodes (a NaN node
  also turns the node before it on every axis into NaN, in SciPy and here alike:
  NaNs go last)."""
  dim, n = coords.shape
  nan = np.isnan(coords).any(axis=0)
  coords = np.concatenate([coords[:, ~nan], coords[:, nan]], axis=1)
  width = 48
  rows = -(-n // width)
  out_shape = (1,) * (dim - 2) + (rows, width)
  full = np.zeros((dim, rows * width))
  full[:, :n] = coords
  absolute = full.reshape((dim,) + out_shape)[::-1]      # channels x, y[, z]
  idx = np.mgrid[tuple(slice(0, s) for s in out_shape)][::-1]
  cmap = np.ascontiguousarray(absolute - idx)
  stride = (1,) * dim
  zero = np.zeros(dim, np.int64)
  size = np.array(out_shape[::-1], np.int64)
  b = types.SimpleNamespace(start=zero, size=size)
  got = warp.ndimage_warp(img, cmap, stride, tuple(size), (0,) * dim, order=order,
                          image_box=types.SimpleNamespace(start=zero, size=zero),
                          map_box=b, out_box=b)
  want = ref.ndimage_warp(img, cmap, stride, order, image_start=zero, map_start=zero,
                          out_start=zero, out_size=size, scipy_sampler=True)
  return got, want


# -- the prefilter -----------------------------------------------------------------------
@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_prefilter_coefficients(gpu, order):
  """Every edge shape and dtype: the float64 coefficients, bit for bit."""
  rng = np.random.default_rng(100 + order)
  for shape in ref.EDGE_SHAPES + ((1, 1), (1, 1, 1), (130, 70), (3, 66, 33)):
    for dtype in DTYPES:
      img = ref.edge_image(rng, shape, dtype)
      assert_same(device_coeffs(img, order, gpu), ref.prefilter(img, order), (shape, dtype))


@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_far_voxel_reaches_the_line_start(gpu, order):
  """An all-zero image with one non-zero voxel at the far end of a 200-long axis:
  an initialisation sweep that is cut short loses its trace at the line's start."""
  big = np.finfo(np.float32).max
  for shape, far in (((3, 200), (1, 199)), ((200, 3), (199, 2)), ((200, 2, 3), (199, 1, 1)),
                     ((2, 200, 3), (1, 199, 2))):
    img = np.zeros(shape, np.float32)
    img[far] = big
    want = ref.prefilter(img, order)
    near = tuple(0 if n == 200 else f for n, f in zip(shape, far))
    assert want[near] != 0.0
    assert_same(device_coeffs(img, order, gpu), want, shape)
    img8 = (img != 0).astype(np.uint8) * np.uint8(255)
    assert_same(device_coeffs(img8, order, gpu), ref.prefilter(img8, order), shape)
  # ... and through ndimage_warp, sampled along the first voxels of that line
  img = np.zeros((3, 200), np.float32)
  img[1, 199] = big
  coords = np.stack([np.full(40, 1.0), np.linspace(0.0, 9.75, 40)])
  got, want = warp_at(img, coords, order)
  assert_same(got, want)


def test_regions_of_a_larger_array_in_one_batch(gpu):
  """Three regions of one array (one a single plane, one a single column) through one
  table: each is filtered where it lies, mirrored at its own edges."""
  rng = np.random.default_rng(5)
  arr = rng.integers(0, 65536, (6, 40, 70)).astype(np.uint16)
  t = torch.from_numpy(arr.view(np.int16)).to(gpu)
  pitch = (40 * 70, 70, 1)
  crops = [((1, 3, 2), (4, 30, 67)), ((2, 0, 5), (1, 40, 33)), ((0, 7, 69), (6, 9, 1))]
  regions = [(t.data_ptr() + 2 * sum(a * p for a, p in zip(start, pitch)), size, pitch)
             for start, size in crops]
  ws, offsets = _spline.prefilter(regions, _abi.DTYPE_U16, 3, gpu)
  ws = ws.cpu().numpy()
  for (start, size), off in zip(crops, offsets):
    sl = tuple(slice(a, a + n) for a, n in zip(start, size))
    got = ws[off:off + int(np.prod(size))].reshape(size)
    assert_same(got, ref.prefilter(arr[sl], 3), (start, size))


# -- ndimage_warp ------------------------------------------------------------------------
def test_ndimage_warp_fixture(gpu, fixture):
  for c in ref.warp_cases(fixture):
    kw = {}
    if c['boxes'] is not None:
      kw = {k + '_box': types.SimpleNamespace(start=c['boxes'][k][0], size=c['boxes'][k][1])
            for k in ('image', 'map', 'out')}
    got = warp.ndimage_warp(c['image'], c['map'], c['stride'], c['work'], c['overlap'],
                            order=c['order'], parallelism=2, **kw)
    assert_same(got, c['warped'], c['name'])


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_edge_shapes_against_scipy(gpu, order, dtype):
  rng = np.random.default_rng(1000 + 10 * order + np.dtype(dtype).itemsize)
  for shape in ref.EDGE_SHAPES:
    img = ref.edge_image(rng, shape, dtype)
    coords = ref.edge_coords(rng, shape, order, n_random=100)
    got, want = warp_at(img, coords, order)
    assert_same(got, want, shape)
    assert np.mean(want != 0) > 0.2, shape


def test_work_size_and_overlap_do_not_matter(gpu, fixture):
  c = next(c for c in ref.warp_cases(fixture) if c['name'] == 'u8_3d_o3')
  for work, ov in (((64, 64, 16), (0, 0, 0)), ((7, 5, 2), (3, 2, 1)), ((36, 30, 9), (1, 1, 1))):
    got = warp.ndimage_warp(c['image'], c['map'], c['stride'], work, ov, order=3)
    assert_same(got, c['warped'], (work, ov))


def test_random_volume_against_scipy(gpu):
  """More than one workgroup on every pass; maps that leave the image."""
  rng = np.random.default_rng(77)
  img = (rng.standard_normal((21, 90, 77)) * 50).astype(np.float32)
  cmap = (rng.standard_normal((3, 6, 11, 9)) * 6).astype(np.float32)
  stride = (4.5, 9.0, 9.5)
  for order in (3, 5):
    got = warp.ndimage_warp(img, cmap, stride, (64, 64, 16), (8, 8, 2), order=order)
    assert_same(got, warp_oracle.ndimage_warp(img, cmap, stride, order=order), order)


# -- the render --------------------------------------------------------------------------
def test_render_fixture(gpu, fixture, scenes):
  for sc, order, reqs in ref.render_cases(fixture, scenes):
    r = processor_warp.TileRenderer(sc['tiles'], sc['meshes'], sc['tile_idx_to_xy'],
                                    sc['inverted'], sc['stride'], offset=sc['offset'],
                                    margin=sc['margin'], order=order)
    for name, b, plan, want in reqs:
      got_plan = r.plan(b)
      assert render3d_ref.same_plan(got_plan, plan), (sc['name'], name)
      assert_same(r.render(b, plan=got_plan), want, (sc['name'], order, name))
    # ... and through the function, on NumPy inputs
    name, b, plan, want = reqs[-5]
    got = processor_warp.render(b, sc['tiles'], plan, sc['inverted'], sc['weights'],
                                sc['stride'], order=order)
    assert_same(got, want, (sc['name'], order, name))


def _montage(seed, dtype):
  """2 x 2 tiles of (4, 24, 24); tile 3 is sent to its plane 2 alone, so its crop is one
  voxel thick; the crops of the others differ with their maps."""
  from tests.test_gpu_render3d import grid_montage
  m = grid_montage(seed, (4, 24, 24), (2, 4, 4), (2, 2), 4, dtype=dtype, margin=1)
  tg_box, inv = m['inverted'][3]
  z_nodes = (tg_box.start[2] + np.arange(tg_box.size[2])) * 2.0
  inv[2] = 2.0 - z_nodes[:, None, None]
  return m


@pytest.mark.parametrize('seed,dtype', [(31, np.uint8), (32, np.uint16), (33, np.float32)])
def test_fused_equals_the_sequence(gpu, seed, dtype):
  """One kernel on batched crop coefficients == per tile warp.ndimage_warp(order=3) of
  the crop and order 1 of the weights, and the NumPy blend in ascending tile index."""
  m = _montage(seed, dtype)
  b = box((-2, -1, -1), (48, 46, 6))
  plan = processor_warp.plan_render(b, m['boxes'], m['inverted'], m['xy'], m['tile_shape'],
                                    m['stride'])
  assert [item[0] for item in plan] == [0, 1, 2, 3]
  sizes = [tuple(int(v) for v in item[1].size) for item in plan]
  assert len(set(sizes)) > 1 and sizes[3][2] == 1
  pairs = []
  for i, data_box, tg_box, lw_box, _ in plan:
    sl = tuple(slice(int(a), int(a + n)) for a, n in zip(data_box.start[::-1],
                                                        data_box.size[::-1]))
    kw = dict(image_box=data_box, map_box=tg_box, out_box=lw_box)
    image = warp.ndimage_warp(m['tiles'][i][sl], m['inverted'][i][1], m['stride'],
                              (32, 32, 8), (0, 0, 0), order=3, **kw)
    dts = np.repeat(m['weights'][i][sl[1:]][None], int(data_box.size[2]), axis=0)
    pairs.append((image, warp.ndimage_warp(dts, m['inverted'][i][1], m['stride'],
                                           (32, 32, 8), (0, 0, 0), **kw)))
  args = (b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'])
  got = processor_warp.render(*args, order=3)
  assert_same(got, render3d_ref.blend(b, plan, pairs, dtype))
  # (the montage is 44 x 44 x 4 of the 48 x 46 x 6 box, 0.58 of it, less the rim that
  # margin = 1 and the map jitter leave dark: at least half of that share is rendered)
  assert np.mean(got != 0) > 0.29
  linear = processor_warp.render(*args, order=1)
  assert np.mean(got != linear) > 0.25
  # ... the restatement agrees, and float32 output of the same sums
  assert_same(got, ref.render(*args, 3))
  got32 = processor_warp.render(*args, order=3, out_dtype=np.float32)
  assert_same(got32, render3d_ref.blend(b, plan, pairs, np.float32))


@pytest.mark.parametrize('order', [2, 4, 5])
def test_render_other_orders_against_the_restatement(gpu, order):
  m = _montage(40 + order, np.uint8)
  b = box((5, 3, 0), (30, 33, 4))
  plan = processor_warp.plan_render(b, m['boxes'], m['inverted'], m['xy'], m['tile_shape'],
                                    m['stride'])
  assert len(plan) == 4
  args = (b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'])
  assert_same(processor_warp.render(*args, order=order), ref.render(*args, order))


# -- the old paths and what stays unbuilt ----------------------------------------------
def test_orders_0_and_1_give_the_same_bytes(gpu, fixture, golden, scenes):
  old = golden('ndimage_warp')
  args = (old['u8_3d_image'], old['u8_3d_map'], tuple(int(v) for v in old['u8_3d_stride']),
          tuple(old['u8_3d_work']), tuple(old['u8_3d_overlap']))
  sc = scenes[0]
  name, b, plan, _ = sc['requests'][1]
  assert name == 'cut67'
  for order in (0, 1):
    assert_same(warp.ndimage_warp(*args, order=order), fixture[f'guard_ndwarp_o{order}'])
    got = processor_warp.render(b, sc['tiles'], plan, sc['inverted'], sc['weights'],
                                sc['stride'], order=order)
    assert_same(got, fixture[f'guard_render_o{order}'])


def test_orders_above_1_are_opt_in(gpu):
  """Without the switch the two functions are what they were: orders 2 to 5 raise, and
  the message names the switch; 0 switches them off again."""
  m = _montage(51, np.uint8)
  b = box((0, 0, 0), (16, 12, 4))
  plan = processor_warp.plan_render(b, m['boxes'], m['inverted'], m['xy'], m['tile_shape'],
                                    m['stride'])
  args = (b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'])
  img = np.arange(72, dtype=np.uint8).reshape(8, 9)
  cmap = np.zeros((2, 2, 2), np.float32)
  assert _abi.get_option(_spline.OPTION) in (None, '0')

  def both_raise():
    for order in _spline.ORDERS:
      with pytest.raises(NotImplementedError, match=_spline.OPTION):
        warp.ndimage_warp(img, cmap, (8, 8), (8, 8), (0, 0), order=order)
      with pytest.raises(NotImplementedError, match=_spline.OPTION):
        processor_warp.render(*args, order=order)

  both_raise()
  with _abi.option(_spline.OPTION, 1):
    assert warp.ndimage_warp(img, cmap, (8, 8), (8, 8), (0, 0), order=3).any()
    assert processor_warp.render(*args, order=3).any()
    with _abi.option(_spline.OPTION, 0):
      both_raise()
  both_raise()


def test_what_is_not_built_raises(gpu):
  img = np.zeros((8, 9), np.uint8)
  cmap = np.zeros((2, 2, 2), np.float32)
  for order in (6, -1):
    with pytest.raises(NotImplementedError):
      warp.ndimage_warp(img, cmap, (8, 8), (8, 8), (0, 0), order=order)
  with pytest.raises(NotImplementedError):
    warp.ndimage_warp(img.astype(np.uint64), cmap, (8, 8), (8, 8), (0, 0), order=3)
  with pytest.raises(NotImplementedError):
    warp.ndimage_warp(img.astype(np.int32), cmap, (8, 8), (8, 8), (0, 0), order=3)
  with pytest.raises(NotImplementedError):
    warp.ndimage_warp(img, cmap, (8, 8), (8, 8), (0, 0), order=3,
                      map_coordinates=lambda *a, **k: None)
  m = _montage(50, np.uint8)
  b = box((0, 0, 0), (16, 12, 4))
  plan = processor_warp.plan_render(b, m['boxes'], m['inverted'], m['xy'], m['tile_shape'],
                                    m['stride'])
  with pytest.raises(NotImplementedError):
    processor_warp.render(b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'], order=6)
