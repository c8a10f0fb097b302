"""processor_warp on the device (-m gpu): the fused warp-and-blend kernel
(`render_tiles_kernel`, sfm_render_tiles3d) and its planning.

Parity is exact everywhere -- the kernel's operations are the reference's, in
its order and precision -- so every comparison is assert_array_equal:
  * the golden scenes: what the reference's StitchAndRender3dTiles.process
    returned (tests/golden/render3d.npz), boxes, plans and weights included;
  * fused versus sequence: two warp.ndimage_warp calls per tile (the kernel that
    is pinned already) and the NumPy blend in ascending tile index;
  * edge shapes against tests/render3d_ref.py, the SciPy restatement that
    tests/test_render3d_host.py pins to the reference.
"""
import numpy as np
import pytest
import torch

from sofima_amd import processor_warp
from sofima_amd import warp
from sofima_amd._dev import DeviceArray
from tests import render3d_ref
from tests.render3d_ref import box

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def scenes(golden):
  return render3d_ref.scenes(golden('render3d'))


# -- golden scenes -----------------------------------------------------------------
def test_golden_scenes(gpu, scenes):
  for sc in scenes:
    r = processor_warp.TileRenderer(sc['tiles'], sc['meshes'], sc['tile_idx_to_xy'],
                                    sc['inverted'], sc['stride'], offset=sc['offset'],
                                    margin=sc['margin'], order=sc['order'])
    for i, pair in sc['boxes'].items():
      for a, b in zip(r.boxes[i], pair):
        np.testing.assert_array_equal(a.start, b.start)
        np.testing.assert_array_equal(a.size, b.size)
      np.testing.assert_array_equal(r.weights[i].cpu().numpy(), sc['weights'][i])
    for name, b, plan, want in sc['requests']:
      got_plan = r.plan(b)
      assert render3d_ref.same_plan(got_plan, plan), (sc['name'], name)
      got = r.render(b, plan=got_plan)
      assert got.dtype == want.dtype
      np.testing.assert_array_equal(got, want, err_msg=f"{sc['name']} {name}")


def test_golden_scenes_through_the_functions(gpu, scenes):
  """tile_boxes / plan_render / render on NumPy inputs, the canvas and the cutting
  request of every scene."""
  for sc in scenes:
    shape = sc['tiles'][0].shape
    boxes = processor_warp.tile_boxes(sc['meshes'], sc['tile_idx_to_xy'], shape, sc['stride'],
                                      sc['offset'])
    weights = {i: processor_warp.blend_weights(shape, *sc['tile_idx_to_xy'][i], (2, 2),
                                               sc['margin']) for i in boxes}
    for name, b, plan, want in sc['requests'][:2]:
      got_plan = processor_warp.plan_render(b, boxes, sc['inverted'], sc['tile_idx_to_xy'],
                                            shape, sc['stride'], sc['offset'])
      assert render3d_ref.same_plan(got_plan, plan), (sc['name'], name)
      got = processor_warp.render(b, sc['tiles'], got_plan, sc['inverted'], weights,
                                  sc['stride'], order=sc['order'])
      np.testing.assert_array_equal(got, want, err_msg=f"{sc['name']} {name}")


# -- synthetic montages --------------------------------------------------------------
def montage(seed, xy, tile_shape, stride, starts, region_nodes, dtype=np.uint8, amp=1.5,
            margin=0):
  """Tiles, inverted maps, weights and tile boxes made up directly.  Tile i sits at
  grid position xy[i] and renders the global region starts[i] (xyz) of
  region_nodes (xyz) map cells; its inverted map covers that region and one node
  more on every side, and sends it back onto the tile, with a jitter of `amp`."""
  rng = np.random.default_rng(seed)
  tz, ty_, tx_ = tile_shape
  sxyz = np.array(stride[::-1])
  grid = (max(p[1] for p in xy.values()) + 1, max(p[0] for p in xy.values()) + 1)
  tiles, inverted, weights, boxes = {}, {}, {}, {}
  for i, (gx, gy) in xy.items():
    if np.dtype(dtype) == np.float32:
      tiles[i] = rng.uniform(-50, 300, tile_shape).astype(np.float32)
    else:
      tiles[i] = rng.integers(0, np.iinfo(dtype).max + 1, tile_shape).astype(dtype)
    local = np.array(starts[i]) - (gx * tx_, gy * ty_, 0)
    assert np.all(local % sxyz == 0)
    nodes = np.array(region_nodes) + 3
    tg_box = box(local // sxyz - 1, nodes)
    inv = rng.uniform(-amp, amp, (3,) + tuple(nodes[::-1]))
    inv -= local.reshape(3, 1, 1, 1)
    inverted[i] = (tg_box, inv)
    weights[i] = processor_warp.blend_weights(tile_shape, gx, gy, grid, margin)
    boxes[i] = (box(starts[i], np.array(region_nodes) * sxyz), None)
  return dict(xy=xy, tile_shape=tile_shape, stride=stride, tiles=tiles, inverted=inverted,
              weights=weights, boxes=boxes)


def grid_montage(seed, tile_shape, stride, grid_yx, overlap, **kw):
  xy, starts, i = {}, {}, 0
  for gy in range(grid_yx[0]):
    for gx in range(grid_yx[1]):
      xy[i] = (gx, gy)
      starts[i] = (gx * (tile_shape[2] - overlap), gy * (tile_shape[1] - overlap), 0)
      i += 1
  nodes = tuple(int(n // s) for n, s in zip(tile_shape[::-1], stride[::-1]))
  return montage(seed, xy, tile_shape, stride, starts, nodes, **kw)


def plan_of(m, b):
  return processor_warp.plan_render(b, m['boxes'], m['inverted'], m['xy'], m['tile_shape'],
                                    m['stride'])


def check(m, b, order=1, out_dtype=None, min_items=1, **kw):
  plan = plan_of(m, b)
  assert len(plan) >= min_items
  want = render3d_ref.render(b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'],
                             order, out_dtype)
  got = processor_warp.render(b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'],
                              order=order, out_dtype=out_dtype, **kw)
  got = np.asarray(got)
  assert got.dtype == want.dtype and got.shape == want.shape
  np.testing.assert_array_equal(got, want)
  return plan, got


@pytest.mark.parametrize('seed,dtype,order,margin', [
    (1, np.uint8, 1, 0), (2, np.uint8, 0, 2), (3, np.uint16, 1, 2), (4, np.float32, 1, 0),
    (5, np.float32, 0, 2), (6, np.uint16, 0, 0)])
def test_fused_equals_the_sequence(gpu, seed, dtype, order, margin):
  """One kernel == per tile warp.ndimage_warp of the image and of the weights, and
  the NumPy blend in ascending tile index."""
  m = grid_montage(seed, (6, 20, 24), (2, 4, 4), (2, 2), 4, dtype=dtype, margin=margin)
  b = box((-3, -2, -1), (51, 41, 8))
  plan = plan_of(m, b)
  assert [item[0] for item in plan] == [0, 1, 2, 3]
  pairs = []
  for i, data_box, tg_box, lw_box, _ in plan:
    sl = tuple(slice(int(a), int(a + n)) for a, n in zip(data_box.start[::-1],
                                                        data_box.size[::-1]))
    kw = dict(image_box=data_box, map_box=tg_box, out_box=lw_box)
    image = warp.ndimage_warp(m['tiles'][i][sl], m['inverted'][i][1], m['stride'],
                              (32, 32, 8), (0, 0, 0), order=order, **kw)
    dts = np.repeat(m['weights'][i][sl[1:]][None], int(data_box.size[2]), axis=0)
    pairs.append((image, warp.ndimage_warp(dts, m['inverted'][i][1], m['stride'],
                                           (32, 32, 8), (0, 0, 0), **kw)))
  want = render3d_ref.blend(b, plan, pairs, dtype)
  got = processor_warp.render(b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'],
                              order=order)
  np.testing.assert_array_equal(got, want)
  # (the montage is 44 x 36 x 6 of the 51 x 41 x 8 box; two voxels of rim may stay dark)
  assert np.mean(got != 0) > 40 * 32 * 4 / (51 * 41 * 8) - 0.01
  # ... and float32 output of the same sums
  got32 = processor_warp.render(b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'],
                                order=order, out_dtype=np.float32)
  np.testing.assert_array_equal(got32, render3d_ref.blend(b, plan, pairs, np.float32))


# -- edge shapes ---------------------------------------------------------------------
def test_tile_and_map_of_two_nodes(gpu):
  rng = np.random.default_rng(11)
  tile = rng.integers(0, 256, (2, 2, 2)).astype(np.uint8)
  inv = rng.uniform(-0.4, 0.4, (3, 2, 2, 2))
  m = dict(xy={0: (0, 0)}, tile_shape=(2, 2, 2), stride=(1, 1, 1), tiles={0: tile},
           inverted={0: (box((0, 0, 0), (2, 2, 2)), inv)},
           weights={0: processor_warp.blend_weights((2, 2, 2), 0, 0, (1, 1), 0)},
           boxes={0: (box((0, 0, 0), (2, 2, 2)), None)})
  _, got = check(m, box((-1, -1, -1), (4, 4, 4)))
  assert got.any() and not got[0].any()


def test_data_box_of_one_plane(gpu):
  """The z channel sends everything to plane 2 of the tile: data_box is one plane
  thick, the z coordinate in it is exactly 0, on the first and last sample at once."""
  m = grid_montage(12, (4, 12, 16), (2, 4, 4), (1, 1), 0)
  tg_box, inv = m['inverted'][0]
  z_nodes = (tg_box.start[2] + np.arange(tg_box.size[2])) * 2.0
  inv[2] = 2.0 - z_nodes[:, None, None]
  plan, got = check(m, box((0, 0, 0), (16, 12, 4)))
  assert int(plan[0][1].size[2]) == 1 and int(plan[0][1].start[2]) == 2
  assert got.any()


def test_one_voxel_and_67_wide_requests(gpu):
  m = grid_montage(13, (3, 10, 48), (1, 2, 4), (1, 2), 8, dtype=np.uint16, margin=1)
  _, got = check(m, box((43, 5, 1), (1, 1, 1)), min_items=2)
  assert got.shape == (1, 1, 1)
  plan, got = check(m, box((5, 1, 0), (67, 7, 3)), min_items=2)
  assert got.shape == (3, 7, 67) and np.mean(got != 0) > 0.5
  check(m, box((5, 1, 0), (67, 7, 3)), order=0, min_items=2)


def test_five_tiles_on_one_voxel(gpu):
  """All five tiles of a 5 x 1 grid render the same spot."""
  xy = {i: (i, 0) for i in range(5)}
  m = montage(14, xy, (4, 16, 12), (2, 4, 4), {i: (0, 0, 0) for i in range(5)}, (4, 4, 2),
              dtype=np.float32)
  b = box((-2, -1, 0), (20, 18, 4))
  plan, got = check(m, b, min_items=5)
  assert [item[0] for item in plan] == [0, 1, 2, 3, 4]
  v = np.array((5, 6, 1))
  assert all(np.all(item[4].start <= v) and np.all(v < item[4].start + item[4].size)
             for item in plan)
  assert got[1, 7, 7] != 0
  # the same voxel alone
  one = processor_warp.render(box(v, (1, 1, 1)), m['tiles'], plan_of(m, box(v, (1, 1, 1))),
                              m['inverted'], m['weights'], m['stride'])
  assert one[0, 0, 0] == got[1, 7, 7]


def test_empty_plan_renders_zeros(gpu):
  m = grid_montage(15, (4, 12, 16), (2, 4, 4), (1, 1), 0, dtype=np.uint16)
  b = box((400, 300, 50), (70, 5, 2))
  assert plan_of(m, b) == []
  got = processor_warp.render(b, m['tiles'], [], m['inverted'], m['weights'], m['stride'])
  assert got.dtype == np.uint16 and got.shape == (2, 5, 70) and not got.any()


def test_nan_in_an_inverted_map(gpu):
  """The voxels whose coordinates interpolate the NaN node sample 0 for image and
  weight, as in SciPy; the others are untouched."""
  m = grid_montage(16, (6, 20, 24), (2, 4, 4), (1, 2), 4, dtype=np.uint8)
  b = box((0, 0, 0), (44, 20, 6))
  _, clean = check(m, b, min_items=2)
  m['inverted'][0][1][0, 2, 3, 3] = np.nan
  _, got = check(m, b, min_items=2)
  changed = got != clean
  assert changed.any() and np.mean(changed) < 0.2
  assert not got[changed][:1].any() or np.mean(got[changed] == 0) > 0.5


def test_device_tiles_and_device_output(gpu):
  m = grid_montage(17, (6, 20, 24), (2, 4, 4), (2, 2), 4, dtype=np.uint8)
  b = box((3, 2, 1), (40, 30, 4))
  plan = plan_of(m, b)
  want = render3d_ref.render(b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'])
  dev_tiles = {i: DeviceArray(torch.from_numpy(t).to(gpu)) for i, t in m['tiles'].items()}
  for i, t in dev_tiles.items():   # used where they lie
    assert processor_warp._device_tile(t, gpu).data_ptr() == t.tensor.data_ptr()
  dev_inv = {i: (tg, DeviceArray(torch.from_numpy(inv).to(gpu)))
             for i, (tg, inv) in m['inverted'].items()}
  assert render3d_ref.same_plan(
      processor_warp.plan_render(b, m['boxes'], dev_inv, m['xy'], m['tile_shape'], m['stride']),
      plan)
  got = processor_warp.render(b, dev_tiles, plan, dev_inv, m['weights'], m['stride'],
                              device_output=True)
  assert isinstance(got, DeviceArray) and got.tensor.is_cuda and got.dtype == np.uint8
  np.testing.assert_array_equal(np.asarray(got), want)


def test_what_is_not_built_raises(gpu):
  m = grid_montage(18, (4, 12, 16), (2, 4, 4), (1, 1), 0)
  b = box((0, 0, 0), (16, 12, 4))
  plan = plan_of(m, b)
  args = (b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'])
  with pytest.raises(NotImplementedError):
    processor_warp.render(*args, order=3)
  with pytest.raises(NotImplementedError):
    processor_warp.render(*args, out_dtype=np.uint16)
  with pytest.raises(NotImplementedError):
    processor_warp.render(b, {0: m['tiles'][0].astype(np.uint64)}, *args[2:])
