"""The host side of processor_warp (no GPU): the closed-form blending weights
against SciPy's distance transform, the box arithmetic of tile_boxes /
plan_render against the boxes the reference produced (tests/golden/render3d.npz;
the device `outer_box` is replaced by a NumPy one), and the NumPy / SciPy
restatement of the render loop (tests/render3d_ref.py), which serves the GPU
tests as reference, bit for bit against the reference's rendered volumes."""
import numpy as np
import pytest
from scipy import ndimage

from sofima_amd import map_utils
from sofima_amd import processor_warp
from tests import render3d_ref


@pytest.fixture(scope='module')
def scenes(golden):
  return render3d_ref.scenes(golden('render3d'))


@pytest.fixture
def numpy_outer_box(monkeypatch):
  monkeypatch.setattr(map_utils, 'outer_box', render3d_ref.outer_box_np)


def _edt_weights(shape_yx, tx, ty, grid_yx, margin):
  """processor/warp.py:147-161 with edt.edt(mask, black_border=True) written as the
  SciPy transform of the mask padded with background."""
  mask = np.zeros(shape_yx, dtype=bool)
  if margin > 0:
    x0 = margin if tx > 0 else 0
    x1 = -margin if tx < grid_yx[-1] - 1 else -1
    y0 = margin if ty > 0 else 0
    y1 = -margin if ty < grid_yx[-2] - 1 else -1
    mask[y0:y1, x0:x1] = 1
  else:
    mask[...] = 1
  return ndimage.distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1].astype(np.float32)


@pytest.mark.parametrize('shape', [(7, 9), (16, 5), (3, 3)])
@pytest.mark.parametrize('margin', [0, 1, 2, 3])
def test_blend_weights_equal_the_distance_transform(shape, margin):
  grid = (3, 2)
  for ty in range(grid[0]):
    for tx in range(grid[1]):
      got = processor_warp.blend_weights((4,) + shape, tx, ty, grid, margin)
      want = _edt_weights(shape, tx, ty, grid, margin)
      assert got.dtype == np.float32 and got.shape == shape
      np.testing.assert_array_equal(got, want, err_msg=f'{shape} {margin} {(tx, ty)}')


def test_blend_weights_keep_the_outer_edge_quirk():
  """margin > 0: a side on the outer edge of the grid ends at -1, so the last
  column / row has weight 0; margin == 0 cuts nothing."""
  w = processor_warp.blend_weights((2, 6, 8), 1, 1, (2, 2), 2)
  assert np.all(w[-1] == 0) and np.all(w[:, -1] == 0) and w[2, 2] == 1 and w[1, 2] == 0
  w = processor_warp.blend_weights((2, 6, 8), 1, 1, (2, 2), 0)
  assert np.all(w[-1] == 1) and np.all(w[:, -1] == 1) and w.max() == 3


def test_blend_weights_match_the_golden_ones(scenes):
  for sc in scenes:
    shape = sc['tiles'][0].shape
    for i, (tx, ty) in sc['tile_idx_to_xy'].items():
      got = processor_warp.blend_weights(shape, tx, ty, (2, 2), sc['margin'])
      np.testing.assert_array_equal(got, sc['weights'][i])


def test_tile_boxes_match_the_reference(scenes, numpy_outer_box):
  for sc in scenes:
    got = processor_warp.tile_boxes(sc['meshes'], sc['tile_idx_to_xy'], sc['tiles'][0].shape,
                                    sc['stride'], sc['offset'])
    assert sorted(got) == sorted(sc['boxes'])
    for i, (out_box, tg_box) in sc['boxes'].items():
      for a, b in zip(got[i], (out_box, tg_box)):
        np.testing.assert_array_equal(a.start, b.start)
        np.testing.assert_array_equal(a.size, b.size)


def test_plan_render_matches_the_reference(scenes, numpy_outer_box):
  seen = set()
  for sc in scenes:
    for name, box, plan, _ in sc['requests']:
      got = processor_warp.plan_render(box, sc['boxes'], sc['inverted'], sc['tile_idx_to_xy'],
                                       sc['tiles'][0].shape, sc['stride'], sc['offset'])
      assert render3d_ref.same_plan(got, plan), (sc['name'], name)
      seen.add((name, len(plan)))
  # the requests are what their names say
  assert ('canvas', 4) in seen and ('inside', 1) in seen and ('nothing', 0) in seen
  assert ('corner', 4) in seen and ('voxel', 4) in seen


def test_plan_render_takes_pairs_and_skips_unknown_tiles(scenes, numpy_outer_box):
  sc = scenes[1]
  name, box, plan, _ = sc['requests'][1]
  boxes = {i: tuple((b.start, b.size) for b in pair) for i, pair in sc['boxes'].items()}
  inverted = {i: ((b.start, b.size), m) for i, (b, m) in sc['inverted'].items() if i != 2}
  got = processor_warp.plan_render((box.start, box.size), boxes, inverted,
                                   sc['tile_idx_to_xy'], sc['tiles'][0].shape, sc['stride'],
                                   sc['offset'])
  assert render3d_ref.same_plan(got, [item for item in plan if item[0] != 2])


def test_restated_render_loop_equals_the_reference(scenes):
  """tests/render3d_ref.render == the volumes StitchAndRender3dTiles.process
  returned, every scene and request, bit for bit."""
  for sc in scenes:
    for name, box, plan, want in sc['requests']:
      got = render3d_ref.render(box, sc['tiles'], plan, sc['inverted'], sc['weights'],
                                sc['stride'], sc['order'], sc['dtype'])
      assert got.dtype == want.dtype
      np.testing.assert_array_equal(got, want, err_msg=f"{sc['name']} {name}")


def test_golden_canvas_is_not_trivial(scenes):
  for sc in scenes:
    name, box, plan, out = sc['requests'][0]
    assert name == 'canvas' and len(plan) == 4
    assert np.mean(out != 0) > 0.5
    assert np.all(sc['requests'][4][3] == 0)     # no tile reaches it
    assert sc['requests'][1][1].size[0] == 67
