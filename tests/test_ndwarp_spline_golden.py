"""tests/ndwarp_spline_ref.py against tests/golden/ndimage_warp_spline.npz, what the
UNMODIFIED reference returned with spline orders 2 to 5: `warp.ndimage_warp` and
the render loop of StitchAndRender3dTiles, element for element."""
import numpy as np
import pytest

from tests import ndwarp_spline_ref as ref
from tests import render3d_ref


@pytest.fixture(scope='module')
def fixture(golden):
  return golden('ndimage_warp_spline')


def test_fixture_covers_what_it_should(fixture):
  cases = ref.warp_cases(fixture)
  seen = {(c['image'].dtype.name, c['image'].ndim, c['order']) for c in cases}
  for dtype in ('uint8', 'uint16', 'float32'):
    for dim in (2, 3):
      assert (dtype, dim, 3) in seen
  for order in (2, 4, 5):
    for dim in (2, 3):
      assert any(s[1] == dim and s[2] == order for s in seen)
  assert any(c['boxes'] is not None for c in cases)
  assert any(any(w < s for w, s in zip(c['work'], c['warped'].shape[::-1])) and any(c['overlap'])
             for c in cases)


def test_ndimage_warp_cases(fixture):
  for c in ref.warp_cases(fixture):
    kw = {}
    if c['boxes'] is not None:
      kw = dict(image_start=c['boxes']['image'][0], map_start=c['boxes']['map'][0],
                out_start=c['boxes']['out'][0], out_size=c['boxes']['out'][1])
    got = ref.ndimage_warp(c['image'], c['map'], c['stride'], c['order'], **kw)
    assert got.dtype == c['warped'].dtype and got.shape == c['warped'].shape, c['name']
    assert np.array_equal(got, c['warped']), c['name']


def test_render_scenes(fixture, golden):
  scenes = render3d_ref.scenes(golden('render3d'))
  cases = ref.render_cases(fixture, scenes)
  assert sorted(order for _, order, _ in cases) == [2, 3, 3, 3]
  for sc, order, reqs in cases:
    assert len(reqs) >= 5
    for name, b, plan, want in reqs:
      got = ref.render(b, sc['tiles'], plan, sc['inverted'], sc['weights'], sc['stride'], order)
      assert got.dtype == want.dtype and np.array_equal(got, want), (sc['name'], order, name)


def test_guards_are_the_old_fixtures(fixture, golden):
  assert np.array_equal(fixture['guard_ndwarp_o1'], golden('ndimage_warp')['u8_3d_warped'])
  assert np.array_equal(fixture['guard_render_o1'], golden('render3d')['s00_r01_out'])
  assert not np.array_equal(fixture['guard_ndwarp_o0'], fixture['guard_ndwarp_o1'])
  assert not np.array_equal(fixture['guard_render_o0'], fixture['guard_render_o1'])
