"""Generates tests/golden/ndimage_warp_spline.npz: the UNMODIFIED reference with
spline orders 2 to 5 (`scipy.ndimage.map_coordinates` with its B-spline
prefilter), through `_refshim`.

  * `warp.ndimage_warp` (warp.py:189-335): order 3 on uint8 / uint16 / float32 in
    2-D and 3-D; orders 2, 4 and 5 in 2-D and 3-D; work boxes smaller than the
    output, with overlap; map / image / output boxes.
  * `processor/warp.py: StitchAndRender3dTiles.process` with `order=3` (and one
    scene with `order=2`), run by the machinery of make_golden_render3d.py, which
    is imported, not edited.  The scenes are scenes of render3d.npz with only the
    order changed, so tiles, meshes, inverted maps, weights, boxes and plans (none
    of which depends on the order) are the ones stored there, the request boxes
    and the order-1 volumes are asserted to be, and only the rendered volumes are
    new.
  * guards of the old paths: orders 0 and 1 of `ndimage_warp` on case `u8_3d` of
    ndimage_warp.npz and of the render on scene geometry s00, as the reference
    computes them (which is what the order-0 / order-1 kernels reproduce).

Every spline case is asserted to differ from its order-1 output.  The archive is
written with fixed time stamps: running the script again gives the same bytes.

Stored -- data only:
  img2 [40, 52], img3 [9, 30, 36] uint8     base images (`image_of` derives the
                                            uint16 and float32 ones)
  map2 [2, 5, 6], map3 [3, 4, 6, 7] float32 coordinate maps
  names                                     the ndimage_warp cases
  NAME_{dtype,order,stride,work,overlap,warped}, NAME_{image,map,out}_box
  rNN_{base,order}   render scene: index of the scene of render3d.npz, order
  rNN_qMM_out        rendered volume of request MM (REQUESTS of render3d_ref.py)
  guard_ndwarp_o{0,1}, guard_render_o{0,1}
Run:
  python tests/golden/make_golden_ndwarp_spline.py
"""
import io
import os
import shutil
import tempfile
import zipfile

import numpy as np
from scipy import ndimage

import make_golden_render3d as g   # installs the shim and the processor stand-ins

from sofima import warp as rwarp  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
refshim = g.refshim


def save_npz(path, arrays):
  """np.savez_compressed with fixed time stamps (byte-identical on every run)."""
  with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
    for name, arr in arrays.items():
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
      info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      zf.writestr(info, buf.getvalue())


def image_of(base, dtype):
  """The image of a dtype from a stored uint8 one (tests restate this)."""
  dtype = np.dtype(dtype)
  if dtype == np.uint8:
    return base
  if dtype == np.uint16:
    return base.astype(np.uint16) * np.uint16(257)
  assert dtype == np.float32
  return base.astype(np.float32) / np.float32(3) - np.float32(20)


def textured(rng, shape, sigma):
  """Smooth structure plus pixel noise, full 8-bit range with both ends present:
  sharp enough for the spline orders to overshoot and to differ from linear."""
  img = ndimage.gaussian_filter(rng.standard_normal(shape), sigma)
  img = (img - img.min()) / (img.max() - img.min()) * 255
  img = np.clip(img + rng.integers(-40, 41, shape), 0, 255)
  return np.rint(img).astype(np.uint8)


def field(rng, shape, amp, sig):
  f = ndimage.gaussian_filter(rng.standard_normal(shape), (0,) + (sig,) * (len(shape) - 1))
  return (f / np.abs(f).max() * amp).astype(np.float32)


BOXES3 = dict(image=((100, 200, 10), (36, 30, 9)), map=((16, 33, 3), (7, 6, 4)),
              out=((103, 202, 11), (28, 24, 7)))

# name: base image, dtype, order, stride zyx, work xyz, overlap xyz, boxes
CASES = {
    'u8_2d_o3': ('img2', 'uint8', 3, (10, 10), (24, 16), (6, 4), None),
    'u16_2d_o3': ('img2', 'uint16', 3, (10, 10), (64, 64), (0, 0), None),
    'f32_2d_o3': ('img2', 'float32', 3, (10.0, 10.0), (20, 20), (5, 3), None),
    'u8_3d_o3': ('img3', 'uint8', 3, (3, 6, 6), (16, 12, 4), (4, 4, 2), None),
    'u16_3d_o3': ('img3', 'uint16', 3, (3, 6, 6), (64, 64, 16), (0, 0, 0), None),
    'f32_3d_o3': ('img3', 'float32', 3, (3, 6, 6), (20, 20, 6), (3, 5, 1), None),
    'u8_3d_boxes_o3': ('img3', 'uint8', 3, (3, 6, 6), (12, 10, 3), (4, 2, 1), BOXES3),
    'u8_2d_o2': ('img2', 'uint8', 2, (10, 10), (24, 16), (6, 4), None),
    'f32_2d_o4': ('img2', 'float32', 4, (10, 10), (30, 30), (8, 8), None),
    'u16_2d_o5': ('img2', 'uint16', 5, (10, 10), (24, 16), (6, 4), None),
    'u16_3d_o2': ('img3', 'uint16', 2, (3, 6, 6), (16, 12, 4), (4, 4, 2), None),
    'u8_3d_o4': ('img3', 'uint8', 4, (3, 6, 6), (20, 20, 6), (3, 5, 1), None),
    'f32_3d_boxes_o5': ('img3', 'float32', 5, (3, 6, 6), (12, 10, 3), (4, 2, 1), BOXES3),
}


def gen_ndimage_warp(out):
  rng = np.random.default_rng(2025)
  out['img2'] = textured(rng, (40, 52), 1.5)
  out['img3'] = textured(rng, (9, 30, 36), 1.2)
  out['map2'] = field(rng, (2, 5, 6), 4.0, 1.0)
  out['map3'] = field(rng, (3, 4, 6, 7), 2.0, 1.0)
  assert out['img2'].min() == 0 and out['img2'].max() == 255
  out['names'] = np.array(list(CASES))
  for name, (base, dtype, order, stride, work, ov, boxes) in CASES.items():
    img = image_of(out[base], dtype)
    cmap = out['map2' if img.ndim == 2 else 'map3']
    kw = {}
    if boxes is not None:
      for k in ('image', 'map', 'out'):
        kw[k + '_box'] = refshim.BoundingBox(start=boxes[k][0], size=boxes[k][1])
        out[f'{name}_{k}_box'] = np.array(boxes[k], np.int64)
    got = rwarp.ndimage_warp(img, cmap, stride, work, ov, order=order, parallelism=2, **kw)
    linear = rwarp.ndimage_warp(img, cmap, stride, work, ov, order=1, parallelism=2, **kw)
    # one work box instead of many: the reference prefilters the whole image per box
    shape_xyz = got.shape[::-1]
    whole = rwarp.ndimage_warp(img, cmap, stride, shape_xyz, (0,) * img.ndim, order=order, **kw)
    assert np.array_equal(got, whole), name
    differ = np.mean(got != linear)
    print(f'ndimage_warp {name}: {got.shape} {got.dtype}, non-zero {(got != 0).mean():.3f}, '
          f'differs from order 1 in {differ:.3f}')
    assert got.dtype == img.dtype and (got != 0).mean() > 0.5, name
    assert differ > 0.25, name
    out[f'{name}_base'] = np.array(base)
    out[f'{name}_dtype'] = np.array(dtype)
    out[f'{name}_order'] = np.int64(order)
    out[f'{name}_stride'] = np.array(stride, np.float64)
    out[f'{name}_stride_is_int'] = np.bool_(all(isinstance(v, int) for v in stride))
    out[f'{name}_work'] = np.array(work, np.int64)
    out[f'{name}_overlap'] = np.array(ov, np.int64)
    out[f'{name}_warped'] = got
  # guard: orders 0 and 1 on an existing fixture case
  old = np.load(os.path.join(HERE, 'ndimage_warp.npz'))
  args = (old['u8_3d_image'], old['u8_3d_map'], tuple(int(v) for v in old['u8_3d_stride']),
          tuple(old['u8_3d_work']), tuple(old['u8_3d_overlap']))
  for order in (0, 1):
    out[f'guard_ndwarp_o{order}'] = rwarp.ndimage_warp(*args, order=order)
  assert np.array_equal(out['guard_ndwarp_o1'], old['u8_3d_warped'])


# (scene of render3d.npz whose geometry is used, order, requests stored)
RENDER_SCENES = [(0, 3, (0, 1, 2, 3, 4, 5)), (2, 3, (1, 2, 3, 4, 5)), (3, 3, (1, 2, 3, 4, 5)),
                 (1, 2, (1, 2, 3, 4, 5))]


def gen_render(out):
  old = np.load(os.path.join(HERE, 'render3d.npz'))
  base, meshes = old['tiles_uint8'], old['meshes']
  key_to_idx = {(i % 2, i // 2): i for i in range(4)}
  tmp_dir = tempfile.mkdtemp(prefix='render3d_')
  mesh_path = os.path.join(tmp_dir, 'meshes.npz')
  np.savez(mesh_path, x=meshes, key_to_idx=np.array(key_to_idx, dtype=object))

  def renders(scene, order, which):
    """[(request index, rendered volume)] of the scene's geometry with `order`;
    boxes and plans are asserted to be the stored ones."""
    g.reset_caches()
    tiles = g.tiles_of(base, scene['dtype'])
    g.Renderer.tiles = {i: tiles[i] for i in range(4)}
    proc = g.Renderer(tile_map=g.TILE_MAP, tile_mesh_path=mesh_path, tile_pattern_path='',
                      stride=g.STRIDE, offset=scene['offset'], margin=scene['margin'],
                      work_size=(32, 32, 8), order=order, parallelism=1)
    dtype = np.dtype(scene['dtype'])

    def run(box):
      sub = g.Subvolume(np.zeros((1,) + tuple(box.size[::-1]), dtype), box)
      return proc.process(sub).data[0]

    run(g.bb((0, 0, 0), (1, 1, 1)))
    boxes = dict(g.pwarp.StitchAndRender3dTiles._tile_boxes)
    off = np.array(scene['offset'])
    nominal = np.array((g.GRID[1] * g.TILE[2] - g.OVERLAP, g.GRID[0] * g.TILE[1] - g.OVERLAP,
                        g.TILE[0]))
    canvas = g.bb(off - (2, 2, 1), nominal + (4, 4, 2))
    reach = np.max([b[0].end for b in boxes.values()], axis=0)
    reqs = g.requests(canvas, reach, boxes, scene['offset'])
    return [(r, reqs[r], run(reqs[r])) for r in which]

  try:
    for n, (s, order, which) in enumerate(RENDER_SCENES):
      scene = g.SCENES[s]
      p = f's{s:02d}_'
      assert str(old[p + 'dtype']) == scene['dtype']
      linear = {r: v for r, _, v in renders(scene, 1, which)}
      out[f'r{n:02d}_base'] = np.int64(s)
      out[f'r{n:02d}_order'] = np.int64(order)
      for r, box, vol in renders(scene, order, which):
        assert np.array_equal(g.rows(box), old[f'{p}r{r:02d}_box'])
        if scene['order'] == 1:
          assert np.array_equal(linear[r], old[f'{p}r{r:02d}_out'])
        differ = np.mean(vol != linear[r]) if vol.size else 0.0
        print(f'render scene {s} order {order} request {r}: {vol.shape} {vol.dtype}, '
              f'differs from order 1 in {differ:.3f}')
        if linear[r].any() and vol.size > 100:
          assert differ > 0.25, (s, r)
        out[f'r{n:02d}_q{r:02d}_out'] = vol
      assert any(out[f'r{n:02d}_q{r:02d}_out'].any() for r in which)
    # guard: orders 0 and 1 on the geometry of scene 0, the cutting request
    for order in (0, 1):
      (_, _, vol), = renders(g.SCENES[0], order, (1,))
      out[f'guard_render_o{order}'] = vol
    assert np.array_equal(out['guard_render_o1'], old['s00_r01_out'])
  finally:
    shutil.rmtree(tmp_dir)
    g.reset_caches()


def main():
  out = {}
  gen_ndimage_warp(out)
  gen_render(out)
  path = os.path.join(HERE, 'ndimage_warp_spline.npz')
  save_npz(path, out)
  print('wrote', path, os.path.getsize(path), 'bytes')
  assert os.path.getsize(path) < 400 * 1024


if __name__ == '__main__':
  main()
