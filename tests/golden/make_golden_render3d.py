"""Generates tests/golden/render3d.npz from the UNMODIFIED reference
`processor/warp.py: StitchAndRender3dTiles` (NumPy / SciPy / Qhull): the class
runs as it is, `process` included, with the reference's own `map_utils.invert_map`
and `fill_missing(extrapolate=True, interpolate_first=False)` and its own
`warp.ndimage_warp`.

Build-container only.  `_refshim` makes `import sofima` and the connectomics box
types resolve; what the processor needs beyond that is declared HERE, restated
from the documented behaviour of the packages that are not in this container:

  edt.edt(mask, black_border=True, parallel=0)
      the Euclidean distance transform with everything outside the array taken
      as background: scipy.ndimage.distance_transform_edt of the mask padded by
      one background pixel, cropped back, as float32
  connectomics.common.file.Path(path).open(mode)            -> open(path, mode)
  BoundingBox.scale(s)            floor of start * s, ceil of end * s
  BoundingBox.to_slice_tuple(a, b)   slices of dims [a, b) in reverse (.. y x) order
  SubvolumeProcessor.output_type(dtype) -> dtype;  crop_box_and_data(box, data)
      -> Subvolume(data, box) (crop_at_borders is False in this processor)
  Subvolume(data, bbox), OutputNums
  futures.ThreadPoolExecutor / as_completed of processor/warp.py only: jobs run
      at submission and come back in submission order, so the float32 sums are
      taken in ascending tile index (the reference's order is unspecified)

Stored -- data only:
  tiles_uint8     [4, 10, 36, 44]         the four tiles; the uint16 and float32
                                          ones follow from them (`tiles_of`)
  meshes          [3, 4, 4, 6, 7]         solved tile meshes (relative format)
  key_xy          [4, 2]                  (tx, ty) of tile index i
  sNN_*  per scene: dtype, order, margin, offset (xyz), stride (zyx), boxes
         ([4, 4, 3]: out_box start, size, tg_box start, size), w_i (blend weights)
  inv_i, inv_box_i   inverted map of tile i and its box (start, size), the same in
         every scene
  sNN_rMM_*  per request: box (start, size), plan ([n, 9, 3]: tile index
         (repeated), data_box, tg_box, local_warp_box, sub_box as start, size
         rows), out (the rendered volume)
Run:
  python tests/golden/make_golden_render3d.py
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()


# -- stand-ins (see the module docstring) ----------------------------------------
def _edt(mask, black_border=False, parallel=1):
  del parallel
  assert black_border
  return ndimage.distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1].astype(np.float32)


sys.modules['edt'] = types.ModuleType('edt')
sys.modules['edt'].edt = _edt


class _Path:

  def __init__(self, path):
    self._path = path

  def open(self, mode='r'):
    return open(self._path, mode)


sys.modules['connectomics.common.file'].Path = _Path


def _scale(self, scale_factor):
  s = np.asarray(scale_factor)
  return refshim.BoundingBox(start=np.floor(self.start * s).astype(np.int64),
                             end=np.ceil(self.end * s).astype(np.int64))


def _to_slice_tuple(self, start_dim, end_dim):
  return tuple(slice(int(self.start[d]), int(self.end[d]))
               for d in range(end_dim - 1, start_dim - 1, -1))


refshim.BoundingBox.scale = _scale
refshim.BoundingBox.to_slice_tuple = _to_slice_tuple


class Subvolume:

  def __init__(self, data, bbox):
    self.data = data
    self.bbox = bbox


_sp = sys.modules['connectomics.volume.subvolume_processor']
_sp.OutputNums = type('OutputNums', (), {'SINGLE': 1, 'MULTI': 2})
_sp.SubvolumeOrMany = Subvolume
_sp.SubvolumeProcessor.output_type = lambda self, dtype: dtype
_sp.SubvolumeProcessor.crop_box_and_data = lambda self, box, data: Subvolume(data, box)
sys.modules['connectomics.volume.subvolume'].Subvolume = Subvolume
sys.modules['connectomics.volume.subvolume'].SubvolumeOrMany = Subvolume

from concurrent import futures as _futures  # noqa: E402

from sofima.processor import warp as pwarp  # noqa: E402


class _InlineExecutor:
  """Runs a job when it is submitted; numbers the futures."""

  def __init__(self, max_workers=None):
    self._n = 0

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    return False

  def submit(self, fn, *args, **kwargs):
    f = _futures.Future()
    f.set_result(fn(*args, **kwargs))
    f.order = self._n
    self._n += 1
    return f


pwarp.futures = types.SimpleNamespace(
    ThreadPoolExecutor=_InlineExecutor, Executor=_futures.Executor, Future=_futures.Future,
    as_completed=lambda fs: iter(sorted(fs, key=lambda f: f.order)))


class Renderer(pwarp.StitchAndRender3dTiles):
  tiles = None

  def _open_tile_volume(self, tile_id):
    return Renderer.tiles[tile_id]


def reset_caches():
  pwarp.StitchAndRender3dTiles._tile_meshes = None
  pwarp.StitchAndRender3dTiles._tile_idx_to_xy = None
  pwarp.StitchAndRender3dTiles._tile_boxes = {}
  pwarp.StitchAndRender3dTiles._inverted_meshes = {}


# -- inputs ----------------------------------------------------------------------
TILE = (10, 36, 44)       # zyx
STRIDE = (4, 8, 8)        # zyx
NODES = (4, 6, 7)         # zyx
GRID = (2, 2)             # yx
OVERLAP = 8
TILE_MAP = [[0, 1], [2, 3]]


def make_tiles(rng):
  """Four uint8 tiles: a smooth pattern that continues across the montage, a
  per-tile contrast change and a little noise."""
  base = np.zeros((4,) + TILE, np.uint8)
  z, y, x = np.mgrid[:TILE[0], :TILE[1], :TILE[2]]
  for i in range(4):
    tx, ty = i % 2, i // 2
    gx, gy = x + tx * (TILE[2] - OVERLAP), y + ty * (TILE[1] - OVERLAP)
    v = 120 + 70 * np.sin(gx / 5.0 + z / 3.0) * np.cos(gy / 7.0) + 25 * np.sin((gx + gy) / 3.0)
    v = v * (0.9 + 0.05 * i) + rng.integers(-2, 3, TILE)
    base[i] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
  base[0, 0, 0, :5] = (0, 255, 1, 254, 128)
  return base


def tiles_of(base, dtype):
  """The tiles of a dtype from the stored uint8 ones (tests/render3d_ref.py restates
  this): uint16 above the 8-bit range with both ends of the range planted, float32
  with negative values and quarter steps."""
  if dtype == 'uint8':
    return base
  if dtype == 'uint16':
    t = base.astype(np.uint16) * np.uint16(3) + np.uint16(1000)
    t[1, 0, 0, :4] = (0, 65535, 1, 65534)
    return t
  assert dtype == 'float32'
  return base.astype(np.float32) * np.float32(0.25) - np.float32(7.5)


def make_meshes(rng):
  """[3, 4, z, y, x] float32: coarse shift of -OVERLAP per grid step, a smooth
  deformation of a few voxels and a little node noise."""
  m = np.zeros((3, 4) + NODES, np.float32)
  z, y, x = np.mgrid[:NODES[0], :NODES[1], :NODES[2]].astype(np.float64)
  for i in range(4):
    tx, ty = i % 2, i // 2
    ph = 0.7 * i
    m[0, i] = -OVERLAP * tx + 2.5 * np.sin(y / 2.0 + ph) + 0.8 * np.cos(z + ph)
    m[1, i] = -OVERLAP * ty + 2.0 * np.cos(x / 2.5 + ph) - 0.7 * np.sin(z / 1.5)
    m[2, i] = 1.2 * np.sin(x / 3.0 + y / 2.0 + ph)
  m += rng.uniform(-0.3, 0.3, m.shape).astype(np.float32)
  return m


SCENES = [
    dict(dtype='uint8', order=1, margin=0, offset=(0, 0, 0)),
    dict(dtype='uint8', order=0, margin=3, offset=(5, -3, 2)),
    dict(dtype='uint16', order=1, margin=3, offset=(-7, 11, -1)),
    dict(dtype='float32', order=1, margin=0, offset=(5, -3, 2)),
]


def bb(start, size):
  return refshim.BoundingBox(start=np.array(start, np.int64), size=np.array(size, np.int64))


def requests(canvas, reach, boxes, offset):
  """The whole canvas; a box cutting through tiles, 67 wide; a box inside tile 0;
  a box around the four-tile corner; a box no tile reaches; one voxel."""
  c0 = canvas.start
  corner = np.array((TILE[2] - OVERLAP // 2 + offset[0], TILE[1] - OVERLAP // 2 + offset[1],
                     4 + offset[2]))
  inside = boxes[0][0].start + np.array((9, 7, 3))
  return [
      canvas,
      bb(c0 + (6, 23, 3), (67, 21, 4)),
      bb(inside, (13, 9, 4)),
      bb(corner - (6, 5, 2), (12, 10, 5)),
      bb(reach + (3, 2, 1), (9, 6, 3)),
      bb(corner + (1, -2, 0), (1, 1, 1)),
  ]


def rows(*boxes_):
  return np.array([v for b in boxes_ for v in (b.start, b.size)], np.int64)


def main():
  rng = np.random.default_rng(41)
  base = make_tiles(rng)
  meshes = make_meshes(rng)
  key_to_idx = {(i % 2, i // 2): i for i in range(4)}
  tmp_dir = tempfile.mkdtemp(prefix='render3d_')
  mesh_path = os.path.join(tmp_dir, 'meshes.npz')
  np.savez(mesh_path, x=meshes, key_to_idx=np.array(key_to_idx, dtype=object))

  arrays = dict(meshes=meshes, key_xy=np.array([(i % 2, i // 2) for i in range(4)], np.int64))
  arrays['tiles_uint8'] = base
  try:
    for s, scene in enumerate(SCENES):
      reset_caches()
      scene_tiles = tiles_of(base, scene['dtype'])
      Renderer.tiles = {i: scene_tiles[i] for i in range(4)}
      proc = Renderer(tile_map=TILE_MAP, tile_mesh_path=mesh_path, tile_pattern_path='',
                      stride=STRIDE, offset=scene['offset'], margin=scene['margin'],
                      work_size=(32, 32, 8), order=scene['order'], parallelism=1)
      dtype = np.dtype(scene['dtype'])

      def run(box):
        sub = Subvolume(np.zeros((1,) + tuple(box.size[::-1]), dtype), box)
        return proc.process(sub).data[0]

      # the tile boxes exist after the first call: a throw-away one-voxel request
      run(bb((0, 0, 0), (1, 1, 1)))
      boxes = dict(pwarp.StitchAndRender3dTiles._tile_boxes)
      # the canvas: the nominal extent of the montage and a rim of two voxels (one in
      # z); `reach` is the end of everything any tile could render
      off = np.array(scene['offset'])
      nominal = np.array((GRID[1] * TILE[2] - OVERLAP, GRID[0] * TILE[1] - OVERLAP, TILE[0]))
      canvas = bb(off - (2, 2, 1), nominal + (4, 4, 2))
      reach = np.max([b[0].end for b in boxes.values()], axis=0)
      p = f's{s:02d}_'
      arrays[p + 'dtype'] = np.array(scene['dtype'])
      arrays[p + 'order'] = np.array(scene['order'])
      arrays[p + 'margin'] = np.array(scene['margin'])
      arrays[p + 'offset'] = np.array(scene['offset'], np.int64)
      arrays[p + 'stride'] = np.array(STRIDE, np.int64)
      arrays[p + 'boxes'] = np.array([rows(*boxes[i]).reshape(4, 3) for i in range(4)])

      for r, box in enumerate(requests(canvas, reach, boxes, scene['offset'])):
        out = run(box)
        # the plan: what _load_tile_images hands to the render loop
        contexts = []
        fs = proc._load_tile_images(box, Renderer.tiles[0].shape, Renderer.tiles,
                                    _InlineExecutor())
        inv_idx = {id(v[1]): i for i, v in pwarp.StitchAndRender3dTiles._inverted_meshes.items()}
        for f in sorted(fs, key=lambda f: f.order):
          _, (inv, tg_box, lw_box, sub_box, _, data_box) = f.result()
          i = inv_idx[id(inv)]
          contexts.append(np.concatenate(
              [np.full((1, 3), i, np.int64), rows(data_box, tg_box, lw_box, sub_box)]))
        q = f'{p}r{r:02d}_'
        arrays[q + 'box'] = rows(box)
        arrays[q + 'plan'] = np.array(contexts, np.int64).reshape(-1, 9, 3)
        arrays[q + 'out'] = out
        assert out.dtype == dtype and out.shape == tuple(box.size[::-1])

      inverted = pwarp.StitchAndRender3dTiles._inverted_meshes
      assert sorted(inverted) == [0, 1, 2, 3]
      for i in range(4):
        tg_box, inv = inverted[i]
        assert inv.dtype == np.float64 and not np.isnan(inv).any()
        # (the inverted maps depend on the meshes and the stride alone: stored once)
        if s == 0:
          arrays[f'inv_{i}'] = inv
          arrays[f'inv_box_{i}'] = rows(tg_box)
        assert np.array_equal(arrays[f'inv_{i}'], inv)
        assert np.array_equal(arrays[f'inv_box_{i}'], rows(tg_box))
        tx, ty = i % 2, i // 2
        arrays[f'{p}w_{i}'] = proc._get_dts(Renderer.tiles[0].shape, tx, ty)

      # norm > 0 / two tiles / four tiles on the whole canvas, from the reference's
      # own weights: the warped weights of every tile, summed
      box = canvas
      norm = np.zeros(tuple(box.size[::-1]), np.float32)
      count = np.zeros(norm.shape, np.int64)
      for c in arrays[p + 'r00_plan']:
        i = int(c[0, 0])
        data_box, tg_box, lw_box, sub_box = (bb(c[k], c[k + 1]) for k in (1, 3, 5, 7))
        w = arrays[f'{p}w_{i}'][data_box.to_slice_tuple(0, 2)][None]
        w = np.repeat(w, data_box.size[2], axis=0)
        ww = pwarp.warp.ndimage_warp(w, inverted[i][1], STRIDE, work_size=(32, 32, 8),
                                     overlap=(0, 0, 0), image_box=data_box, map_box=tg_box,
                                     out_box=lw_box)
        sl = sub_box.translate(-box.start).to_slice3d()
        norm[sl] += ww
        count[sl] += ww > 0
      frac1, frac2, n4 = np.mean(norm > 0), np.mean(count >= 2), int(np.sum(count >= 4))
      print(f'scene {s}: norm > 0 {frac1:.3f}, two or more tiles {frac2:.3f}, four tiles {n4}')
      assert frac1 >= 0.5, frac1
      assert frac2 >= 0.05, frac2
      assert n4 >= 1, n4
  finally:
    shutil.rmtree(tmp_dir)
    reset_caches()

  path = os.path.join(HERE, 'render3d.npz')
  np.savez_compressed(path, **arrays)
  print('wrote', path, os.path.getsize(path), 'bytes')
  assert os.path.getsize(path) < 500 * 1024


if __name__ == '__main__':
  main()
