"""Device time of the fused 3-D tile render against the same volume assembled from
the ops the package had before it.

One output box of 512 x 512 x 128 voxels over a 2 x 2 grid of uint8 tiles of
[128, 288, 288] voxels (32 voxels of overlap, mesh stride (8, 16, 16), a smooth
deformation of a few voxels), tiles, inverted maps and weights resident on the
device.  The forms alternate in one process, torch events around every call, 3
warm-up calls and `--reps` timed calls each, taken in rounds of 5:

  A        processor_warp.TileRenderer.render(box): the per-request planning
           (one outer_box reduction per tile, read by the host), the upload of
           the tile table and ONE sfm_render_tiles3d launch; the volume stays on
           the device
  A_kernel the same with the plan given: table upload and launch only
  B        per tile two warp.ndimage_warp calls (image region, blending weights
           repeated along z), each uploading its inputs and bringing its result
           to the host as that function does, and the float32 blend, the
           normalisation and the cast in NumPy, in ascending tile index

B is checked equal to A, voxel for voxel, before anything is timed.  Written to
profiles/render3d_time.txt as one JSON line: the medians, the spread (max - min)
of the per-round medians, and the kernel's work per (voxel, tile) pair against
the chip's rates: bytes requested from the memory system (24 map taps of 8 B, 8
image taps, 8 weight taps of 4 B -- nearly all served by the caches; what HBM has
to deliver is the tiles once and the output once) and FP64 operations (counted
from the kernel's statements, a division as one; nothing contracts to FMA).

  python tools/measure/render3d_time.py [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sofima_amd import processor_warp, warp  # noqa: E402

TILE = (128, 288, 288)
STRIDE = (8, 16, 16)
OVERLAP = 32
BOX = ((16, 16, 0), (512, 512, 128))
HBM_TB_S = 6.3          # achievable (MI355X_MICROARCH.md, 'HBM')
FP64_TOP_S = 78.6 / 2   # vector FP64, AMD's published 78.6 TFLOP/s counts an FMA as two
REQUEST_BYTES = 24 * 8 + 8 * 1 + 8 * 4
FP64_OPS = 6 + 12 + 3 * 8 * 5 + 2 * (12 + 8 * 5)


def box(start, size):
  return types.SimpleNamespace(start=np.array(start, np.int64), size=np.array(size, np.int64))


def montage():
  """Tiles, solved meshes (a coarse shift of -OVERLAP per grid step and a smooth
  deformation) and inverse maps over the tiles' target boxes widened by one node,
  as a caller holds them; the inverse maps undo the coarse shift and carry a smooth
  deformation of their own (an exact inverse is not needed to time the render)."""
  rng = np.random.default_rng(0)
  nodes = tuple(n // s + 1 for n, s in zip(TILE, STRIDE))
  z, y, x = np.mgrid[:nodes[0], :nodes[1], :nodes[2]].astype(np.float64)
  meshes = np.zeros((3, 4) + nodes, np.float32)
  tiles, xy = {}, {}
  for i in range(4):
    gx, gy = i % 2, i // 2
    xy[i] = (gx, gy)
    tiles[i] = rng.integers(0, 256, TILE).astype(np.uint8)
    meshes[0, i] = -OVERLAP * gx + 2.5 * np.sin(y / 3.0 + i) + np.cos(z / 2.0)
    meshes[1, i] = -OVERLAP * gy + 2.0 * np.cos(x / 4.0 + i) - np.sin(z / 3.0)
    meshes[2, i] = 1.2 * np.sin(x / 5.0 + y / 4.0 + i)
  inverted = {}
  for i, (_, tg_box) in processor_warp.tile_boxes(meshes, xy, TILE, STRIDE).items():
    gx, gy = xy[i]
    n = tg_box.size + 2
    z, y, x = np.mgrid[:n[2], :n[1], :n[0]].astype(np.float64)
    inv = np.stack([OVERLAP * gx - 2.5 * np.sin(y / 3.0 + i) - np.cos(z / 2.0),
                    OVERLAP * gy - 2.0 * np.cos(x / 4.0 + i) + np.sin(z / 3.0),
                    -1.2 * np.sin(x / 5.0 + y / 4.0 + i)])
    inverted[i] = (box(tg_box.start - 1, n), inv)
  return tiles, meshes, inverted, xy


def timed(fns, reps, rounds_of=5):
  for _ in range(3):
    for fn in fns:
      fn()
  torch.cuda.synchronize()
  times = [[] for _ in fns]
  for _ in range(reps):
    for i, fn in enumerate(fns):
      t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      t0.record()
      fn()
      t1.record()
      t1.synchronize()
      times[i].append(t0.elapsed_time(t1))
  out = []
  for t in times:
    rounds = [float(np.median(t[k:k + rounds_of])) for k in range(0, len(t), rounds_of)]
    out.append((float(np.median(t)), max(rounds) - min(rounds)))
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=20)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render3d_time.txt'))
  args = ap.parse_args()
  tiles, meshes, inverted, xy = montage()
  r = processor_warp.TileRenderer(tiles, meshes, xy, inverted, STRIDE)
  b = box(*BOX)
  plan = r.plan(b)
  assert [item[0] for item in plan] == [0, 1, 2, 3]
  weights = {i: w.cpu().numpy() for i, w in r.weights.items()}

  def form_a():
    return r.render(b, device_output=True)

  def form_a_kernel():
    return r.render(b, device_output=True, plan=plan)

  def form_b():
    shape = tuple(int(v) for v in b.size[::-1])
    img = np.zeros(shape, np.float32)
    norm = np.zeros(shape, np.float32)
    for i, data_box, tg_box, lw_box, sub_box in plan:
      sl = tuple(slice(int(a), int(a + n)) for a, n in zip(data_box.start[::-1],
                                                          data_box.size[::-1]))
      kw = dict(image_box=data_box, map_box=tg_box, out_box=lw_box)
      image = warp.ndimage_warp(tiles[i][sl], inverted[i][1], STRIDE, (128,) * 3, (0,) * 3, **kw)
      dts = np.repeat(weights[i][sl[1:]][None], int(data_box.size[2]), axis=0)
      dts = warp.ndimage_warp(dts, inverted[i][1], STRIDE, (128,) * 3, (0,) * 3, **kw)
      o = tuple(slice(int(a), int(a + n)) for a, n in zip((sub_box.start - b.start)[::-1],
                                                          sub_box.size[::-1]))
      img[o] += image * dts
      norm[o] += dts
    img[norm > 0] /= norm[norm > 0]
    return img.astype(np.uint8)

  got_a = np.asarray(form_a())
  got_b = form_b()
  assert np.array_equal(got_a, got_b), 'forms differ'
  assert np.mean(got_a != 0) > 0.9

  (a, a_sp), (ak, ak_sp), (bt, b_sp) = timed([form_a, form_a_kernel, form_b], args.reps)
  voxels = int(np.prod(b.size))
  pairs = int(sum(np.prod(item[4].size) for item in plan))
  rec = {
      'box': [int(v) for v in b.size], 'tiles': 4, 'tile_shape': list(TILE), 'dtype': 'uint8',
      'reps': args.reps, 'A_fused_ms': round(a, 3), 'A_round_spread_ms': round(a_sp, 3),
      'A_kernel_ms': round(ak, 3), 'A_kernel_round_spread_ms': round(ak_sp, 3),
      'B_sequence_ms': round(bt, 3), 'B_round_spread_ms': round(b_sp, 3),
      'B_over_A': round(bt / a, 1), 'voxel_tile_pairs': pairs,
      'pairs_per_voxel': round(pairs / voxels, 3),
      'request_bytes_per_pair': REQUEST_BYTES, 'fp64_ops_per_pair': FP64_OPS,
      'hbm_bytes': voxels + 4 * int(np.prod(TILE)),
      'hbm_floor_ms': round((voxels + 4 * int(np.prod(TILE))) / (HBM_TB_S * 1e9), 4),
      'fp64_floor_ms': round(pairs * FP64_OPS / (FP64_TOP_S * 1e9), 3),
      'kernel_fp64_Top_s': round(pairs * FP64_OPS / ak / 1e9, 2),
      'kernel_request_TB_s': round(pairs * REQUEST_BYTES / ak / 1e9, 2)}
  line = json.dumps(rec)
  print(line, flush=True)
  with open(args.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
