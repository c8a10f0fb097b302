"""Processors for coordinate maps on MI355X, at array level.

`reconcile_cross_block_maps` is the compute of the reference's
`ReconcileCrossBlockMaps` (processor/maps.py:35-326: `_interpolate` and
`process`) without the volume framework around it: the step between a
block-wise mesh solve (`processor_mesh.relax_sections` with `block_starts`) and
the render.  It stitches the blocks into one continuous geometry: the first
section of every block takes its position from the cross-block map, and the
sections inside a block are composed with an offset field that grows with the
position in the block.  Every composition is `map_utils.compose_maps` on the
device, so the map stays resident from the solve to `invert_map` and the warp.
"""
from __future__ import annotations

import bisect
import types

import numpy as np
import torch

from . import _dev
from . import map_utils
from ._dev import DeviceArray


def _get_z_range(sorted_z, z: int):
  """The first and last + 1 sections of the block for `z` (the reference's
  `_get_z_range`); `sorted_z` are the sorted keys of `z_map`."""
  idx = bisect.bisect_left(sorted_z, z)
  if idx == 0:
    return 0, sorted_z[idx]
  return sorted_z[idx - 1], sorted_z[idx]


def block_ranges(sorted_z, z_start: int, z_end: int):
  """The (first, last + 1) section pairs of the blocks that sections
  [z_start, z_end) touch, in the order the reference's `process` visits them."""
  ranges = []
  z = z_start
  while z < z_end:
    s, e = _get_z_range(sorted_z, z)
    ranges.append((s, e))
    z = e + 1
  return ranges


def _section(load, z, dev):
  """A [2, 1, y, x] section of a volume as a contiguous device tensor of its
  own float32 / float64."""
  m = map_utils._engine_map(load(z), dev, keep_f32=True)
  if m.ndim != 4 or m.shape[0] != 2 or m.shape[1] != 1:
    raise ValueError(f'a volume section must be [2, 1, y, x], got {tuple(m.shape)}')
  return m


def reconcile_cross_block_maps(coord_map, box, *, cross_block, cross_block_inv, last_inv,
                               main_inv, z_map, stride, backward=False) -> DeviceArray:
  """Reconciles a block-wise solved coordinate map with a cross-block map.

  `coord_map` is the [2, z, y, x] relative map of `box` (`.start` / `.size` in
  xyz; NumPy, CUDA tensor or DeviceArray, float32 or float64, never modified).
  The four volumes of the reference's config are callables `z -> [2, 1, y, x]`
  over the box's xy extent, host or resident: `cross_block` and
  `cross_block_inv` are asked at the low-resolution z of `z_map`
  (`{section: cross-block section}`, the first sections of the blocks),
  `last_inv` and `main_inv` at high-resolution sections.  `stride` is the node
  distance, `backward` says that the mesh was solved from high z to low.

  Per block, as in the reference: `offset = compose(compose(xblock_pre_inv,
  block_end_inv), xblock_post)`; the first and last section of the block are
  copied from the cross-block map; every section inside the block becomes
  `compose(compose(section, xblock_pre), offset * scale)` with `scale = i /
  block_size` (`(block_size - i) / block_size` when backward), `offset *
  scale` formed in the offset's dtype.  All interior sections of a block go
  through two launches: the stack against the one slice `xblock_pre`, which is
  triangulated once, then against `offset` with a per-section scale.  A
  section is processed once (the shared section of two blocks belongs to the
  first that reaches it).  Afterwards the result is NaN where the input was.
  Nothing is cropped: the overlap belongs to the volume framework.

  Returns a DeviceArray of the input's shape and dtype.  The values carry the
  contract of `map_utils.compose_maps`; a refused triangulation raises
  SofimaAmdError (one status read per block).
  """
  shape = map_utils._map_shape(coord_map)
  if len(shape) != 4 or shape[0] != 2:
    raise ValueError(f'coord_map must be [2, z, y, x], got shape {shape}')
  start = [int(v) for v in np.asarray(box.start).ravel()]
  size = [int(v) for v in np.asarray(box.size).ravel()]
  if (shape[3], shape[2], shape[1]) != tuple(size[:3]):
    raise ValueError(f'box shape ({size}) mismatch with coord map ({shape})')
  z_map = {int(k): int(v) for k, v in z_map.items()}
  sorted_z = sorted(z_map)
  dev = _dev.device()
  data = map_utils._engine_map(coord_map, dev, keep_f32=True)
  ret = data.clone()
  flat = types.SimpleNamespace(start=tuple(start), size=(size[0], size[1], 1))
  z_lo, z_hi = start[2], start[2] + size[2]
  done = set()
  for z0, z1 in block_ranges(sorted_z, z_lo, z_hi):
    if backward:
      xblock_post = _section(cross_block, z_map[z0], dev)
    else:
      xblock_post = _section(cross_block, z_map[z1], dev)
    if not backward and z0 > 0:
      xblock_pre = _section(cross_block, z_map[z0], dev)
      xblock_pre_inv = _section(cross_block_inv, z_map[z0], dev)
    elif backward and z1 < sorted_z[-1]:
      xblock_pre = _section(cross_block, z_map[z1], dev)
      xblock_pre_inv = _section(cross_block_inv, z_map[z1], dev)
    else:
      xblock_pre_inv = xblock_pre = torch.zeros_like(xblock_post)
    if backward:
      block_end_inv = _section(last_inv if z0 != sorted_z[0] else main_inv, z0, dev)
    else:
      block_end_inv = _section(last_inv if z1 != sorted_z[-1] else main_inv, z1, dev)

    inner, st0 = map_utils._compose_launch(xblock_pre_inv, flat, stride, block_end_inv, flat,
                                           stride)
    offset, st1 = map_utils._compose_launch(inner, flat, stride, xblock_post, flat, stride)
    status = [st0, st1]

    block_size = z1 - z0
    interior, scales = [], []
    for z in range(max(z_lo, z0), min(z_hi, z1 + 1)):
      i = z - z0
      if z in done:
        continue
      rel_z = z - z_lo
      if i == block_size:
        ret[:, rel_z:rel_z + 1] = xblock_pre if backward else xblock_post
      elif i == 0:
        ret[:, rel_z:rel_z + 1] = xblock_post if backward else xblock_pre
      else:
        interior.append(rel_z)
        scales.append((block_size - i) / block_size if backward else i / block_size)
      done.add(z)
    if interior:
      idx = torch.tensor(interior, dtype=torch.int64, device=dev)
      stack = ret.index_select(1, idx)
      n = len(interior)
      stack_box = types.SimpleNamespace(start=flat.start, size=(size[0], size[1], n))
      aligned, st2 = map_utils._compose_launch(stack, stack_box, stride, xblock_pre, flat,
                                               stride)
      scale2 = torch.tensor(scales, dtype=torch.float64, device=dev)
      final, st3 = map_utils._compose_launch(aligned, stack_box, stride, offset, flat, stride,
                                             scale2=scale2)
      ret.index_copy_(1, idx, final)
      status += [st2, st3]
    # one read per block; "slice" k is the k-th composition of the block:
    # 0 block_end_inv, 1 xblock_post, 2 xblock_pre, 3 the scaled offset
    map_utils._raise_refused(f'reconcile_cross_block_maps, block {z0}:{z1}', torch.cat(status))

  assert not set(range(z_lo, z_hi)) - done
  return DeviceArray(torch.where(torch.isnan(data), torch.full_like(ret, float('nan')), ret))
