"""Generates tests/golden/reconcile_cross_block.npz by driving the UNMODIFIED
reference `ReconcileCrossBlockMaps.process` (processor/maps.py:35-326) over
in-memory volumes: a subclass supplies `_open_volume` and `crop_box_and_data`
(the members of the volume framework that `process` calls), `_refshim` makes
the imports resolve, and the names processor/maps.py needs beyond it
(`subvolume_processor.SubvolumeOrMany`, `OutputNums`, `metadata.VolumeMetadata`)
are registered here, before the import.

Build-container only.  float64, a 12 x 14 lattice at stride 4 cut out of
16 x 18 volumes, 9 sections, z_map {0: 0, 4: 1, 8: 2}.  The four volumes are
affine in position with dyadic coefficients of at most 1/128 and offsets of at
most 0.25 (one cross-block slice has a NaN blob), so every map2 of every
composition is affine and the answer does not depend on the triangulation; the
main map is generic in +-1 with a NaN block.  Boundary nodes that land outside
the hull of the valid nodes are NaN, correctly: asserted here that at least
55 % of every interior section is finite and that each has a NaN, so a test
cannot pass on NaN alone.
  forward   the whole z range
  backward  the same data solved backward
  inside    a box that starts inside a block (z 2 .. 6) 
Run:
  python tests/golden/make_golden_cross_block.py
"""
import enum
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()


class _Subvolume:

  def __init__(self, data, bbox):
    self.data, self.bbox = data, bbox


class _OutputNums(enum.Enum):
  SINGLE = 1
  MULTI = 2


def _register(name, **attrs):
  mod = types.ModuleType(name)
  mod.__dict__.update(attrs)
  sys.modules[name] = mod
  parent, _, leaf = name.rpartition('.')
  setattr(sys.modules[parent], leaf, mod)


_register('connectomics.volume.metadata', VolumeMetadata=type('VolumeMetadata', (), {}),
          DecoratedVolume=type('DecoratedVolume', (), {}))
_register('connectomics.volume.subvolume', Subvolume=_Subvolume)
_register('connectomics.volume.subvolume_processor',
          SubvolumeProcessor=type('SubvolumeProcessor', (), {}),
          SubvolumeOrMany=_Subvolume, OutputNums=_OutputNums,
          SuggestedXyz=type('SuggestedXyz', (), {}), TupleOrSuggestedXyz=tuple)

from connectomics.common import bounding_box  # noqa: E402
from sofima.processor import maps as rmaps  # noqa: E402

STRIDE = 4
Z_MAP = {0: 0, 4: 1, 8: 2}
VOL_YX = (16, 18)


class Proc(rmaps.ReconcileCrossBlockMaps):

  def __init__(self, config, volumes):
    self.volumes = volumes
    super().__init__(config)

  def _open_volume(self, path):
    return self.volumes[path]

  def crop_box_and_data(self, box, data):
    return _Subvolume(data, box)


def affine_volume(rng, nz):
  """[2, nz, y, x] float64 from the origin, affine in the node position per
  section: offsets multiples of 1/16 up to 0.25, slopes multiples of 1/256 up
  to 1/128."""
  yy, xx = np.mgrid[:VOL_YX[0], :VOL_YX[1]].astype(np.float64) * STRIDE
  vol = np.zeros((2, nz) + VOL_YX)
  for k in range(nz):
    for c in range(2):
      c0 = rng.integers(-4, 5) / 16.0
      c1, c2 = rng.integers(-2, 3, 2) / 256.0
      vol[c, k] = c0 + c1 * xx + c2 * yy
  return vol


def run_case(volumes, main, box, backward):
  config = rmaps.ReconcileCrossBlockMaps.Config(
      cross_block='cross_block', cross_block_inv='cross_block_inv', last_inv='last_inv',
      main_inv='main_inv', z_map={str(k): v for k, v in Z_MAP.items()}, stride=STRIDE,
      xy_overlap=0, backward=backward)
  proc = Proc(config, volumes)
  data = main[box.to_slice4d()].copy()
  keep = data.copy()
  out = proc.process(_Subvolume(data, box)).data
  assert np.array_equal(data, keep, equal_nan=True)
  assert out.shape == data.shape and out.dtype == data.dtype
  sorted_z = sorted(Z_MAP)
  for rel_z in range(out.shape[1]):
    z = rel_z + int(box.start[2])
    if z in sorted_z:
      continue
    frac = np.isfinite(out[:, rel_z]).all(axis=0).mean()
    print(f'  z {z}: {100 * frac:.0f} % finite')
    assert frac >= 0.55, (z, frac)
    assert np.isnan(out[:, rel_z]).any(), z
  # the block ranges and z ranges the tests compare with
  ranges = []
  z = int(box.start[2])
  while z < int(box.end[2]):
    s, e = proc._get_z_range(z)
    ranges.append((s, e))
    z = e + 1
  return data, out, np.array(ranges, np.int64)


def main():
  rng = np.random.default_rng(41)
  volumes = {
      'cross_block': affine_volume(rng, 3),
      'cross_block_inv': affine_volume(rng, 3),
      'last_inv': affine_volume(rng, 9),
      'main_inv': affine_volume(rng, 9),
  }
  volumes['cross_block'][:, 1, 7:10, 8:11] = np.nan      # a NaN blob in one slice
  main_map = rng.uniform(-1, 1, (2, 9) + VOL_YX)
  main_map[:, 2:7, 5:8, 6:9] = np.nan
  arrays = {name: vol for name, vol in volumes.items()}
  arrays['z_map'] = np.array(sorted(Z_MAP.items()), np.int64)
  arrays['stride'] = np.array(STRIDE, np.int64)
  arrays['z_range_of'] = np.array(
      [[z, *Proc(rmaps.ReconcileCrossBlockMaps.Config(
          cross_block='', cross_block_inv='', last_inv='', main_inv='',
          z_map={str(k): v for k, v in Z_MAP.items()}, stride=STRIDE), {})._get_z_range(z)]
       for z in range(9)], np.int64)
  cases = {
      'forward': (bounding_box.BoundingBox(start=(2, 3, 0), size=(14, 12, 9)), False),
      'backward': (bounding_box.BoundingBox(start=(2, 3, 0), size=(14, 12, 9)), True),
      'inside': (bounding_box.BoundingBox(start=(2, 3, 2), size=(14, 12, 5)), False),
  }
  for name, (box, backward) in cases.items():
    print(name)
    data, out, ranges = run_case(volumes, main_map, box, backward)
    arrays[f'{name}_box'] = np.array([box.start, box.size], np.int64)
    arrays[f'{name}_backward'] = np.array(backward)
    arrays[f'{name}_map'] = data
    arrays[f'{name}_ranges'] = ranges
    arrays[f'{name}_out'] = out
  arrays['names'] = np.array(list(cases))
  path = os.path.join(HERE, 'reconcile_cross_block.npz')
  np.savez_compressed(path, **arrays)
  print(f'{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
  main()
