"""Generates tests/golden/reconcile_filter.npz by driving the UNMODIFIED
reference `ReconcileAndFilterFlows.process` (processor/flow.py:386-493) over
in-memory volumes: a subclass supplies `_get_metadata`, `_open_volume`,
`_build_mask`, `_get_mask_configs`, `_context` and `crop_box_and_data` (the
members of the volume framework that `process` calls), `_refshim` makes the
imports resolve, and the stand-in modules processor/flow.py needs beyond it
are registered here, before the import.  The box handed to `process` carries
the framework's `scale` (start floored, end ceiled); it only decides which
slab of the coarse volume is read, and the slab and its box are stored.

Build-container only.  The coarse flows are affine in position with NaN blobs,
with coefficients that are multiples of 1/64, so the float32 flows are affine
exactly and every Delaunay triangulation of their valid nodes interpolates the
same values: the reference's output is the one answer (`run_case` asserts that
every upsampled vector equals the affine function to the bit); the thresholds
lie well away from the values.
  affine   a 4-channel base flow with holes, a 4-channel coarse flow at scale 0.5
  multi    multi_section with base_delta_z 1: a 2-channel base flow, a 3-channel
           coarse flow with an explicit divisor of 0.25, a mask
  clipped  the coarse volume ends inside the box: fine nodes outside the coarse
           grid
Stored per case: the config (JSON), the box, the base flow, per coarse flow the
slab that was read with its read box, scale and divisor, the mask (or an empty
array) and the output.  Run:
  python tests/golden/make_golden_reconcile_filter.py
"""
import contextlib
import json
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()


class _Subvolume:

  def __init__(self, data, bbox):
    self.data, self.bbox = data, bbox


def _register(name, **attrs):
  mod = types.ModuleType(name)
  mod.__dict__.update(attrs)
  sys.modules[name] = mod
  parent, _, leaf = name.rpartition('.')
  setattr(sys.modules[parent], leaf, mod)


_register('connectomics.common.beam_utils',
          counter=lambda namespace, name: None,
          timer_counter=lambda namespace, name: contextlib.nullcontext())
_register('connectomics.volume.metadata', VolumeMetadata=type('VolumeMetadata', (), {}),
          DecoratedVolume=type('DecoratedVolume', (), {}))
_register('connectomics.volume.subvolume', Subvolume=_Subvolume)

from connectomics.common import bounding_box  # noqa: E402
from sofima.processor import flow as rflow  # noqa: E402


class Box(bounding_box.BoundingBox):
  """The box `process` receives: the framework's `scale`."""

  def scale(self, factor):
    factor = np.asarray(factor, np.float64)
    return bounding_box.BoundingBox(start=np.floor(self.start * factor).astype(np.int64),
                                    end=np.ceil(self.end * factor).astype(np.int64))


class Volume:
  """What `_open_volume` returns: CZYX data from the origin."""

  def __init__(self, data):
    self.data = data
    self.read = []

  def clip_box_to_volume(self, box):
    c, z, y, x = self.data.shape
    return box.intersection(bounding_box.BoundingBox(start=(0, 0, 0), size=(x, y, z)))

  def __getitem__(self, key):
    self.read.append(key)
    return self.data[key]


class Proc(rflow.ReconcileAndFilterFlows):

  def __init__(self, config, volumes, pixel_sizes, mask, context):
    self.volumes, self.pixel_sizes, self.mask = volumes, pixel_sizes, mask
    self._context = (np.array(context), np.array(context))
    super().__init__(config)

  def _get_metadata(self, path):
    px = self.pixel_sizes[path]
    return types.SimpleNamespace(path=path, pixel_size=types.SimpleNamespace(x=px, y=px, z=1.0))

  def _get_mask_configs(self, configs):
    return configs

  def _open_volume(self, path):
    return self.volumes[path]

  def _build_mask(self, mask_configs, box):
    return self.mask[box.to_slice3d()].copy()

  def crop_box_and_data(self, box, data):
    return _Subvolume(data, box)


def blobs(rng, shape, frac):
  noise = ndimage.gaussian_filter(rng.standard_normal(shape), (0, 1.2, 1.2))
  return noise > np.quantile(noise, 1 - frac)


def affine_flow(rng, channels, z, y, x, hole_frac):
  """[channels, z, y, x] float32 over a volume from the origin: vectors affine
  in the position per section, peak statistics far above the thresholds, a
  third channel of small integers when channels == 3.  The coefficients are
  multiples of 1/64 (exact in binary), so every vector is a multiple of 1/64
  below 8 and the float32 flow is exactly affine: interpolants at the half
  positions of a 2 x upsampling are multiples of 1/128, exact in float32 too."""
  yy, xx = np.mgrid[:y, :x].astype(np.float64)
  flow = np.zeros((channels, z, y, x), np.float32)
  coeffs = np.zeros((z, 2, 3))
  for k in range(z):
    a = rng.integers(-3, 4, (2, 3)) / 64.0
    a[:, 1:][a[:, 1:] == 0] = 1 / 64.0          # no constant plane
    coeffs[k] = a
    for c in range(2):
      exact = 4 * a[c, 0] + a[c, 1] * xx + a[c, 2] * yy
      flow[c, k] = exact
      assert np.array_equal(flow[c, k].astype(np.float64), exact)
  if channels == 4:
    flow[2:] = rng.uniform(3.0, 4.0, (2, z, y, x))
  if channels == 3:
    flow[2] = rng.integers(1, 4, (z, y, x))
  flow[:, blobs(rng, (z, y, x), hole_frac)] = np.nan
  return flow, coeffs


def base_flow(rng, channels, z, y, x, hole_frac):
  flow = rng.uniform(-1.5, 1.5, (channels, z, y, x)).astype(np.float32)
  if channels == 4:
    flow[2:] = rng.uniform(3.0, 4.0, (2, z, y, x))
  flow[:, blobs(rng, (z, y, x), hole_frac)] = np.nan
  return flow


THRESHOLDS = dict(min_peak_ratio=1.5, min_peak_sharpness=1.5, max_magnitude=20.0,
                  max_deviation=10.0, max_gradient=10.0, min_patch_size=4)


def run_case(name, base, coarse, coarse_px, divisor, box, mask, context, multi_section,
             base_delta_z):
  coarse, coeffs = coarse
  volumes = {'base': Volume(base), 'coarse': Volume(coarse)}
  spec = 'coarse' if divisor is None else f'coarse:{divisor}'
  config = rflow.ReconcileAndFilterFlows.Config(
      flow_volinfos=['base', spec], mask_configs='mask' if mask is not None else None,
      multi_section=multi_section, base_delta_z=base_delta_z, **THRESHOLDS)
  proc = Proc(config, volumes, {'base': 8.0, 'coarse': coarse_px}, mask, context)
  result = proc.process(_Subvolume(None, box))
  key = volumes['coarse'].read[-1]
  read_start = [key[3].start, key[2].start, key[1].start]
  read_size = [key[3].stop - key[3].start, key[2].stop - key[2].start,
               key[1].stop - key[1].start]
  out = result.data
  base_box = base[(slice(None),) + box.to_slice3d()]
  filled = np.isnan(base_box[0]) & ~np.isnan(out[0])
  assert filled.sum() > 50
  # the one answer: every upsampled vector is the affine function itself, to the bit
  scale = 8.0 / coarse_px
  qy, qx = np.mgrid[:box.size[1], :box.size[0]]
  qx, qy = (qx + box.start[0]) * scale, (qy + box.start[1]) * scale
  for k in range(out.shape[1]):
    for c in range(2):
      a = coeffs[k, c]
      exact = (4 * a[0] + a[1] * qx + a[2] * qy) / (scale if divisor is None else divisor)
      assert np.array_equal(out[c, k][filled[k]].astype(np.float64), exact[filled[k]]), (name, k, c)
  return {
      'config': np.array(json.dumps(dict(THRESHOLDS, multi_section=multi_section,
                                         base_delta_z=base_delta_z))),
      'box': np.array([box.start, box.size], np.int64),
      'base': base_box.copy(),
      'coarse': coarse[key].copy(),
      'read_box': np.array([read_start, read_size], np.int64),
      'scale': np.array([8.0 / coarse_px, np.nan if divisor is None else divisor]),
      'mask': (mask[box.to_slice3d()] if mask is not None else np.zeros((0,), bool)),
      'out': out,
  }


def main():
  rng = np.random.default_rng(31)
  box = Box(start=(10, 6, 0), size=(28, 24, 2))
  cases = {}
  cases['affine'] = run_case(
      'affine', base_flow(rng, 4, 2, 40, 48, 0.25), affine_flow(rng, 4, 2, 24, 28, 0.12),
      16.0, None, box, None, (1, 1, 0), False, 0)
  mask = np.zeros((2, 40, 48), bool)
  mask[0, 10:16, 20:30] = True
  mask[1, 22:, :14] = True
  cases['multi'] = run_case(
      'multi', base_flow(rng, 2, 2, 40, 48, 0.3), affine_flow(rng, 3, 2, 24, 28, 0.1),
      16.0, 0.25, box, mask, (2, 2, 0), True, 1)
  # the coarse volume ends at x 16, y 13: fine nodes beyond x 30 and y 24 are outside
  cases['clipped'] = run_case(
      'clipped', base_flow(rng, 4, 2, 40, 48, 0.25), affine_flow(rng, 4, 2, 13, 16, 0.1),
      16.0, None, box, None, (1, 1, 0), False, 0)
  arrays = {}
  for name, case in cases.items():
    for key, value in case.items():
      arrays[f'{name}_{key}'] = value
  arrays['names'] = np.array(list(cases))
  path = os.path.join(HERE, 'reconcile_filter.npz')
  np.savez_compressed(path, **arrays)
  print(f'{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
  main()
