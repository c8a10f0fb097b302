"""processor_maps.reconcile_cross_block_maps on the device: against a golden of
the unmodified reference processor (affine volumes: the answer does not depend
on the triangulation), and bit for bit against a host-driven loop of public
`compose_maps` calls in the reference's statement order on generic float32
data."""
import os

import numpy as np
import pytest
import torch

from sofima_amd import map_utils, processor_maps
from sofima_amd._dev import DeviceArray
from tests import compose_maps_scipy as cms

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'reconcile_cross_block.npz')
VOLUMES = ('cross_block', 'cross_block_inv', 'last_inv', 'main_inv')


def loaders(volumes, box, resident=False):
  """z -> [2, 1, y, x] over the box's xy extent of CZYX volumes from the origin."""
  x0, y0 = box.start[0], box.start[1]
  nx, ny = box.size[0], box.size[1]

  def make(vol):
    def load(z):
      sec = np.ascontiguousarray(vol[:, z:z + 1, y0:y0 + ny, x0:x0 + nx])
      return DeviceArray(torch.from_numpy(sec).cuda()) if resident else sec
    return load

  return {name: make(volumes[name]) for name in VOLUMES}


def same_bits(a, b):
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('name', ['forward', 'backward', 'inside'])
def test_golden_of_the_reference_processor(name):
  g = np.load(GOLDEN)
  box = cms.box(*g[f'{name}_box'])
  data, want = g[f'{name}_map'], g[f'{name}_out']
  keep = data.copy()
  z_map = {int(k): int(v) for k, v in g['z_map']}
  got = processor_maps.reconcile_cross_block_maps(
      data, box, z_map=z_map, stride=int(g['stride']), backward=bool(g[f'{name}_backward']),
      **loaders({v: g[v] for v in VOLUMES}, box))
  assert isinstance(got, DeviceArray)
  got = np.asarray(got)
  assert same_bits(data, keep)
  assert got.dtype == want.dtype and got.shape == want.shape
  assert np.array_equal(np.isnan(got), np.isnan(want))
  err = np.nanmax(np.abs(got - want))
  print(name, 'max error', err, 'finite', np.isfinite(want).mean())
  assert err <= 1e-6


def host_loop(data, box, volumes, z_map, stride, backward):
  """The reference's `process` / `_interpolate`, statement by statement, with
  the public device `compose_maps` for every composition."""
  load = loaders(volumes, box)
  sorted_z = sorted(z_map)
  flat = cms.box(box.start, (box.size[0], box.size[1], 1))

  def compose(m1, m2):
    return np.asarray(map_utils.compose_maps(np.ascontiguousarray(m1), flat, stride,
                                             np.ascontiguousarray(m2), flat, stride))

  ret = data.copy()
  done = set()
  z_lo, z_hi = box.start[2], box.start[2] + box.size[2]
  for z0, z1 in processor_maps.block_ranges(sorted_z, z_lo, z_hi):
    xblock_post = load['cross_block'](z_map[z0] if backward else z_map[z1])
    if not backward and z0 > 0:
      xblock_pre = load['cross_block'](z_map[z0])
      xblock_pre_inv = load['cross_block_inv'](z_map[z0])
    elif backward and z1 < sorted_z[-1]:
      xblock_pre = load['cross_block'](z_map[z1])
      xblock_pre_inv = load['cross_block_inv'](z_map[z1])
    else:
      xblock_pre_inv = xblock_pre = np.zeros_like(xblock_post)
    if backward:
      block_end_inv = (load['last_inv'] if z0 != sorted_z[0] else load['main_inv'])(z0)
    else:
      block_end_inv = (load['last_inv'] if z1 != sorted_z[-1] else load['main_inv'])(z1)
    offset = compose(compose(xblock_pre_inv, block_end_inv), xblock_post)
    block_size = z1 - z0
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
        scale = (block_size - i) / block_size if backward else i / block_size
        aligned = compose(ret[:, rel_z:rel_z + 1], xblock_pre)
        ret[:, rel_z:rel_z + 1] = compose(aligned, offset * scale)
      done.add(z)
  ret[np.isnan(data)] = np.nan
  return ret


@pytest.mark.parametrize('backward', [False, True])
@pytest.mark.parametrize('resident', [False, True])
def test_generic_float32_equals_a_loop_of_public_calls(backward, resident):
  from scipy import ndimage
  rng = np.random.default_rng(13 + backward)
  ny, nx = 14, 17
  z_map = {0: 0, 3: 1, 8: 2}
  volumes = {
      'cross_block': rng.uniform(-1, 1, (2, 3, ny, nx)).astype(np.float32),
      'cross_block_inv': rng.uniform(-1, 1, (2, 3, ny, nx)).astype(np.float32),
      'last_inv': rng.uniform(-1, 1, (2, 9, ny, nx)).astype(np.float32),
      'main_inv': rng.uniform(-1, 1, (2, 9, ny, nx)).astype(np.float32),
  }
  noise = ndimage.gaussian_filter(rng.standard_normal((3, ny, nx)), (0, 1.2, 1.2))
  volumes['cross_block'][:, noise > np.quantile(noise, 0.95)] = np.nan
  data = rng.uniform(-1.5, 1.5, (2, 8, ny - 2, nx - 3)).astype(np.float32)
  data[:, 2:5, 4:6, 5:8] = np.nan
  box = cms.box((2, 1, 1), (nx - 3, ny - 2, 8))         # z 1 .. 8: starts inside the first block
  want = host_loop(data, box, volumes, z_map, 4, backward)
  src = DeviceArray(torch.from_numpy(data).cuda()) if resident else data
  got = processor_maps.reconcile_cross_block_maps(
      src, box, z_map=z_map, stride=4, backward=backward, **loaders(volumes, box, resident))
  got = np.asarray(got)
  assert got.dtype == np.float32
  interior = [k for k in range(8) if k + 1 not in z_map]
  assert np.isfinite(got[:, interior]).mean() > 0.3 and np.isnan(got).any()
  assert same_bits(got, want)
  if resident:
    assert same_bits(np.asarray(src), data)
