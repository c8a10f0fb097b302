"""NumPy restatements and fixture access shared by the prev_state tests
(tests/golden/prev_state.npz, written by tests/golden/make_golden_prev_state.py)."""
import json

import numpy as np
from scipy import ndimage


def composition_tolerance(avg):
  """4 * (2e-5 + 1e-5 * max|prev|): twice the composition tolerance of
  test_compose_maps_fast_golden (rtol 1e-5, atol 2e-5) on each of the two nodes
  of a neighbour difference."""
  return 4 * (2e-5 + 1e-5 * np.nanmax(np.abs(avg)))


def threshold_margin(avg, stride, min_frac, max_frac):
  """Least distance of a neighbour difference (+ stride) of a [2, y, x] map to a
  fold limit of mask_irregular."""
  sx, sy = stride
  dx = np.diff(avg[0], axis=-1) + sx
  dy = np.diff(avg[1], axis=-2) + sy
  gaps = [np.abs(d - f * s) for d, s in ((dx, sx), (dy, sy)) for f in (min_frac, max_frac)]
  return min(float(np.nanmin(g)) for g in gaps if np.isfinite(g).any())


def mask_irregular_np(coord_map, stride, frac, max_frac=None, dilation_iters=1):
  """map_utils.py:737-786 in the map's own dtype; in place, returns the mask."""
  stride = np.asarray(stride)
  if max_frac is None:
    max_frac = 2 - frac
  stride_x, stride_y = stride
  diff_x = np.diff(coord_map[0, ...], axis=-1)
  diff_y = np.diff(coord_map[1, ...], axis=-2)
  diff_x = np.pad(diff_x, [[0, 0], [0, 1]], mode='constant') + stride_x
  diff_y = np.pad(diff_y, [[0, 1], [0, 0]], mode='constant') + stride_y
  bad = (diff_x < frac * stride_x) | (diff_y < frac * stride_y)
  bad |= (diff_x > max_frac * stride_x) | (diff_y > max_frac * stride_y)
  if dilation_iters > 0:
    bad = ndimage.binary_dilation(bad, ndimage.generate_binary_structure(2, 2),
                                  iterations=dilation_iters)
  coord_map[0, ...][bad] = np.nan
  coord_map[1, ...][bad] = np.nan
  return bad


class Case:
  """One case of the fixture: inputs and per-section records."""

  def __init__(self, g, name):
    self.g, self.name = g, name
    self.cfg = json.loads(str(g['cfg']))
    self.block_starts = [int(v) for v in g['block_starts']]
    self.min_frac, self.max_frac = float(g['min_frac']), float(g['max_frac'])
    self.backward = bool(g[name + '_backward'])
    self.skip = [int(v) for v in g[name + '_skip']]
    self.sections = [int(v) for v in g[name + '_sections']]
    self.mask = g['mask'] if bool(g[name + '_masked']) else None
    sign = -1 if self.backward else 1
    f2 = g['f2'].copy()
    f2[2] *= sign
    self.flow_arrays = [g['f0'], g['f1'], f2]
    self.delta_z = [sign * 1, sign * 2, sign * 1]

  def rec(self, z, key):
    return self.g[f'{self.name}_{z}_{key}']

  def has_prev(self, z):
    return bool(self.rec(z, 'hasprev'))

  def pairs(self, z):
    return [(int(a), int(b)) for a, b in self.rec(z, 'pairs')]

  def history(self):
    """The reference's own solved meshes, [2, nz, y, x] (zeros where it solved none)."""
    nz, y, x = self.flow_arrays[0].shape[1:]
    h = np.zeros((2, nz, y, x), np.float32)
    for z in self.sections:
      h[:, z] = self.rec(z, 'x')[:, 0]
    return h

  def flow_volumes(self):
    from sofima_amd import processor_mesh
    return [processor_mesh.FlowVolume(a, dz) for a, dz in zip(self.flow_arrays, self.delta_z)]

  def integration_config(self):
    from sofima_amd import mesh
    return mesh.IntegrationConfig(**self.cfg)
