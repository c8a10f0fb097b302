"""Generates tests/golden/prev_state.npz by driving the UNMODIFIED reference
`RelaxMesh.get_prev_state` / `run_relaxation` (processor/mesh.py:170-552) over
in-memory arrays: a subclass supplies `_open_volume`, `_load_stitched_tile`
and `_build_mask`, `_refshim` makes the imports resolve.

The boxes carry float starts, so that the stand-in builds compose_maps_fast's
lattice in float32, as JAX does; with integer starts NumPy promotes the int32
lattice plus the float32 map to float64 and the stand-in would compose at a
precision the reference does not have (4.9e-4 apart at coordinate 2760).

Build-container only.  Two cases over the same flows, mesh [19, 70] x 6
sections, block_starts [0, 4], the `relax_passes` integration config:
  fwd  forward, section 1 skipped, no mask, sections 0..5
  bwd  backward (every look-back negated), section 3 skipped, a tissue mask,
       sections 4..0
Stored: the inputs (f0, f1: 2-channel flows for |dz| 1 and 2 with NaN holes;
f2: 3-channel flow, channel 2 in {0, 1, 2, 3, NaN}; the bwd case reads channel
2 negated), and per case and solved section z the (flow, ref z) pairs the
reference loaded, the average before mask_irregular (`avg`), `prev`, the
solution x, energies, steps and status.  Sections whose prev is None have
`hasprev` 0 and no avg / prev.
Run:
  python tests/golden/make_golden_prev_state.py
"""
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
from connectomics.common import bounding_box  # noqa: E402
from sofima import mesh as rmesh  # noqa: E402
from sofima.processor import mesh as rproc  # noqa: E402

SEED = 5
NZ, Y, X = 6, 19, 70
BLOCK_STARTS = [0, 4]
MIN_FRAC, MAX_FRAC = 0.5, 1.5
CFG = dict(dt=0.001, gamma=0.0, k0=0.3, k=0.1, stride=(40, 40), num_iters=100,
           max_iters=400, stop_v_max=0.005, dt_max=1000, start_cap=1e6,
           final_cap=1e6, prefer_orig_order=True)
CASES = {
    'fwd': dict(backward=False, skip=[1], masked=False, sections=[0, 1, 2, 3, 4, 5]),
    'bwd': dict(backward=True, skip=[3], masked=True, sections=[4, 3, 2, 1, 0]),
}


def tolerance(prev):
  """Twice the composition tolerance (rtol 1e-5, atol 2e-5) on each of two nodes."""
  return 4 * (2e-5 + 1e-5 * np.nanmax(np.abs(prev)))


def threshold_margin(avg, stride, min_frac, max_frac):
  """Least distance of a pre-mask neighbour difference (+ stride) to a fold limit."""
  sx, sy = stride
  dx = np.diff(avg[0], axis=-1) + sx
  dy = np.diff(avg[1], axis=-2) + sy
  gaps = [np.abs(d - f * s) for d, s in ((dx, sx), (dy, sy)) for f in (min_frac, max_frac)]
  # the zero-padded far edge compares the bare stride: a constant, never near
  return min(float(np.nanmin(g)) for g in gaps if np.isfinite(g).any())


class Vol:
  """An in-memory volume: what `_open_volume` returns."""

  def __init__(self, index, arr):
    self.index = index
    self.arr = arr
    self.meta = types.SimpleNamespace(num_channels=arr.shape[0])

  def __getitem__(self, sl):
    return self.arr[sl].copy()


class Proc(rproc.RelaxMesh):

  def __init__(self, config, mask):
    super().__init__(config)
    self.mask = mask
    self.history = {}     # z -> [2, 1, y, x] float32, the stitched output
    self.cur_flow = None
    self.pairs = []

  def _open_volume(self, vol):
    self.cur_flow = vol.index
    return vol

  def _load_stitched_tile(self, output_dir, box):
    z = int(box.start[2])
    self.pairs.append((self.cur_flow, z))
    return self.history[z].copy()

  def _build_mask(self, mask_config, box):
    return self.mask[box.to_slice3d()].copy()


def make_flows(rng):
  def smooth(amp, sigma):
    f = ndimage.gaussian_filter(rng.standard_normal((2, NZ, Y, X)), (0, 0, sigma, sigma))
    return f / np.abs(f).max() * amp

  f0 = smooth(12.0, 3) + rng.standard_normal((2, NZ, Y, X)) * 0.3
  f1 = smooth(12.0, 3) + rng.standard_normal((2, NZ, Y, X)) * 0.3
  f0[0, :, 8:11, 30:33] += 45.0               # a fold for mask_irregular to find
  f0[:, :, 2:5, 50:58] = np.nan
  f0[:, 2, :, :6] = np.nan
  f1[:, :, 12:16, 10:20] = np.nan
  f1[:, :, 2:4, 52:56] = np.nan
  f2 = np.concatenate([smooth(10.0, 3), np.zeros((1, NZ, Y, X))])
  dz = rng.integers(0, 4, size=(NZ, Y, X)).astype(np.float64)
  dz[rng.random((NZ, Y, X)) < 0.1] = np.nan
  dz[:, 2:5, 50:58] = np.where(rng.random((NZ, 3, 8)) < 0.5, 0, np.nan)   # count 0 nodes
  f2[2] = dz
  f2[:2, :, 6:8, 60:64] = np.nan
  return [a.astype(np.float32) for a in (f0, f1, f2)]


def run_case(name, spec, flows, mask, rng):
  sign = -1 if spec['backward'] else 1
  f2 = flows[2].copy()
  f2[2] *= sign
  vols = [rproc.FlowVolume(sign * 1, Vol(0, flows[0])), rproc.FlowVolume(sign * 2, Vol(1, flows[1])),
          rproc.FlowVolume(sign * 1, Vol(2, f2))]
  icfg = rmesh.IntegrationConfig(**CFG)
  config = rproc.RelaxMesh.Config(
      output_dir='', integration_config=icfg, mesh=None, flows=vols,
      sections_to_skip=spec['skip'], ranges_to_skip=[], mask='mask' if spec['masked'] else None,
      block_starts=BLOCK_STARTS, block_ends=[], backward=spec['backward'],
      mesh_min_frac=MIN_FRAC, mesh_max_frac=MAX_FRAC, coming_in=[])
  proc = Proc(config, mask)
  captured = {}
  real_mask_irregular = rproc.map_utils.mask_irregular

  def spy(coord_map, *a, **k):
    if captured.get('armed'):
      captured['avg'] = coord_map.copy()
      captured['armed'] = False
    return real_mask_irregular(coord_map, *a, **k)

  out = {}
  seen = dict(count0=False, count2=False, lookbacks=set())
  rproc.map_utils.mask_irregular = spy
  try:
    for z in spec['sections']:
      # float starts: the stand-in's lattice becomes float32, as JAX's is (an int32
      # lattice plus a float32 map is float32 in JAX, but float64 in NumPy, which
      # would compose at a precision the reference does not have)
      box = bounding_box.BoundingBox(start=np.array((0, 0, z), np.float64), size=(X, Y, 1))
      proc.pairs = []
      captured.update(armed=True, avg=None)
      prev = proc.get_prev_state(icfg.stride, box)
      pairs = list(proc.pairs)
      avg = captured['avg']
      captured['armed'] = False
      x, e_kin, steps, status = proc.run_relaxation(box)
      proc.history[z] = np.asarray(x, dtype=np.float32)
      key = f'{name}_{z}'
      out[key + '_hasprev'] = np.int64(prev is not None)
      out[key + '_pairs'] = np.array(pairs, np.int64).reshape(-1, 2)
      out[key + '_x'] = proc.history[z]
      out[key + '_ekin'] = np.asarray(e_kin, np.float64)
      out[key + '_steps'] = np.int64(steps)
      out[key + '_status'] = np.int64(int(status))
      print(name, z, 'pairs', pairs, 'status', int(status), 'steps', steps)
      if prev is None:
        continue
      out[key + '_avg'] = avg
      out[key + '_prev'] = prev
      tol = tolerance(avg)
      margin = threshold_margin(avg, icfg.stride, MIN_FRAC, MAX_FRAC)
      assert margin > tol, (name, z, margin, tol)
      n_ref = np.zeros((Y, X), int)
      for f, rz in pairs:
        if f < 2:
          n_ref += np.isfinite(flows[f][0, z])
        else:
          n_ref += f2[2, z] == z - rz
          seen['lookbacks'].add(z - rz)
      seen['count0'] |= bool((np.isnan(avg[0]) & (n_ref == 0)).any())
      seen['count2'] |= bool((n_ref >= 2).any())
      # the solver's outcome must not hinge on prev within the tolerance
      if int(status) != int(rproc.SolutionStatus.UNDEFINED):
        noise = rng.choice([-1.0, 1.0], size=prev.shape) * (2e-5 + 1e-5 * np.abs(prev))
        m = None if mask is None or not spec['masked'] else mask[z:z + 1]
        x2, _, steps2, status2 = proc.relax_mesh(np.zeros_like(prev), prev + noise, icfg, m)
        assert steps2 == steps and status2 == status, (name, z, steps2, status2)
        assert np.array_equal(np.isnan(x2), np.isnan(x)), (name, z)
  finally:
    rproc.map_utils.mask_irregular = real_mask_irregular
  assert seen['count0'] and seen['count2'], seen
  assert {abs(v) for v in seen['lookbacks']} >= {1, 2, 3}, seen
  vals = f2[2][np.isfinite(f2[2])]
  assert set(np.abs(vals).astype(int)) == {0, 1, 2, 3} and np.isnan(f2[2]).any()
  return out


def main():
  rng = np.random.default_rng(SEED)
  flows = make_flows(rng)
  mask = np.zeros((NZ, Y, X), bool)
  mask[:, :2, :] = True
  mask[2, 9:12, 40:44] = True
  arrays = dict(cfg=np.array(json.dumps(CFG)), block_starts=np.array(BLOCK_STARTS, np.int64),
                min_frac=np.float64(MIN_FRAC), max_frac=np.float64(MAX_FRAC),
                f0=flows[0], f1=flows[1], f2=flows[2], mask=mask,
                cases=np.array(list(CASES)))
  for name, spec in CASES.items():
    arrays[name + '_backward'] = np.bool_(spec['backward'])
    arrays[name + '_masked'] = np.bool_(spec['masked'])
    arrays[name + '_skip'] = np.array(spec['skip'], np.int64)
    arrays[name + '_sections'] = np.array(spec['sections'], np.int64)
    arrays.update(run_case(name, spec, flows, mask, rng))
  path = os.path.join(HERE, 'prev_state.npz')
  np.savez_compressed(path, **arrays)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
