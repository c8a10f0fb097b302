"""Generates tests/golden/tile_flows.npz from the UNMODIFIED reference:
`flow_utils.clean_flow` + `flow_utils.reconcile_flows` per tile pair (pure
NumPy / SciPy) and `stitch_elastic.aggregate_arrays` (pure NumPy; `_refshim`
only makes `import sofima` resolve).

Build-container only.  The file holds arrays only:

  montages   names of the montages; montage m has the flow dicts `x` and `y`:
             {m}_{x|y}_keys int [n, 2], {m}_{x|y}_flow_{i} [c, h, w] (3-D montage:
             [c, z, y, x]), {m}_{x|y}_offsets int [n, 2 or 3], and {m}_cx, {m}_cy,
             {m}_coarse, {m}_tiles int [t, 2], {m}_stride, {m}_tile_shape
  params     names of the parameter sets; {p}_thr float64 [7]: min_peak_ratio,
             min_peak_sharpness, max_magnitude, max_deviation (clean), max_gradient,
             max_deviation, min_patch_size (reconcile); {p}_flags int [3]: clean
             given, reconcile given, thresholds passed as np.float64 scalars
  filtered   {m}_{x|y}_{p}_out_{i}: clean_flow + reconcile_flows of pair i alone
             (2-D montages)
  aggregated {m}_agg_fx, _fy, _x, _nbors, _idx int [t, 3] (x, y, index)

The generator asserts what the fixture is for (see check_claims).
Run:  python tests/golden/make_golden_tile_flows.py
"""
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()
from sofima import flow_utils as rfu  # noqa: E402
from sofima import stitch_elastic as rse  # noqa: E402

NAN, INF = np.nan, np.inf
F32 = np.float32
STAGES = ('ratio', 'sharp', 'mag', 'cdev', 'grad', 'rdev', 'patch')


def pair_flow(rng, c, h, w, holes=0.25):
  """[c, h, w]: smooth vectors with outliers, sharpness, peak ratio, NaN blobs."""
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((h, w)), 1.5) * 12
                for _ in range(2)]).astype(F32)
  hit = rng.random((h, w)) < 0.08
  f[:, hit] += (rng.choice([-1, 1], size=(2, hit.sum())) *
                rng.uniform(3, 20, (2, hit.sum()))).astype(F32)
  if c == 4:
    sharp = rng.uniform(0.5, 6, (h, w)).astype(F32) * rng.choice([-1, 1], (h, w)).astype(F32)
    ratio = rng.choice([0, 0.2, 0.6, 1.5, 3.0], (h, w)).astype(F32)
    f = np.concatenate([f, sharp[None], ratio[None]])
  if holes and h * w > 4:
    noise = ndimage.gaussian_filter(rng.standard_normal((h, w)), 1.0)
    f[:, noise > np.quantile(noise, 1 - holes)] = NAN
  return f


def filter_pair(v, clean, reconcile):
  a = rfu.clean_flow(v[:, None].copy(), **clean) if clean is not None else v[:2, None].copy()
  b = rfu.reconcile_flows([a], **reconcile) if reconcile is not None else a
  assert b.dtype == F32
  return b[:, 0]


def padded_result(v, full, clean, reconcile):
  """The pair filtered inside a NaN-padded [c, Y, X] array, cropped back."""
  p = np.full((v.shape[0],) + full, NAN, F32)
  p[:, :v.shape[1], :v.shape[2]] = v
  return filter_pair(p, clean, reconcile)[:, :v.shape[1], :v.shape[2]]


def same(a, b):
  return np.array_equal(a, b, equal_nan=True)


def montages(rng):
  out = {}
  # 2 x 2: unequal extents, the vertical pair of column 1 is missing
  m = {'tiles': [(0, 0), (1, 0), (0, 1), (1, 1)], 'stride': (20, 20), 'tile_shape': (260, 240)}
  m['x'] = {(0, 0): pair_flow(rng, 4, 12, 5), (0, 1): pair_flow(rng, 4, 10, 5)}
  m['y'] = {(0, 0): pair_flow(rng, 4, 5, 11)}
  # the quirk pair: a single partially-NaN vector, nothing else invalid
  q = pair_flow(rng, 4, 6, 5, holes=0)
  q[:2] = np.clip(q[:2], -2, 2)
  q[0, 2, 3] = NAN
  m['x'][(0, 1)] = q
  out['m2x2'] = m
  # 3 x 2: 2- and 4-channel flows mixed, thin pairs; (0, 1) is the padding example
  # of the gradient test, constant 7 on [6, 5] beside larger pairs
  m = {'tiles': [(x, y) for y in range(2) for x in range(3)], 'stride': (20, 20),
       'tile_shape': (200, 200)}
  m['x'] = {(0, 0): pair_flow(rng, 4, 9, 4), (1, 0): pair_flow(rng, 2, 8, 4),
            (0, 1): np.full((2, 6, 5), 7, F32), (1, 1): pair_flow(rng, 4, 10, 3, holes=0.4)}
  m['y'] = {(0, 0): pair_flow(rng, 4, 4, 9), (1, 0): pair_flow(rng, 2, 1, 7, holes=0),
            (2, 0): pair_flow(rng, 4, 3, 10)}
  # smooth and sharp, but large: only the magnitude test objects
  m['y'][(2, 0)][:2] = 16
  m['y'][(2, 0)][2:] = 3
  # thresholds float32 cannot hold: planted float32(1.1) / float32(0.7) values
  e = np.zeros((4, 5, 4), F32)
  e[2] = 2
  e[3] = 2
  e[0, 1, 1] = F32(1.1)
  e[2, 3, 2] = F32(0.7)
  e[3, 1, 3] = F32(0.7)
  e[1, 3, 0] = F32(0.1)
  m['x'][(1, 0)] = e
  e2 = pair_flow(rng, 2, 8, 4)
  e2[0, 0, 0], e2[1, 7, 3] = INF, -INF
  m['x'][(0, 0)] = np.concatenate([e2, pair_flow(rng, 4, 8, 4, holes=0)[2:]])
  out['m3x2'] = m
  # 4 x 1: one row, no vertical pairs at all
  m = {'tiles': [(x, 0) for x in range(4)], 'stride': (16, 16), 'tile_shape': (128, 96)}
  m['x'] = {(0, 0): pair_flow(rng, 2, 7, 3), (1, 0): pair_flow(rng, 4, 8, 2),
            (2, 0): pair_flow(rng, 4, 1, 1, holes=0)}
  m['y'] = {}
  out['m4x1'] = m
  # no flow at all
  out['mnone'] = {'tiles': [(0, 0), (1, 0)], 'stride': (20, 20), 'tile_shape': (60, 80),
                  'x': {}, 'y': {}}
  for name, m in out.items():
    gx = max(t[0] for t in m['tiles']) + 1
    gy = max(t[1] for t in m['tiles']) + 1
    m['cx'] = rng.integers(-9, 10, (2, gy, gx)).astype(np.float64)
    m['cy'] = rng.integers(-9, 10, (2, gy, gx)).astype(np.float64)
    m['cx'][:, 0, 0] += 0.5                 # fractional offsets are truncated in nbors
    m['coarse'] = rng.normal(0, 30, (2, gy, gx))
    m['x_offsets'] = {k: tuple(int(v) for v in rng.integers(-40, 5, 2)) for k in m['x']}
    m['y_offsets'] = {k: tuple(int(v) for v in rng.integers(-40, 5, 2)) for k in m['y']}
  # 3-D montage, for aggregate_arrays only: flows [c, z, y, x], 11-field nbors
  m = {'tiles': [(0, 0), (1, 0), (0, 1)], 'stride': (10, 20, 20), 'tile_shape': (40, 100, 120),
       'x': {(0, 0): rng.normal(0, 2, (5, 3, 4, 2)).astype(F32)},
       'y': {(0, 0): rng.normal(0, 2, (3, 4, 2, 5)).astype(F32)}}
  m['x'][(0, 0)][:, 1, 2] = NAN
  m['cx'] = rng.integers(-9, 10, (3, 2, 2)).astype(np.float64)
  m['cy'] = rng.integers(-9, 10, (3, 2, 2)).astype(np.float64)
  m['coarse'] = rng.normal(0, 30, (3, 2, 2))
  m['x_offsets'] = {(0, 0): (-40, 3, 1)}
  m['y_offsets'] = {(0, 0): (2, -40, -1)}
  out['m3d'] = m
  return out


def parameter_sets():
  """name -> (clean or None, reconcile or None, thresholds are np.float64)."""
  def clean(ratio=0, sharp=0, mag=0, dev=0):
    return dict(min_peak_ratio=ratio, min_peak_sharpness=sharp, max_magnitude=mag,
                max_deviation=dev)

  def rec(grad=0, dev=0, patch=0):
    return dict(max_gradient=grad, max_deviation=dev, min_patch_size=patch)

  sets = {
      'ratio': (clean(ratio=1.0), None, False),
      'sharp': (clean(sharp=1.5), None, False),
      'mag': (clean(mag=14.0), None, False),
      'cdev': (clean(dev=5.0), None, False),
      'grad': (None, rec(grad=6.0), False),
      'rdev': (None, rec(dev=4.0), False),
      'patch': (None, rec(patch=3), False),
      'all': (clean(1.0, 1.5, 14.0, 5.0), rec(6.0, 4.0, 3), False),
      'all_loose': (clean(0.5, 0.8, 30.0, 12.0), rec(15.0, 10.0, 8), False),
      'nonpos': (clean(0, -1.0, 0, -2.0), rec(-1.0, 0, -3), False),
      'py_edge': (clean(0.7, 0.7, 1.1, 0), None, False),
      'f64_edge': (clean(0.7, 0.7, 1.1, 0), None, True),
      'py_rdev_edge': (None, rec(0, 0.1, 0), False),
      'f64_rdev_edge': (None, rec(0, 0.1, 0), True),
      'py_grad_edge': (None, rec(1.1, 0, 0), False),
  }
  out = {}
  for name, (c, r, f64) in sets.items():
    if f64:
      c = c and {k: np.float64(v) for k, v in c.items()}
      r = r and {k: (np.float64(v) if k != 'min_patch_size' else v) for k, v in r.items()}
    out[name] = (c, r, f64)
  return out


def flagged_by(v, clean, reconcile):
  """Which test flags which vector in the chain (clean, reconcile): the four
  clean tests flag the raw input, each alone; a reconcile test flags vectors that
  are still valid when its stage begins.  The stages run one after the other
  give the chain's result."""
  def newly(out, inp):
    return np.isnan(out).any(axis=0) & ~np.isnan(inp).any(axis=0)

  flags = {}
  for s, key in (('ratio', 'min_peak_ratio'), ('sharp', 'min_peak_sharpness'),
                 ('mag', 'max_magnitude'), ('cdev', 'max_deviation')):
    only = dict.fromkeys(clean, 0)
    only[key] = clean[key]
    flags[s] = newly(rfu.clean_flow(v[:, None].copy(), **only)[:, 0], v[:2])
  cur = rfu.clean_flow(v[:, None].copy(), **clean)
  for s, key in (('grad', 'max_gradient'), ('rdev', 'max_deviation'),
                 ('patch', 'min_patch_size')):
    only = dict.fromkeys(reconcile, 0)
    only[key] = reconcile[key]
    nxt = rfu.reconcile_flows([cur], **only)
    flags[s] = newly(nxt[:, 0], cur[:, 0])
    cur = nxt
  assert same(cur[:, 0], filter_pair(v, clean, reconcile))
  return flags


def check_claims(mont, psets, results):
  """What the fixture is for; a weak fixture must not pass silently."""
  # 1. every one of the seven tests flags, in some chain, a vector that no other
  #    test of the chain flags
  alone = {s: False for s in STAGES}
  quirk = False
  differs = {'grad': False, 'rdev': False, 'patch': False}
  for mname, m in mont.items():
    if mname == 'm3d':
      continue
    for d in 'xy':
      if not m[d]:
        continue
      full = tuple(np.max([v.shape[1:] for v in m[d].values()], axis=0))
      for k, v in m[d].items():
        for chain in ('all', 'all_loose'):
          flags = flagged_by(v, *psets[chain][:2])
          for s in STAGES:
            others = np.zeros(v.shape[1:], bool)
            for t in STAGES:
              if t != s:
                others |= flags[t]
            alone[s] |= bool((flags[s] & ~others).any())
        # 2. the invalid count of the pair's own extent: 0 < n0 < min_patch_size
        mp = psets['patch'][1]['min_patch_size']
        invalid = np.isnan(v[:2]).any(axis=0)
        if 0 < invalid.sum() < mp:
          out = results[mname, d, 'patch'][k]
          partial = invalid & ~np.isnan(v[:2]).all(axis=0)
          assert np.isnan(out[:, invalid]).all()
          quirk |= bool(partial.any())
        # 3. filtering the NaN-padded array is not filtering the pair
        if v.shape[1:] != full:
          for s in differs:
            c, r, _ = psets[s]
            differs[s] |= not same(padded_result(v, full, c, r), results[mname, d, s][k])
  assert all(alone.values()), alone
  assert quirk, 'no pair with 0 < n0 < min_patch_size and a partially NaN vector'
  assert all(differs.values()), differs
  # the float64 thresholds decide differently from the Python numbers
  for py, f64 in (('py_edge', 'f64_edge'), ('py_rdev_edge', 'f64_rdev_edge')):
    assert any(not same(results[m, d, py][k], results[m, d, f64][k])
               for (m, d, p) in results if p == py for k in results[m, d, p])


def main():
  rng = np.random.default_rng(11)
  mont = montages(rng)
  psets = parameter_sets()
  arrs = {'montages': np.array(list(mont)), 'params': np.array(list(psets))}
  for pname, (c, r, f64) in psets.items():
    thr = [c[k] if c else 0 for k in ('min_peak_ratio', 'min_peak_sharpness', 'max_magnitude',
                                      'max_deviation')]
    thr += [r[k] if r else 0 for k in ('max_gradient', 'max_deviation', 'min_patch_size')]
    arrs[f'{pname}_thr'] = np.array(thr, np.float64)
    arrs[f'{pname}_flags'] = np.array([c is not None, r is not None, f64], np.int64)
  results = {}
  for mname, m in mont.items():
    for d in 'xy':
      keys = list(m[d])
      arrs[f'{mname}_{d}_keys'] = np.array(keys, np.int64).reshape(len(keys), 2)
      nd = len(m['stride'])
      arrs[f'{mname}_{d}_offsets'] = np.array(
          [m[d + '_offsets'][k] for k in keys], np.int64).reshape(len(keys), nd)
      for i, k in enumerate(keys):
        arrs[f'{mname}_{d}_flow_{i}'] = m[d][k]
      if mname == 'm3d':
        continue
      for pname, (c, r, _) in psets.items():
        res = {}
        for i, k in enumerate(keys):
          before = m[d][k].copy()
          res[k] = filter_pair(m[d][k], c, r)
          assert same(before, m[d][k])
          arrs[f'{mname}_{d}_{pname}_out_{i}'] = res[k]
        results[mname, d, pname] = res
    for name in ('cx', 'cy', 'coarse'):
      arrs[f'{mname}_{name}'] = m[name]
    arrs[f'{mname}_tiles'] = np.array(m['tiles'], np.int64)
    arrs[f'{mname}_stride'] = np.array(m['stride'], np.int64)
    arrs[f'{mname}_tile_shape'] = np.array(m['tile_shape'], np.int64)
    fx, fy, x, nbors, idx = rse.aggregate_arrays(
        (m['cx'], m['x'], m['x_offsets']), (m['cy'], m['y'], m['y_offsets']), m['tiles'],
        m['coarse'], m['stride'], m['tile_shape'])
    assert fx.dtype == fy.dtype == np.float64 and x.dtype == F32 and nbors.dtype == np.int64
    arrs[f'{mname}_agg_fx'], arrs[f'{mname}_agg_fy'] = fx, fy
    arrs[f'{mname}_agg_x'], arrs[f'{mname}_agg_nbors'] = x, nbors
    arrs[f'{mname}_agg_idx'] = np.array([k + (i,) for k, i in idx.items()], np.int64)
  assert mont['mnone']['x'] == {} and arrs['mnone_agg_fx'].shape == (2, 2, 1, 1)
  assert arrs['m3d_agg_nbors'].shape[-1] == 11
  check_claims(mont, psets, results)
  path = os.path.join(HERE, 'tile_flows.npz')
  np.savez_compressed(path, **arrs)
  print(f'tile_flows: {len(mont)} montages, {len(psets)} parameter sets, '
        f'{os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
  main()
