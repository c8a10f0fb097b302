"""The montage fine-flow stage without a GPU: the per-pair filter chain restated
from what the repository already pins (`oracle.flow_utils_oracle.clean_flow`,
`tests.test_reconcile.reconcile_restated`), a NumPy statement of
`stitch_elastic.aggregate_arrays`, and the readers of tests/golden/tile_flows.npz.
Test infrastructure only."""
import numpy as np

from oracle import flow_utils_oracle
from tests.test_reconcile import reconcile_restated

CLEAN_KEYS = ('min_peak_ratio', 'min_peak_sharpness', 'max_magnitude', 'max_deviation')
RECONCILE_KEYS = ('max_gradient', 'max_deviation', 'min_patch_size')


def filter_pair(v, clean=None, reconcile=None):
  """One tile pair [c, h, w] -> [2, h, w] float32, filtered on its own extent."""
  v = np.asarray(v, np.float32)
  a = (flow_utils_oracle.clean_flow(v[:, None], **clean) if clean is not None
       else v[:2, None].copy())
  b = reconcile_restated([a], **reconcile) if reconcile is not None else a
  return b[:, 0]


def filter_flow_maps(flows, clean=None, reconcile=None):
  return {k: filter_pair(v, clean, reconcile) for k, v in flows.items()}


def aggregate_arrays(x_data, y_data, tile_coords, coarse_mesh, stride, tile_shape):
  """The packing of a montage, written from the contract: flows float64 and
  NaN-padded to the largest one, meshes float32 at the coarse position,
  NeighborInfo rows for the -x, +x, -y, +y neighbour of every tile."""
  (cx, fine_x, off_x), (cy, fine_y, off_y) = x_data, y_data
  idx = {tuple(t): i for i, t in enumerate(tile_coords)}
  n, dim = len(idx), len(stride)

  def pack(fine):
    full = [1] * dim
    for f in fine.values():
      full = [max(a, b) for a, b in zip(full, f.shape[1:])]
    out = np.full([dim, n] + full, np.nan, np.float64)
    for k, f in fine.items():
      if k in idx:
        out[(slice(None), idx[k]) + tuple(slice(0, s) for s in f.shape[1:])] = f[:dim]
    return out

  nbors = np.full((n, 4, 8 if dim == 2 else 11), -1, np.int64)
  for (tx, ty), i in idx.items():
    for e, (nbor, fk, coarse, fine, offs, axis) in enumerate((
        ((tx - 1, ty), (tx - 1, ty), cx, fine_x, off_x, 0),
        ((tx + 1, ty), (tx, ty), cx, fine_x, off_x, 0),
        ((tx, ty - 1), (tx, ty - 1), cy, fine_y, off_y, 1),
        ((tx, ty + 1), (tx, ty), cy, fine_y, off_y, 1))):
      if fk not in fine:
        continue
      c = coarse[:, fk[1], fk[0]]
      size = fine[fk].shape[1:]
      row = [idx[nbor], idx[fk], c[1 - axis], size[-2 + axis], size[-1 - axis],
             offs[fk][0], offs[fk][1], axis]
      if dim == 3:
        row += [c[2], size[0], offs[fk][2]]
      nbors[i, e] = np.trunc(np.array(row, np.float64)).astype(np.int64)
  x = np.zeros([dim, n] + [int(t) // int(s) for t, s in zip(tile_shape, stride)], np.float32)
  for (tx, ty), i in idx.items():
    x[:, i] = np.asarray(coarse_mesh)[:, ty, tx].reshape((dim,) + (1,) * dim)
  return pack(fine_x), pack(fine_y), x, nbors, idx


# -- tests/golden/tile_flows.npz ------------------------------------------------
def parameter_sets(g):
  """name -> (clean dict or None, reconcile dict or None); the thresholds are
  Python numbers, np.float64 scalars where the reference was given those."""
  out = {}
  for name in g['params']:
    thr, (has_clean, has_rec, f64) = g[f'{name}_thr'], g[f'{name}_flags']
    num = np.float64 if f64 else float
    clean = dict(zip(CLEAN_KEYS, (num(t) for t in thr[:4]))) if has_clean else None
    rec = None
    if has_rec:
      rec = dict(max_gradient=num(thr[4]), max_deviation=num(thr[5]),
                 min_patch_size=int(thr[6]))
    out[str(name)] = (clean, rec)
  return out


def montage(g, name):
  """The flow dicts, offsets and aggregate_arrays arguments of one montage."""
  m = {'name': str(name)}
  for d in 'xy':
    keys = [tuple(int(v) for v in k) for k in g[f'{name}_{d}_keys']]
    m[d] = {k: g[f'{name}_{d}_flow_{i}'] for i, k in enumerate(keys)}
    m[d + '_offsets'] = {k: tuple(int(v) for v in o)
                         for k, o in zip(keys, g[f'{name}_{d}_offsets'])}
  m['tiles'] = [tuple(int(v) for v in t) for t in g[f'{name}_tiles']]
  m['stride'] = tuple(int(v) for v in g[f'{name}_stride'])
  m['tile_shape'] = tuple(int(v) for v in g[f'{name}_tile_shape'])
  for k in ('cx', 'cy', 'coarse'):
    m[k] = g[f'{name}_{k}']
  m['want'] = tuple(g[f'{name}_agg_{k}'] for k in ('fx', 'fy', 'x', 'nbors'))
  m['want_idx'] = {(int(a), int(b)): int(i) for a, b, i in g[f'{name}_agg_idx']}
  return m


def aggregate_args(m, fine_x=None, fine_y=None):
  return ((m['cx'], m['x'] if fine_x is None else fine_x, m['x_offsets']),
          (m['cy'], m['y'] if fine_y is None else fine_y, m['y_offsets']),
          m['tiles'], m['coarse'], m['stride'], m['tile_shape'])


def filter_cases(g):
  """(montage name, 'x' | 'y', parameter-set name, flows, clean, reconcile,
  {key: expected}) for every 2-D montage and parameter set."""
  psets = parameter_sets(g)
  for name in g['montages']:
    m = montage(g, name)
    if len(m['stride']) != 2:
      continue
    for d in 'xy':
      for pname, (clean, rec) in psets.items():
        want = {k: g[f'{name}_{d}_{pname}_out_{i}'] for i, k in enumerate(m[d])}
        yield str(name), d, pname, m[d], clean, rec, want


def same(a, b):
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
