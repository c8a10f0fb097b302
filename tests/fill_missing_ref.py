"""Brute-force NumPy statement of the contract of `map_utils.fill_missing` on the
device: the reference's semantics (map_utils.py:227-304) without its Delaunay
branch, and with the tie rule that the device states -- among equidistant valid
nodes the lowest C-order index of [z,] y, x.  Integer distances, no k-d tree.
"""
import numpy as np


def nearest_valid(valid, chunk=4096):
  """For a bool lattice `valid` with at least one True: (idx, unique), flat
  arrays over the lattice in C order.  idx[p] is the flat index of the valid
  node at the smallest squared Euclidean distance in node indices from p, the
  lowest index among equidistant ones; unique[p] says that no other valid node
  is as near."""
  shape = valid.shape
  coords = np.stack(np.unravel_index(np.arange(valid.size), shape), axis=1).astype(np.int64)
  flat_valid = np.flatnonzero(valid.ravel())          # ascending C order
  vc = coords[flat_valid]
  idx = np.empty(valid.size, np.int64)
  unique = np.empty(valid.size, bool)
  for lo in range(0, valid.size, chunk):
    q = coords[lo:lo + chunk]
    d2 = ((q[:, None, :] - vc[None, :, :]) ** 2).sum(axis=2)
    first = d2.argmin(axis=1)                         # the first minimum: the lowest index
    idx[lo:lo + chunk] = flat_valid[first]
    unique[lo:lo + chunk] = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) == 1
  return idx, unique


def tied_candidates(valid, p):
  """Flat indices of all valid nodes nearest to the node of flat index p."""
  coords = np.stack(np.nonzero(valid), axis=1).astype(np.int64)
  q = np.array(np.unravel_index(p, valid.shape), np.int64)
  d2 = ((coords - q) ** 2).sum(axis=1)
  return np.ravel_multi_index(tuple(coords[d2 == d2.min()].T), valid.shape)


def fill_missing_ref(coord_map, *, extrapolate=False, invalid_to_zero=False,
                     interpolate_first=True):
  m = np.asarray(coord_map)
  assert m.ndim == 4 and m.shape[0] in (2, 3)
  if not np.isnan(m).any():
    return m.copy()
  if interpolate_first:
    raise NotImplementedError('Delaunay branch')
  out = m.copy()
  problems = [np.s_[:, z] for z in range(m.shape[1])] if m.shape[0] == 2 else [np.s_[:]]
  for sel in problems:
    src, dst = m[sel], out[sel]                       # dst is a view of out
    valid = np.isfinite(src).all(axis=0)
    if not valid.any():
      if invalid_to_zero:
        dst[...] = 0
      elif extrapolate:
        dst[...] = np.nan
      continue
    if not extrapolate or valid.all():
      continue
    idx, _ = nearest_valid(valid)
    dst[...] = src.reshape(src.shape[0], -1)[:, idx].reshape(src.shape)
  return out


def cases(g):
  out = []
  i = 0
  while f'c{i:02d}_name' in g.files:
    p = f'c{i:02d}_'
    out.append(dict(name=str(g[p + 'name']), map=g[p + 'map'], out=g[p + 'out'],
                    unique=g[p + 'unique'], filled=g[p + 'filled'],
                    kw=dict(extrapolate=bool(g[p + 'extrapolate']),
                            invalid_to_zero=bool(g[p + 'invalid_to_zero']),
                            interpolate_first=False)))
    i += 1
  return out


def bits(a):
  return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)
