"""Generates tests/golden/fill_missing.npz from the UNMODIFIED reference
`map_utils.fill_missing` with `interpolate_first=False` (NumPy / SciPy's
NearestNDInterpolator; `_refshim` only makes `import sofima` resolve).

Build-container only.  Per case `cNN_*`:
  name, map, extrapolate, invalid_to_zero   the input and the keywords
  out      the reference's result
  unique   bool [z, y, x]: the node was filled AND has exactly one nearest valid
           node (integer brute force below); there the reference's result is
           the contract, elsewhere its pick among equidistant nodes is an
           artefact of SciPy's k-d tree
  filled   bool [z, y, x]: the node was filled from another node
The generator asserts that the reference always picked A nearest node, and
that at least 60 % of every case's filled nodes are `unique` -- a fixture of
mostly tied nodes would pin nothing to the reference.
Run:
  python tests/golden/make_golden_fill_missing.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()
from sofima import map_utils as rmu  # noqa: E402

NAN = np.nan
MIN_UNIQUE = 0.6


def nearest_sets(valid):
  """(d2 [n, n_valid] int64, flat indices of the valid nodes) of a bool lattice."""
  coords = np.stack(np.unravel_index(np.arange(valid.size), valid.shape), axis=1).astype(np.int64)
  flat_valid = np.flatnonzero(valid.ravel())
  d2 = ((coords[:, None, :] - coords[flat_valid][None, :, :]) ** 2).sum(axis=2)
  return d2, flat_valid


def audit(cm, out, extrapolate):
  """unique / filled masks of one case; asserts the reference picked a nearest node."""
  dim = cm.shape[0]
  unique = np.zeros(cm.shape[1:], bool)
  filled = np.zeros(cm.shape[1:], bool)
  problems = [np.s_[z] for z in range(cm.shape[1])] if dim == 2 else [np.s_[:]]
  for sel in problems:
    src = cm[(slice(None),) + (sel,)] if dim == 2 else cm
    res = out[(slice(None),) + (sel,)] if dim == 2 else out
    valid = np.isfinite(src).all(axis=0)
    if not extrapolate or not valid.any() or valid.all():
      continue
    d2, flat_valid = nearest_sets(valid)
    near = d2 == d2.min(axis=1, keepdims=True)
    inv = ~valid.ravel()
    u = (near.sum(axis=1) == 1) & inv
    vals = src.reshape(dim, -1)
    got = res.reshape(dim, -1)
    for p in np.flatnonzero(inv):
      cands = flat_valid[near[p]]
      assert any(np.array_equal(vals[:, c], got[:, p]) for c in cands), (
          'the reference took a node that is not nearest', p)
    assert np.array_equal(got[:, valid.ravel()], vals[:, valid.ravel()])
    unique[sel] = u.reshape(valid.shape)
    filled[sel] = inv.reshape(valid.shape)
  return unique, filled


def main():
  rng = np.random.default_rng(41)
  cases = []

  def reference(cm, **kw):
    # The reference reshapes a slice's update to the WHOLE map's [z, y, x]
    # (map_utils.py:294), which only works for z == 1: a 2-channel map of several
    # slices that needs a fill raises ValueError there.  Such a map goes through the
    # unmodified function one slice at a time -- what its per-slice loop computes.  Its
    # "no NaN: return" test then sees the slice, not the map, so a slice without NaN
    # must hold no inf either (it would be left alone here and filled there).
    if cm.shape[0] == 3 or cm.shape[1] == 1:
      return rmu.fill_missing(cm.copy(), **kw)
    for z in range(cm.shape[1]):
      assert np.isnan(cm[:, z]).any() or np.isfinite(cm[:, z]).all()
    return np.concatenate([rmu.fill_missing(cm[:, z:z + 1].copy(), **kw)
                           for z in range(cm.shape[1])], axis=1)

  def add(name, cm, extrapolate=True, invalid_to_zero=False):
    out = reference(cm, extrapolate=extrapolate, invalid_to_zero=invalid_to_zero,
                    interpolate_first=False)
    assert out.dtype == cm.dtype and out.shape == cm.shape
    unique, filled = audit(cm, out, extrapolate)
    share = unique.sum() / max(filled.sum(), 1)
    print(f'{name:28s} {cm.shape} filled {int(filled.sum()):5d} unique {int(unique.sum()):5d}'
          f' ({100 * share:.0f} %)')
    assert not filled.any() or share >= MIN_UNIQUE, (name, share)
    cases.append(dict(name=np.array(name), map=cm, extrapolate=np.array(int(extrapolate)),
                      invalid_to_zero=np.array(int(invalid_to_zero)), out=out, unique=unique,
                      filled=filled))

  def field(shape, dtype):
    # distinct values: a filled node names its source
    return rng.uniform(-30.0, 30.0, shape).astype(dtype)

  # 2-D: a rectangle rotated by 0.4 rad with a round hole; slice 1 all NaN, slice 2 whole
  y, x = np.mgrid[:23, :31]
  u = np.cos(0.4) * (x - 15) + np.sin(0.4) * (y - 11)
  v = -np.sin(0.4) * (x - 15) + np.cos(0.4) * (y - 11)
  inside = (np.abs(u) <= 10) & (np.abs(v) <= 6) & ((x - 17) ** 2 + (y - 10) ** 2 > 9)
  rot = field((2, 3, 23, 31), np.float32)
  rot[:, 0][:, ~inside] = NAN
  rot[:, 1] = NAN
  add('rot_rect_f32', rot)
  add('rot_rect_f64', rot.astype(np.float64))
  add('rot_rect_to_zero', rot, invalid_to_zero=True)
  add('rot_rect_zero_only', rot, extrapolate=False, invalid_to_zero=True)
  add('rot_rect_neither', rot, extrapolate=False)

  # 3-D: a sheared ellipsoid
  z, y, x = np.mgrid[:9, :14, :17]
  xs = x - 8 - 0.5 * (y - 6.5)
  ell = ((z - 4) / 3.2) ** 2 + ((y - 6.5) / 4.5) ** 2 + (xs / 5.5) ** 2 <= 1
  cm = field((3, 9, 14, 17), np.float32)
  cm[:, ~ell] = NAN
  add('ellipsoid_f32', cm)

  # 3-D: 5 % random valid nodes
  cm = field((3, 9, 14, 17), np.float32)
  cm[:, rng.uniform(size=(9, 14, 17)) >= 0.05] = NAN
  add('sparse3d_f32', cm)
  add('sparse3d_f64', cm.astype(np.float64))

  # 2-D, sparse, with inf: an inf in either channel makes the node invalid; slice 1
  # is whole but for inf nodes and one NaN
  cm = field((2, 2, 11, 13), np.float32)
  cm[:, 0][:, rng.uniform(size=(11, 13)) >= 0.1] = NAN
  cm[0, 0, 2, 3] = np.inf
  cm[1, 0, 8, 9] = -np.inf
  cm[0, 0, 5, 5] = 1.5                # one channel finite, the other NaN
  cm[0, 1, 4, 6] = np.inf
  cm[1, 1, 0, 0] = -np.inf
  cm[:, 1, 10, 12] = np.inf
  cm[1, 1, 7, 2] = NAN
  add('inf_2d_f32', cm)

  # 3-D of inverse-map shape: a NaN shell around a valid core; one channel of one
  # core node NaN
  cm = field((3, 6, 12, 13), np.float64)
  shell = np.ones((6, 12, 13), bool)
  shell[1:-1, 2:-3, 2:-2] = False
  cm[:, shell] = NAN
  cm[2, 3, 5, 6] = NAN
  add('inverse_map_shell_f64', cm)

  # 3-D without a valid node
  cm = field((3, 2, 3, 4), np.float32)
  cm[0] = NAN
  cm[1, 0, 0, 0] = np.inf
  add('none_valid_3d', cm)
  add('none_valid_3d_to_zero', cm, invalid_to_zero=True)

  arrays = {}
  for i, rec in enumerate(cases):
    for k, val in rec.items():
      arrays[f'c{i:02d}_{k}'] = val
  path = os.path.join(HERE, 'fill_missing.npz')
  # np.savez stamps every member with the time of day; a fixed stamp makes the file
  # regenerate bit for bit
  with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
    for k, val in arrays.items():
      info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
      zf.writestr(info, buf.getvalue())
  print(f'{len(cases)} cases, {os.path.getsize(path)} bytes -> {path}')


if __name__ == '__main__':
  main()
