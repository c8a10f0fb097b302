"""Shared comparison helpers for the parity tests."""
import json
import types

import numpy as np


def check_flow(got, want, sharp_rtol=2e-4, ratio_rtol=1e-4, ratio_atol=1e-6):
  """Flow-field parity: NaN pattern identical, vector components exact,
  sharpness / ratio within float32 tolerance."""
  assert got.shape == want.shape
  assert got.dtype == np.float32
  nd = got.shape[0] - 2
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
  np.testing.assert_array_equal(got[:nd], want[:nd])
  ok = np.isfinite(want[nd]) & np.isfinite(got[nd])
  np.testing.assert_array_equal(np.isfinite(want[nd]), np.isfinite(got[nd]))
  check_sharpness(got[nd][ok], want[nd][ok], rtol=sharp_rtol)
  m = ~np.isnan(want[nd + 1])
  np.testing.assert_allclose(got[nd + 1][m], want[nd + 1][m], rtol=ratio_rtol,
                             atol=ratio_atol)


def check_sharpness(got, want, rtol=2e-4, inv_atol=5e-6, inv_from=100.0):
  """sharpness = peak / min(window) (flow_field.py:188-192).  On raw surfaces the
  window minimum has either sign and may lie next to 0, where the quotient is
  ill conditioned, so SURVEY 8c pins numerator and minimum separately.  From the
  flow field alone that is: every element agrees to `rtol`, OR -- only where the
  quotient IS ill conditioned, |want| >= `inv_from`, i.e. |window minimum| <=
  |peak| / inv_from -- its reciprocal min / peak agrees to `inv_atol`: the window
  minimum agrees to inv_atol x |peak| (SURVEY 8c allows 1e-3 x |peak|; measured
  on the headline field: <= 2e-6).  A sign flip therefore passes only for
  |sharpness| > 1 / inv_atol = 2e5, where the minimum is within 5e-6 x |peak| of
  zero on both sides; 1000 against 1020 does not."""
  got = np.asarray(got, np.float64)
  want = np.asarray(want, np.float64)
  close = np.abs(got - want) <= rtol * np.abs(want)
  with np.errstate(divide='ignore'):
    inv = np.abs(1.0 / got - 1.0 / want)
  ill = (np.abs(want) >= inv_from) & (np.abs(got) >= inv_from)
  bad = ~(close | (ill & (inv <= inv_atol)))
  assert not bad.any(), (
      f'{int(bad.sum())} of {bad.size} sharpness values differ: worst relative '
      f'{np.max(np.abs(got - want)[bad] / np.abs(want[bad])):.3g}, worst |d(1/s)| '
      f'{inv[bad].max():.3g}')
  # (reported for the tolerance log: the reciprocal criterion alone)
  np.testing.assert_allclose(1.0 / got[~close], 1.0 / want[~close], rtol=0, atol=inv_atol)


def cfg_from(d, cls=None):
  d = dict(d)
  d.pop('_force_cap', None)
  d['stride'] = tuple(d['stride'])
  if cls is None:
    return types.SimpleNamespace(**d)
  return cls(**d)


def load_cfgs(npz):
  return json.loads(str(npz['cfgs']))


def mesh_plan(x, prev, config, mesh_force=None):
  """Which integrator sfm_mesh_relax_chunk would run for this velocity_verlet call
  under the switches in effect (sfm_debug_mesh_plan): an _abi.SfmMeshPlanInfo.  Needs
  a GPU (the planner compares with the device's CU count)."""
  import ctypes as C
  import torch
  from sofima_amd import _abi, _dev, mesh
  spec = mesh._resolve_force(mesh_force or mesh.inplane_force)
  dev = _dev.device()
  x_t = _dev.as_device_f32(x, dev, copy=False)
  prev_t = None if prev is None else _dev.as_device_f32(prev, dev, copy=False)
  ws = torch.empty(1, dtype=torch.uint8, device=dev)
  d = mesh._chunk_desc(x_t, x_t, x_t, prev_t, config, spec, ws)   # nothing is dereferenced
  info = _abi.SfmMeshPlanInfo()
  _abi.check(_abi.load().sfm_debug_mesh_plan(C.byref(d), C.byref(info)))
  return info


def em_texture(rng, shape, sigma=2.0):
  """uint8 EM-like texture (low-pass noise stretched to 0..255)."""
  from scipy import ndimage
  img = ndimage.gaussian_filter(rng.standard_normal(shape, dtype=np.float32), sigma)
  img = (img - img.min()) / (img.max() - img.min()) * 255
  return img.astype(np.uint8)


def synth_montage(rng, gx, gy, mesh_shape, overlap, amp=4.0):
  """Synthetic tile montage for the target-mesh `prev_fn`: gx x gy tiles,
  mesh_shape = (y, x) nodes (in-plane) or (z, y, x) (volumetric), flow strips
  `overlap` nodes wide between all adjacent tiles, consistent NeighborInfo rows
  (stitch_elastic.py:43-72).  Returns (nbors, fx, fy, x0)."""
  from scipy import ndimage
  nd = len(mesh_shape)
  n = gx * gy
  my, mx = mesh_shape[-2:]
  lead = tuple(mesh_shape[:-2])
  fz = tuple(max(1, s - 1) for s in lead)

  def smooth(shape, a):
    sig = (0, 0) + (1.0,) * len(lead) + (3.0, 3.0)
    v = ndimage.gaussian_filter(rng.standard_normal(shape), sig)
    return (v / np.abs(v).max() * a).astype(np.float32)

  fx = smooth((nd, n) + fz + (my - 2, overlap), amp)   # x pairs: ortho y, overlap x
  fy = smooth((nd, n) + fz + (overlap, mx - 3), amp)   # y pairs: overlap y, ortho x
  x0 = smooth((nd, n) + tuple(mesh_shape), amp / 2)
  fields = 8 if nd == 2 else 11
  nb = -np.ones((n, 4, fields), np.int32)

  def entry(nbor, flow_idx, dim, flow, off_o, off_z):
    e = -np.ones(fields, np.int32)
    e[0], e[1], e[7] = nbor, flow_idx, dim
    fyy, fxx = flow.shape[-2:]
    e[4] = fxx if dim == 0 else fyy     # flow_size_overlap
    e[3] = fyy if dim == 0 else fxx     # flow_size_ortho
    e[2] = off_o                        # coarse_offset_ortho
    e[5], e[6] = rng.integers(-2, 3, 2)
    if nd == 3:
      e[8], e[9], e[10] = off_z, flow.shape[-3], rng.integers(-2, 3)
    return e

  offs_x = rng.integers(-2, 3, (n, 2))
  offs_y = rng.integers(-2, 3, (n, 2))
  for t in range(n):
    tx, ty = t % gx, t // gx
    k = 0
    if tx > 0:
      nb[t, k] = entry(t - 1, t - 1, 0, fx, *offs_x[t - 1]); k += 1
    if tx < gx - 1:
      nb[t, k] = entry(t + 1, t, 0, fx, *offs_x[t]); k += 1
    if ty > 0:
      nb[t, k] = entry(t - gx, t - gx, 1, fy, *offs_y[t - gx]); k += 1
    if ty < gy - 1:
      nb[t, k] = entry(t + gx, t, 1, fy, *offs_y[t]); k += 1
  return nb, fx, fy, x0


# ---------------------------------------------------------------------------
# The CPU oracle on many reference batches at once: one SPAWNED process per
# batch (no HIP context is inherited), images handed over as memory-mapped .npy
# files.  Test infrastructure only.
# ---------------------------------------------------------------------------
_ORACLE_ARGS = {}


def _oracle_init(paths, kwargs):
  _ORACLE_ARGS['arrays'] = {k: (None if p is None else np.load(p, mmap_mode='r'))
                            for k, p in paths.items()}
  _ORACLE_ARGS['kwargs'] = kwargs


def _oracle_batch(b):
  from oracle import flow_oracle
  a = _ORACLE_ARGS['arrays']
  kw = dict(_ORACLE_ARGS['kwargs'])
  out = flow_oracle.flow_field(np.asarray(a['pre']), np.asarray(a['post']),
                               pre_mask=None if a['pre_mask'] is None else np.asarray(a['pre_mask']),
                               post_mask=None if a['post_mask'] is None else np.asarray(a['post_mask']),
                               only_batches=(b,), **kw)
  flat = out.reshape(out.shape[0], -1)
  bs = kw['batch_size']
  return b, flat[:, b * bs:(b + 1) * bs].copy()


def oracle_flow_batches(tmp_dir, pre, post, patch_size, step, batch_size, batches,
                        pre_mask=None, post_mask=None, procs=None, fft_workers=None,
                        **kwargs):
  """flow_oracle.flow_field on the reference batches `batches` (indices into
  the row-major list of grid positions -- valid when no patch is dropped by a
  mask, which the callers assert), in parallel.  Returns {batch: [dim + 2, n]}."""
  import multiprocessing as mp
  import os
  cores = os.cpu_count() or 1
  procs = procs or max(1, min(len(batches), cores // 4, 24))
  fft_workers = fft_workers or max(1, min(16, cores // procs))
  paths = {}
  for name, arr in (('pre', pre), ('post', post), ('pre_mask', pre_mask),
                    ('post_mask', post_mask)):
    if arr is None:
      paths[name] = None
    else:
      paths[name] = os.path.join(str(tmp_dir), name + '.npy')
      np.save(paths[name], arr)
  kw = dict(patch_size=patch_size, step=step, batch_size=batch_size,
            workers=fft_workers, **kwargs)
  with mp.get_context('spawn').Pool(procs, initializer=_oracle_init,
                                    initargs=(paths, kw)) as pool:
    return dict(pool.imap_unordered(_oracle_batch, list(batches)))


def ndimage_warp_case(g, name):
  """Arguments of one ndimage_warp fixture: (image, map, stride, work, overlap,
  order, boxes or None ({image, map, out}: (start xyz, size xyz)), out_scale or
  None, expected)."""
  stride = g[f'{name}_stride']
  stride = tuple(int(v) for v in stride) if bool(g[f'{name}_stride_is_int']) else tuple(
      float(v) for v in stride)
  boxes = None
  if f'{name}_image_box' in g.files:
    boxes = {k: (g[f'{name}_{k}_box'][0], g[f'{name}_{k}_box'][1])
             for k in ('image', 'map', 'out')}
  scale = tuple(g[f'{name}_out_scale']) if f'{name}_out_scale' in g.files else None
  return (g[f'{name}_image'], g[f'{name}_map'], stride, tuple(g[f'{name}_work']),
          tuple(g[f'{name}_overlap']), int(g[f'{name}_order']), boxes, scale,
          g[f'{name}_warped'])
