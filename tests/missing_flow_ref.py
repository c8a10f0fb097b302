"""NumPy restatements and fixture access shared by the missing-flow tests
(tests/golden/missing_flow.npz, written by tests/golden/make_golden_missing_flow.py):
the box arithmetic and the section / look-back loop of `EstimateMissingFlow`
(processor/flow.py:634-828) and the pair loop of `EstimateFlow` (:184-231),
with the flow function as a parameter.  Test infrastructure only."""
import json

import numpy as np

GEOMETRY_KEYS = ('patch_size', 'stride', 'search_radius', 'delta_z', 'max_delta_z')


def config(z, name):
  """The configuration of a golden case ('fwd', 'bwd', 'clip')."""
  return json.loads(str(z[name + '_cfg']))


def _clip(start, size, vol):
  lo, hi = np.maximum(start, 0), np.minimum(start + size, vol)
  return None if np.any(hi <= lo) else (lo, hi - lo)


def geometry_np(box_start, box_size, volume_size, *, patch_size, stride, search_radius,
                delta_z, max_delta_z):
  """processor/flow.py:634-737 -> dict of int arrays (xyz boxes; slices as
  [[y0, y1], [x0, x1]]), or None where the reference returns its input."""
  start, size, vol = (np.asarray(v, dtype=np.int64) for v in (box_start, box_size, volume_size))
  sps = patch_size + 2 * search_radius
  full_start = np.array([start[0] * stride - sps // 2, start[1] * stride - sps // 2, start[2]])
  full_size = np.array([(size[0] - 1) * stride + sps, (size[1] - 1) * stride + sps, 1])
  prev_start, prev_size = _clip(full_start, full_size, vol)
  if np.any(prev_size[:2] <= sps):
    return None
  off = (prev_start - full_start) // stride
  out_start, out_end = start + off, start + size
  out_end = out_end - -(((prev_start + prev_size) - (full_start + full_size)) // stride)
  out_size = out_end - out_start
  curr_start, curr_size = _clip(
      np.array([out_start[0] * stride - patch_size // 2, out_start[1] * stride - patch_size // 2,
                out_start[2]]),
      np.array([(out_size[0] - 1) * stride + patch_size, (out_size[1] - 1) * stride + patch_size,
                size[2]]), vol)
  if delta_z > 0:
    z_lo, z_hi = out_start[2] - max_delta_z, out_end[2]
  else:
    z_lo, z_hi = out_start[2], out_end[2] - max_delta_z
  load_start, load_size = _clip(np.array([prev_start[0], prev_start[1], z_lo]),
                                np.array([prev_size[0], prev_size[1], z_hi - z_lo]), vol)
  rel = curr_start - load_start
  return dict(
      out_start=out_start, out_size=out_size,
      flow_slice=np.array([[off[1], off[1] + out_size[1]], [off[0], off[0] + out_size[0]]]),
      load_start=load_start, load_size=load_size,
      curr_slice=np.array([[rel[1], rel[1] + curr_size[1]], [rel[0], rel[0] + curr_size[0]]]),
      z0=np.int64(out_start[2] - load_start[2]))


def geometry_as_dict(g):
  """A `processor_flow.MissingFlowGeometry` in the layout of `geometry_np`."""
  sl = lambda pair: np.array([[s.start, s.stop] for s in pair], dtype=np.int64)
  return dict(out_start=np.array(g.out_start), out_size=np.array(g.out_size),
              flow_slice=sl(g.flow_slice), load_start=np.array(g.load_start),
              load_size=np.array(g.load_size), curr_slice=sl(g.curr_slice), z0=np.int64(g.z0))


def search_deltas(delta_z, max_delta_z):
  if delta_z > 0:
    return list(range(delta_z + 1, max_delta_z + 1))
  return list(range(delta_z - 1, max_delta_z - 1, -1))


def clean_np(flow, min_peak_ratio, min_peak_sharpness, max_magnitude):
  """flow_utils.clean_flow (flow_utils.py:37-78) with max_deviation = 0 on a
  [4, y, x] field -> [2, y, x]."""
  with np.errstate(invalid='ignore'):
    bad = np.abs(flow[2]) < min_peak_sharpness
    ratio = np.abs(flow[3])
    bad |= (ratio > 0.0) & (ratio < min_peak_ratio)
    if max_magnitude > 0:
      bad |= np.max(np.abs(flow[:2]), axis=0) > max_magnitude
  ret = flow[:2].copy()
  ret[:, bad] = np.nan
  return ret


def update_np(field, planes, mask, attempts, *, min_peak_ratio, min_peak_sharpness,
              max_magnitude, delta_z, max_attempts):
  """processor/flow.py:806-828 and the cap of the next round (:785), in place
  on planes [3, ny, nx], mask (bool) and attempts; returns the nodes filled."""
  valid = np.isfinite(field[0])
  sy, sx = valid.shape
  attempts[:sy, :sx][valid] += 1
  clean = clean_np(field, min_peak_ratio, min_peak_sharpness, max_magnitude)
  to_update = mask[:sy, :sx] & np.isfinite(clean[0])
  mask[:sy, :sx][to_update] = False
  planes[2, :sy, :sx][to_update] = delta_z
  planes[0, :sy, :sx][to_update] = clean[0][to_update]
  planes[1, :sy, :sx][to_update] = clean[1][to_update]
  mask &= attempts <= max_attempts
  return int(np.sum(to_update))


def estimate_missing_flow_np(flow, images, flow_fn, *, patch_size, stride, delta_z,
                             max_delta_z, max_attempts, search_radius, min_peak_ratio,
                             min_peak_sharpness, max_magnitude, curr_slice=None, z0=None,
                             masks=None, mask_only_for_patch_selection=False,
                             selection_mask=None, batch_size=1024, trace=None):
  """The loop of processor/flow.py:666-828.  flow_fn(prev, curr, patch, stride,
  prev_mask, curr_mask, mask_only_for_patch_selection=, selection_mask=,
  batch_size=, post_patch_size=) -> [4, gy, gx].  Returns (ret [3, nz, ny, nx]
  float32, filled int64 [nz, n_search_deltas]).  `trace`, a list, receives
  (z, delta_z, event) for 'masked-prev', 'break-stack' and 'break-empty'."""
  nz, ny, nx = flow.shape[1:]
  sps = patch_size + 2 * search_radius
  if curr_slice is None:
    curr_slice = tuple(slice(search_radius, search_radius + (n - 1) * stride + patch_size)
                       for n in (ny, nx))
  if z0 is None:
    z0 = max_delta_z if delta_z > 0 else 0
  ret = np.zeros((3, nz, ny, nx))
  ret[:2] = flow
  ret[2] = delta_z
  invalid = np.isnan(flow[0])
  deltas = search_deltas(delta_z, max_delta_z)
  filled = np.zeros((nz, len(deltas)), np.int64)
  for z in range(nz):
    if np.all(~invalid[z]):
      continue
    ci = z0 + z
    assert 0 <= ci < images.shape[0]
    curr_mask = None
    if masks is not None:
      curr_mask = masks[ci][curr_slice]
      if np.all(curr_mask):
        continue
    attempts = np.zeros((ny, nx), dtype=int)
    mask = ~np.isfinite(ret[0, z])
    if selection_mask is not None:
      mask &= selection_mask[z].astype(bool)
    curr = images[ci][curr_slice]
    for k, dz in enumerate(deltas):
      pi = ci - dz
      if pi < 0 or pi >= images.shape[0]:
        if trace is not None:
          trace.append((z, dz, 'break-stack'))
        break
      prev_mask = None
      if masks is not None:
        prev_mask = masks[pi]
        if np.all(prev_mask):
          if trace is not None:
            trace.append((z, dz, 'masked-prev'))
          continue
      mask &= attempts <= max_attempts
      if not np.any(mask):
        if trace is not None:
          trace.append((z, dz, 'break-empty'))
        break
      field = flow_fn(images[pi], curr, sps, stride, prev_mask, curr_mask,
                      mask_only_for_patch_selection=mask_only_for_patch_selection,
                      selection_mask=mask, batch_size=batch_size, post_patch_size=patch_size)
      planes = ret[:, z]
      filled[z, k] = update_np(np.asarray(field), planes, mask, attempts,
                               min_peak_ratio=min_peak_ratio,
                               min_peak_sharpness=min_peak_sharpness,
                               max_magnitude=max_magnitude, delta_z=dz,
                               max_attempts=np.iinfo(np.int64).max)   # the cap runs above
  return ret.astype(np.float32), filled


def flow_pairs_np(nz, z_stride, fixed_current):
  """processor/flow.py:213-229."""
  if fixed_current:
    return [(z, nz - 1) for z in range(0, nz - 1)] if z_stride > 0 else \
        [(z, 0) for z in range(1, nz)]
  rng = range(0, nz - z_stride) if z_stride > 0 else range(-z_stride, nz)
  return [(z, z + z_stride) for z in rng]


def case_kwargs(z, cfg, name):
  """The keyword arguments of one golden flow case for estimate_missing_flow /
  estimate_missing_flow_np, and its (flow, images)."""
  geo = {k[len(name) + 5:]: z[k] for k in z.files if k.startswith(name + '_geo_')}
  flow = z[name + '_flow'][:, :, geo['flow_slice'][0, 0]:geo['flow_slice'][0, 1],
                           geo['flow_slice'][1, 0]:geo['flow_slice'][1, 1]]
  lo, size = geo['load_start'], geo['load_size']
  box = (slice(lo[2], lo[2] + size[2]), slice(lo[1], lo[1] + size[1]),
         slice(lo[0], lo[0] + size[0]))
  kw = {k: cfg[k] for k in ('patch_size', 'stride', 'delta_z', 'max_delta_z', 'max_attempts',
                            'search_radius', 'min_peak_ratio', 'min_peak_sharpness',
                            'max_magnitude', 'batch_size', 'mask_only_for_patch_selection')}
  kw['curr_slice'] = tuple(slice(int(a), int(b)) for a, b in geo['curr_slice'])
  kw['z0'] = int(geo['z0'])
  if cfg['masked']:
    kw['masks'] = np.ascontiguousarray(z['mask'][box])
  if cfg['selection']:                        # stored for the volume, in flow coordinates
    o, s = geo['out_start'], geo['out_size']
    kw['selection_mask'] = np.ascontiguousarray(
        z['selection'][o[2]:o[2] + s[2], o[1]:o[1] + s[1], o[0]:o[0] + s[0]])
  return np.ascontiguousarray(flow), np.ascontiguousarray(z['images'][box]), kw
