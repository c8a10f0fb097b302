"""Generates tests/golden/missing_flow.npz by driving the UNMODIFIED reference
`EstimateMissingFlow.process` (processor/flow.py:624-844) over an in-memory
volume: a subclass supplies `_open_volume`, `_build_mask` and
`_get_mask_configs`, `_refshim` makes the imports resolve, and the stand-in
modules processor/flow.py needs beyond it (`connectomics.common.beam_utils`
counters and timers, `connectomics.volume.metadata`,
`connectomics.volume.subvolume.Subvolume`) are registered here, before the
import.  The reference's constructor assigns to its frozen config when a
selection mask is configured (:589-595), so the selection-mask config is put
into `_config` after construction; `process` itself runs as it is.

Build-container only.  One uint8 EM-like stack [6, 200, 216]; patch 32, search
radius 8, stride 16, batch size 16; the flow box (2, 2, .) + (11, 10, 3) fills
the volume in xy, a grid of 10 x 11 nodes.  Sections share a texture; section 2
is unrelated texture, section 3 carries an unrelated blob, section 5 is shifted
by (2, 3) pixels.
  fwd   delta_z 1, max_delta_z 4, max_attempts 1, sections 3..5: look-back 2 of
        section 4 is rejected and 3 accepted; section 3 runs out of stack
  bwd   delta_z -1, max_delta_z -3, max_attempts 0, sections 0..2, a tissue
        mask (section 3 all True, blobs elsewhere), a selection mask
  clip  four boxes with the correlation replaced by a recorder: three cut by
        the volume's corners / edges, one the reference returns unchanged.
        Boxes and slices only; where the images of a round lie in the volume is
        read off the addresses of the views the reference hands over.
The thresholds (ratio 2.5, sharpness 2.0, magnitude 12.5) lie where the peaks
of related and unrelated texture are sparse, so the margins asserted below
hold; related nodes report their shift plus the search radius (see run_case).
Stored: the stack, masks, per case the config (JSON), box, input flow, the
output, the output box, the geometry the reference used, and `filled`, the
nodes filled per section and look-back (column sums == the stand-in's
`sections-filled-delta*` counters).
Run:
  python tests/golden/make_golden_missing_flow.py
"""
import collections
import contextlib
import dataclasses
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

COUNTERS = collections.Counter()
LOG = []


class _Counter:

  def __init__(self, name):
    self.name = name

  def inc(self, n=1):
    COUNTERS[self.name] += int(n)


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
          counter=lambda namespace, name: _Counter(name),
          timer_counter=lambda namespace, name: contextlib.nullcontext())
_register('connectomics.volume.metadata', VolumeMetadata=type('VolumeMetadata', (), {}),
          DecoratedVolume=type('DecoratedVolume', (), {}))
_register('connectomics.volume.subvolume', Subvolume=_Subvolume)

from connectomics.common import bounding_box  # noqa: E402
from sofima.processor import flow as rflow  # noqa: E402

SEED = 25
Z, Y, X = 6, 200, 216
BASE = dict(patch_size=32, stride=16, search_radius=8, batch_size=16,
            min_peak_ratio=2.5, min_peak_sharpness=2.0, max_magnitude=12.5)
CASES = {
    'fwd': dict(BASE, delta_z=1, max_delta_z=4, max_attempts=1, masked=False, selection=False,
                mask_only_for_patch_selection=False, box=((2, 2, 3), (11, 10, 3))),
    'bwd': dict(BASE, delta_z=-1, max_delta_z=-3, max_attempts=0, masked=True, selection=True,
                mask_only_for_patch_selection=False, box=((2, 2, 0), (11, 10, 3))),
}
CLIP_BOXES = [((0, 0, 1), (6, 5, 2)),      # low corner, stack start
              ((8, 7, 4), (6, 6, 2)),      # high corner
              ((0, 3, 2), (14, 4, 1)),     # both x edges
              ((12, 11, 2), (2, 2, 1))]    # no context left: returned unchanged
REL_MARGIN = 0.01      # 50 x the sharpness / ratio tolerances of tests/util.check_flow
ABS_MARGIN = 1e-3


class _Recorder:
  """Stands in for absl.logging inside processor/flow.py: keeps (format, args)."""

  def info(self, fmt, *args):
    LOG.append((fmt, args))

  warning = error = debug = info


class Volume:
  """What `_open_volume` returns: CZYX data behind `asarray`."""

  def __init__(self, data):
    self._data = data
    self.loaded = []

  def clip_box_to_volume(self, box):
    return box.intersection(bounding_box.BoundingBox(start=(0, 0, 0), size=self.volume_size))

  @property
  def asarray(self):
    vol = self

    class _Indexer:

      def __getitem__(self, key):
        vol.loaded.append(key)
        return vol._data[key]

    return _Indexer()

  @property
  def volume_size(self):
    return (self._data.shape[3], self._data.shape[2], self._data.shape[1])


class Proc(rflow.EstimateMissingFlow):

  def __init__(self, config, volume, mask, selection):
    sel_cfg = config.selection_mask_configs
    super().__init__(dataclasses.replace(config, selection_mask_configs=None))
    self._config = dataclasses.replace(self._config, selection_mask_configs=sel_cfg)
    self.volume, self.mask, self.selection = volume, mask, selection

  def _get_mask_configs(self, configs):
    return configs

  def _open_volume(self, path):
    return self.volume

  def _build_mask(self, mask_configs, box):
    src = self.mask if mask_configs == 'mask' else self.selection
    return src[box.to_slice3d()].copy()


def make_config(spec):
  return rflow.EstimateMissingFlow.Config(
      patch_size=spec['patch_size'], stride=spec['stride'], delta_z=spec['delta_z'],
      max_delta_z=spec['max_delta_z'], max_attempts=spec['max_attempts'],
      mask_configs='mask' if spec.get('masked') else None,
      mask_only_for_patch_selection=spec['mask_only_for_patch_selection'],
      selection_mask_configs='sel' if spec.get('selection') else None,
      min_peak_ratio=spec['min_peak_ratio'], min_peak_sharpness=spec['min_peak_sharpness'],
      max_magnitude=spec['max_magnitude'], batch_size=spec['batch_size'],
      image_volinfo='volume', image_cache_bytes=0, mask_cache_bytes=0,
      search_radius=spec['search_radius'])


def texture(rng, shape, sigma=2.0):
  t = ndimage.gaussian_filter(rng.standard_normal(shape), sigma)
  return t / t.std()


def make_stack(rng):
  base = texture(rng, (Y + 16, X + 16))
  stack = np.zeros((Z, Y, X))
  for z in range(Z):
    dy, dx = (3, 2) if z == 5 else (0, 0)            # section 5 is shifted by (2, 3) in xy
    stack[z] = base[8 + dy:8 + dy + Y, 8 + dx:8 + dx + X] + 0.35 * texture(rng, (Y, X))
  stack[2] = texture(rng, (Y, X))                    # unrelated: its look-backs are rejected
  stack[3, 60:150, 20:110] = texture(rng, (90, 90))  # unrelated blob: a node fails twice
  return np.clip(128 + 40 * stack, 0, 255).astype(np.uint8)


def make_flow(rng, size):
  nx, ny, nz = size
  flow = rng.uniform(-2, 2, size=(2, nz, ny, nx)).astype(np.float32)
  holes = np.zeros((nz, ny, nx), bool)
  holes[:, 1:6, 1:7] = True
  holes[:, 6:9, 7:11] = True
  holes[1, 0, :] = True
  holes &= rng.random((nz, ny, nx)) < 0.9
  flow[:, holes] = np.nan
  return flow


def make_masks(rng):
  mask = np.zeros((Z, Y, X), bool)
  mask[3] = True                                     # an all-True section
  for z in (0, 1, 2, 4, 5):
    for _ in range(3):
      y, x = rng.integers(0, Y - 40), rng.integers(0, X - 40)
      mask[z, y:y + 38, x:x + 40] = True
  selection = np.ones((Z, Y // 16 + 1, X // 16 + 1), bool)   # flow coordinates
  selection[:, 4, :] = False
  selection[1, :, 3] = False
  return mask, selection


def origin(view, data):
  """(z, y, x) in `data` [1, Z, Y, X] of the first element of `view`, a slice of it."""
  offset = (view.__array_interface__['data'][0] - data.__array_interface__['data'][0])
  assert 0 <= offset < data.nbytes and offset % data.itemsize == 0
  return np.array(np.unravel_index(offset // data.itemsize, data.shape[1:]), np.int64)


def run_process(spec, box, flow, data, mask, selection, correlate=True):
  """process() with the correlation call recorded: per round the selection,
  the raw field, and where in the volume the two images it was given lie (they
  are views of the volume).  correlate=False replaces the correlation by an
  all-NaN field of the shape flow_field() gives (flow_field.py:557)."""
  volume = Volume(data)
  proc = Proc(make_config(spec), volume, mask, selection)
  rounds = []
  real = rflow.flow_field.JAXMaskedXCorrWithStatsCalculator.flow_field

  def spy(self, prev, curr, patch_size, step, *args, **kwargs):
    if correlate:
      field = real(self, prev, curr, patch_size, step, *args, **kwargs)
    else:
      grid = (np.array(curr.shape) - (kwargs['post_patch_size'] - step)) // step
      field = np.full([4] + grid.tolist(), np.nan, np.float32)
    rounds.append(dict(sel=kwargs['selection_mask'].copy(), field=field.copy(),
                       prev_origin=origin(prev, data), curr_origin=origin(curr, data),
                       prev_shape=prev.shape, curr_shape=curr.shape))
    return field

  COUNTERS.clear()
  del LOG[:]
  rflow.flow_field.JAXMaskedXCorrWithStatsCalculator.flow_field = spy
  rflow.logging = _Recorder()
  try:
    result = proc.process(_Subvolume(flow.copy(), box))
  finally:
    rflow.flow_field.JAXMaskedXCorrWithStatsCalculator.flow_field = real
  return result, rounds, volume


def geometry_of(box, flow, result, rounds, volume):
  """The geometry the reference used, read off what it loaded, what it handed
  to the correlation and what it returned."""
  key = volume.loaded[-1]
  load_start = np.array([key[3].start, key[2].start, key[1].start], np.int64)
  load_size = np.array([key[3].stop - key[3].start, key[2].stop - key[2].start,
                        key[1].stop - key[1].start], np.int64)
  out_start = np.array(result.bbox.start, np.int64)
  out_size = np.array(result.bbox.size, np.int64)
  # channel 1 of the input is passed through: its first value names the cut
  first = np.argwhere(flow[1] == result.data[1, 0, 0, 0])
  assert len(first) == 1 and first[0][0] == 0
  off = first[0][:0:-1]                                # (x, y)
  assert np.array_equal(out_start[:2] - np.array(box.start)[:2], off)
  r = rounds[0]
  assert np.array_equal(r['prev_origin'][1:], load_start[1::-1])
  assert tuple(r['prev_shape']) == (load_size[1], load_size[0])
  rel = r['curr_origin'][1:] - load_start[1::-1]       # (y, x)
  return dict(out_start=out_start, out_size=out_size,
              flow_slice=np.array([[off[1], off[1] + out_size[1]], [off[0], off[0] + out_size[0]]]),
              load_start=load_start, load_size=load_size,
              curr_slice=np.array([[rel[0], rel[0] + r['curr_shape'][0]],
                                   [rel[1], rel[1] + r['curr_shape'][1]]]),
              z0=np.int64(out_start[2] - load_start[2]))


def run_case(name, spec, stack, mask, selection, rng):
  (start, size) = spec['box']
  box = bounding_box.BoundingBox(start=start, size=size)
  flow = make_flow(rng, size)
  result, rounds, volume = run_process(spec, box, flow, stack[None], mask, selection)
  ret = np.asarray(result.data)
  out_box = result.bbox
  assert ret.shape[1:] == flow.shape[1:], 'the flow cases are not meant to be clipped'
  assert np.array_equal(ret.astype(np.float32).astype(np.float64), ret, equal_nan=True)

  deltas = (list(range(spec['delta_z'] + 1, spec['max_delta_z'] + 1)) if spec['delta_z'] > 0
            else list(range(spec['delta_z'] - 1, spec['max_delta_z'] - 1, -1)))
  was_nan = np.isnan(flow[0])
  filled = np.array([[np.sum(was_nan[z] & (ret[2, z] == dz)) for dz in deltas]
                     for z in range(flow.shape[1])], np.int64)
  for k, dz in enumerate(deltas):
    assert filled[:, k].sum() == COUNTERS[f'sections-filled-delta{dz}'], (name, dz)

  # ---- the case exercises what it claims (on the reference alone) ----
  # walk the log: sections, look-backs tried, rounds that reached the correlation
  seen = dict(masked_prev=0, stack_break=0, cap_drop=0)
  z = None
  tried = {}
  evaluated = {}
  remaining = None     # nodes left in the mask after the last round of the section

  def close_try():
    # a look-back that was tried, not masked, and did not reach the correlation:
    # the cap emptied the mask (:785-787)
    nonlocal remaining
    if z is None or not tried[z] or tried[z][-1] in evaluated[z]:
      return
    if spec['masked'] and mask[start[2] + z - tried[z][-1]].all():
      return
    if remaining:
      seen['cap_drop'] += remaining
      remaining = 0

  for fmt, args in LOG:
    if fmt.startswith('Processing rel_z'):
      close_try()
      z = args[0]
      tried[z], evaluated[z] = [], []
      remaining = None
    elif fmt.startswith('Trying delta_z'):
      close_try()
      tried[z].append(args[0])
    elif fmt.startswith('.. points to evaluate'):
      evaluated[z].append(tried[z][-1])
      if remaining is not None:
        seen['cap_drop'] += remaining - int(args[0])     # the mask only shrinks
      remaining = int(args[0])
    elif fmt.startswith('.. points to update'):
      remaining -= int(args[0])
  close_try()
  by_section = collections.defaultdict(list)
  it = iter(rounds)
  for z in sorted(evaluated):
    for dz in evaluated[z]:
      by_section[z].append((dz, next(it)))
  assert next(it, None) is None
  for z, dzs in tried.items():
    abs_z = start[2] + z
    for dz in dzs:
      if spec['masked'] and mask[abs_z - dz].all():
        assert dz not in evaluated[z]
        seen['masked_prev'] += 1
    if len(dzs) < len(deltas) and was_nan[z].any() and dzs and dzs[-1] in evaluated[z]:
      nxt = abs_z - deltas[len(dzs)]
      if nxt < 0 or nxt >= Z:
        seen['stack_break'] += 1
  thr = spec
  for z, rs in by_section.items():
    for dz, r in rs:
      sel, field = r['sel'], r['field']
      assert r['curr_origin'][0] == start[2] + z and r['prev_origin'][0] == start[2] + z - dz
      valid = np.isfinite(field[0]) & sel
      sharp, ratio = np.abs(field[2][valid]), np.abs(field[3][valid])
      assert np.all(np.abs(sharp / thr['min_peak_sharpness'] - 1) >= REL_MARGIN), (name, z, dz)
      assert np.all(np.abs(ratio[ratio > 0] / thr['min_peak_ratio'] - 1) >= REL_MARGIN), (name, z, dz)
      comps = np.abs(field[:2][:, valid])
      assert np.all(np.abs(comps - thr['max_magnitude']) >= ABS_MARGIN), (name, z, dz)
  accepted = sorted(dz for k, dz in enumerate(deltas) if filled[:, k].sum() > 0)
  print(name, 'filled', filled.tolist(), 'seen', seen, 'still NaN',
        int(np.isnan(ret[0]).sum()), 'rounds', len(rounds))
  assert len(accepted) >= 2, accepted
  assert np.isnan(ret[0]).any()
  if name == 'fwd':
    assert seen['cap_drop'] >= 1 and seen['stack_break'] >= 1, seen
    rejected_then_accepted = filled[1, deltas.index(3)] > 0      # section 4: 2 rejected, 3 taken
    assert rejected_then_accepted
    shift = ret[:2, 2][:, was_nan[2] & (ret[2, 2] == 2)]
    # section 5 shows what section 3 shows at (y + 3, x + 2): a flow of (2, 3), which the
    # reference reports search_radius larger -- flow_field() starts the previous patch
    # (patch - post_patch) // 2 before the current one (flow_field.py:604-623) although
    # the previous image already begins search_radius earlier (:733-737, :792-803)
    expected = np.array([2.0, 3.0]) + spec['search_radius']
    assert shift.size and np.all(np.abs(np.median(shift, axis=1) - expected) < 0.5), shift
  else:
    assert seen['masked_prev'] >= 1, seen

  geo = geometry_of(box, flow, result, rounds, volume)
  out = {name + '_cfg': np.array(json.dumps({k: v for k, v in spec.items() if k != 'box'})),
         name + '_box': np.array(spec['box'], np.int64), name + '_flow': flow,
         name + '_out': ret.astype(np.float32), name + '_filled': filled,
         name + '_out_box': np.array([out_box.start, out_box.size], np.int64)}
  out.update({f'{name}_geo_{k}': v for k, v in geo.items()})
  return out


def run_clip(spec):
  """The boxes the reference derives for CLIP_BOXES: every flow vector is
  missing, channel 1 of the input numbers its entries, the correlation is
  replaced by the recorder."""
  data = np.zeros((1, Z, Y, X), np.uint8)
  out = {'clip_boxes': np.array(CLIP_BOXES, np.int64),
         'clip_cfg': np.array(json.dumps({k: v for k, v in spec.items() if k != 'box'}))}
  unchanged = []
  for i, (start, size) in enumerate(CLIP_BOXES):
    box = bounding_box.BoundingBox(start=start, size=size)
    flow = np.full((2, size[2], size[1], size[0]), np.nan, np.float32)
    flow[1] = np.arange(flow[1].size, dtype=np.float32).reshape(flow[1].shape)
    result, rounds, volume = run_process(spec, box, flow, data, None, None, correlate=False)
    same = result.data.shape == flow.shape and result.data.shape[0] == 2
    unchanged.append(same)
    if same:
      assert not rounds and np.array_equal(result.data, flow, equal_nan=True)
      continue
    geo = geometry_of(box, flow, result, rounds, volume)
    assert np.any(geo['out_size'] != np.array(size)), 'the box is meant to be cut'
    out.update({f'clip{i}_geo_{k}': v for k, v in geo.items()})
    print('clip', i, {k: v.tolist() for k, v in geo.items()})
  assert unchanged == [False, False, False, True], unchanged
  out['clip_unchanged'] = np.array(unchanged)
  return out


def main():
  rng = np.random.default_rng(SEED)
  stack = make_stack(rng)
  mask, selection = make_masks(rng)
  arrays = dict(images=stack, mask=mask, selection=selection, cases=np.array(list(CASES)))
  for name, spec in CASES.items():
    arrays.update(run_case(name, spec, stack, mask if spec['masked'] else None,
                           selection if spec['selection'] else None, rng))
  arrays.update(run_clip(CASES['fwd']))
  path = os.path.join(HERE, 'missing_flow.npz')
  np.savez_compressed(path, **arrays)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()
