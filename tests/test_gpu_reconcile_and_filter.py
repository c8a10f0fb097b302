"""processor_flow.reconcile_and_filter_flows on the device: goldens of the
unmodified `ReconcileAndFilterFlows.process` whose coarse flows are affine (one
answer whatever the triangulation), and generic coarse flows against a host
restatement of the steps around the upsampling that takes the device's own
`resample_map` output, so everything but the triangulation is checked exactly.
"""
import json
import os

import numpy as np
import pytest
from scipy import ndimage

from sofima_amd import map_utils, processor_flow as pf
from sofima_amd._dev import DeviceArray
from tests import resample_map_scipy as rms
from tests.test_reconcile import reconcile_restated

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'reconcile_filter.npz')
CLEAN = ('min_peak_ratio', 'min_peak_sharpness', 'max_magnitude', 'max_deviation')


def golden_case(name):
  g = np.load(GOLDEN)
  cfg = json.loads(str(g[f'{name}_config']))
  scale, divisor = (float(v) for v in g[f'{name}_scale'])
  mask = g[f'{name}_mask']
  return dict(cfg=cfg, box=rms.box(*g[f'{name}_box']), base=g[f'{name}_base'],
              coarse=g[f'{name}_coarse'], read_box=rms.box(*g[f'{name}_read_box']),
              scale=scale, divisor=None if np.isnan(divisor) else divisor,
              mask=mask if mask.size else None, out=g[f'{name}_out'])


def run(c, cfg=None, **over):
  cfg = dict(cfg or c['cfg'], **over)
  return pf.reconcile_and_filter_flows(
      c['base'], c['box'], [pf.CoarseFlow(c['coarse'], c['read_box'], c['scale'], c['divisor'])],
      mask=c['mask'], **cfg)


@pytest.mark.parametrize('name', ['affine', 'multi', 'clipped'])
def test_golden_process(name):
  """The NaN pattern is the reference's exactly.  A vector is the base flow's,
  copied bit for bit, or an upsampled one.  The coarse vectors are exactly
  affine in float32 (coefficients that are multiples of 1/64), so every
  triangulation interpolates the same value and the reference's output is the
  one answer: every vector lies within one float32 ulp of it."""
  c = golden_case(name)
  got = run(c)
  assert isinstance(got, DeviceArray)
  got, want = np.asarray(got), c['out']
  assert got.dtype == np.float32 and got.shape == want.shape
  assert want.shape[0] == (3 if c['cfg']['multi_section'] else 2)
  assert np.array_equal(np.isnan(got), np.isnan(want))
  ok = ~np.isnan(want)
  filled = np.isnan(c['base'][0]) & ~np.isnan(want[0])
  assert filled.sum() > 50, 'the coarse flow fills nothing'
  g, w = got[:2][ok[:2]], want[:2][ok[:2]]
  print(f'{name}: {int((g != w).sum())} of {g.size} vector components differ from the reference')
  assert np.all(np.abs(g - w) <= np.spacing(np.abs(w)))
  kept = ~np.isnan(c['base'][0]) & ok[0]
  assert np.array_equal(got[:2][:, kept], want[:2][:, kept])
  if want.shape[0] == 3:
    assert np.array_equal(got[2][ok[2]], want[2][ok[2]])
  if name == 'clipped':
    # fine nodes beyond the last coarse node took nothing from the coarse flow
    hi_x = (c['read_box'].start[0] + c['read_box'].size[0] - 1) / c['scale']
    beyond = (np.arange(c['box'].size[0]) + c['box'].start[0]) > hi_x
    assert beyond.any() and not (~np.isnan(got[0]) & np.isnan(c['base'][0]))[:, :, beyond].any()


def clean_restated(flow, min_peak_ratio, min_peak_sharpness, max_magnitude, max_deviation):
  """flow_utils.clean_flow (flow_utils.py:37-78) for c = 2 .. 4, from its contract."""
  flow = np.asarray(flow, np.float32)
  with np.errstate(invalid='ignore'):
    if flow.shape[0] == 4:
      ret = flow[:2].copy()
      pr = np.abs(flow[3])
      bad = (np.abs(flow[2]) < min_peak_sharpness) | ((pr > 0) & (pr < min_peak_ratio))
    else:
      ret = flow.copy()
      bad = np.zeros(flow.shape[1:], bool)
    if max_magnitude > 0:
      bad |= np.max(np.abs(flow[:2]), axis=0) > max_magnitude
    if max_deviation > 0:
      med = ndimage.median_filter(np.nan_to_num(flow[:2]), size=(1, 1, 3, 3))
      bad |= np.max(np.abs(med - flow[:2]), axis=0) > max_deviation
  ret[:, bad] = np.nan
  return ret


def restated(c, cfg):
  """Steps 1 to 4 on the host, with the device's resample_map at step 3."""
  from scipy import interpolate
  thr = [cfg[k] for k in CLEAN]
  channels = 3 if cfg['multi_section'] else 2
  base = clean_restated(c['base'], *thr)
  if cfg['multi_section'] and base.shape[0] != 3:
    third = np.full(base.shape[1:], np.nan, np.float32)
    third[np.isfinite(base[0])] = cfg['base_delta_z']
    base = np.concatenate([base, third[None]])
  coarse = clean_restated(c['coarse'], *thr)
  box, rb, scale = c['box'], c['read_box'], c['scale']
  up = np.asarray(map_utils.resample_map(np.ascontiguousarray(coarse[:2]), rb, box, 1 / scale, 1))
  assert up.dtype == np.float32
  hires = np.zeros_like(base)
  hires[:2] = up / np.float32(scale if c['divisor'] is None else c['divisor'])
  oy = (np.arange(rb.size[1]) + rb.start[1]) / scale
  ox = (np.arange(rb.size[0]) + rb.start[0]) / scale
  qy, qx = np.mgrid[:box.size[1], :box.size[0]]
  qy, qx = qy + box.start[1], qx + box.start[0]
  for z in range(base.shape[1]):
    near = lambda plane: interpolate.RegularGridInterpolator(
        (oy, ox), plane, method='nearest', bounds_error=False)((qy, qx))
    hires[:2, z][:, np.isnan(near(coarse[0, z]))] = np.nan
    for ch in range(2, channels):
      hires[ch, z] = near(coarse[ch, z]).astype(np.float32)
  if c['mask'] is not None:
    hires[:, np.broadcast_to(c['mask'], hires.shape[1:])] = np.nan
  return reconcile_restated([base, hires], cfg['max_gradient'], cfg['max_deviation'],
                            cfg['min_patch_size'])


def generic_case(seed, base_channels, coarse_channels, read_box, mask=False):
  rng = np.random.default_rng(seed)
  box = rms.box((10, 6, 0), (28, 24, 2))
  z, y, x = 2, 24, 28
  cz, cy, cx = 2, read_box.size[1], read_box.size[0]

  def smooth(shape, sigma):
    f = ndimage.gaussian_filter(rng.standard_normal(shape), (0, 0, sigma, sigma))
    return (f / np.abs(f).max()).astype(np.float32)

  def holes(shape, frac):
    noise = ndimage.gaussian_filter(rng.standard_normal(shape), (0, 1.2, 1.2))
    return noise > np.quantile(noise, 1 - frac)

  def peaks(flow):
    if flow.shape[0] == 4:
      flow[2:] = rng.uniform(0.5, 4.0, (2,) + flow.shape[1:])     # some below 1.5
    if flow.shape[0] == 3:
      flow[2] = rng.integers(1, 4, flow.shape[1:])
    return flow

  base = np.zeros((base_channels, z, y, x), np.float32)
  base[:2] = 3 * smooth((2, z, y, x), 3)
  base = peaks(base)
  base[:, holes((z, y, x), 0.3)] = np.nan
  coarse = np.zeros((coarse_channels, cz, cy, cx), np.float32)
  coarse[:2] = 3 * smooth((2, cz, cy, cx), 2)
  coarse = peaks(coarse)
  coarse[:, holes((cz, cy, cx), 0.12)] = np.nan
  m = None
  if mask:
    m = np.zeros((z, y, x), bool)
    m[0, 4:12, 6:20] = True
    m[1, :, 22:] = True
  return dict(box=box, base=base, coarse=coarse, read_box=read_box, scale=0.5, divisor=None,
              mask=m)


CFG = dict(min_peak_ratio=1.5, min_peak_sharpness=1.5, max_magnitude=2.5, max_deviation=0.8,
           max_gradient=0.6, min_patch_size=5, multi_section=False, base_delta_z=0)
FULL = rms.box((4, 2, 0), (16, 14, 2))          # covers the box (x 10 .. 37, y 6 .. 29) at 0.5
CLIPPED = rms.box((6, 2, 0), (10, 11, 2))       # x 12 .. 30, y 4 .. 24: ends inside the box


@pytest.mark.parametrize('name,case,cfg', [
    ('generic', generic_case(1, 4, 4, FULL), CFG),
    ('multi_section', generic_case(2, 2, 3, FULL), dict(CFG, multi_section=True, base_delta_z=2)),
    ('multi_section_base3', generic_case(3, 3, 3, FULL),
     dict(CFG, multi_section=True, base_delta_z=2)),
    ('mask', generic_case(4, 4, 4, FULL, mask=True), CFG),
    ('clipped', generic_case(5, 4, 2, CLIPPED), CFG),
    ('divisor', dict(generic_case(6, 2, 2, FULL), divisor=0.7), CFG),    # not exact in binary
], ids=['generic', 'multi_section', 'multi_section_base3', 'mask', 'clipped', 'divisor'])
def test_generic_flows_against_the_restatement(name, case, cfg):
  got = np.asarray(run(case, cfg))
  want = restated(case, cfg)
  assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
  assert np.array_equal(got, want, equal_nan=True)
  # every filter took part, and the coarse flow filled base holes
  filled = np.isnan(case['base'][0]) & ~np.isnan(want[0])
  assert filled.sum() > 20
  if name == 'mask':
    assert not filled[case['mask']].any() and (~np.isnan(want[0]))[case['mask']].any()
  if name == 'clipped':
    assert np.array_equal(np.isnan(got[0][:, :, 22:]), np.isnan(want[0][:, :, 22:]))


def test_inputs_stay_and_device_arrays_go_in():
  import torch
  c = generic_case(7, 4, 4, FULL, mask=True)
  want = np.asarray(run(c, CFG))
  d = dict(c, base=DeviceArray(torch.from_numpy(c['base']).cuda()),
           coarse=torch.from_numpy(c['coarse']).cuda(), mask=torch.from_numpy(c['mask']).cuda())
  got = np.asarray(run(d, CFG))
  assert np.array_equal(got, want, equal_nan=True)
  assert np.array_equal(np.asarray(d['base']), c['base'], equal_nan=True)
  assert np.array_equal(d['coarse'].cpu().numpy(), c['coarse'], equal_nan=True)


def test_rejections():
  c = generic_case(8, 2, 2, FULL)
  with pytest.raises(ValueError, match='scale'):
    run(dict(c, scale=2.0), CFG)
  with pytest.raises(ValueError, match='read box'):
    run(dict(c, read_box=rms.box((4, 2, 0), (15, 14, 2))), CFG)
  with pytest.raises(ValueError, match='channel 2'):
    run(c, dict(CFG, multi_section=True))
