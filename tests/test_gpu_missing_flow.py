"""processor_flow on the device: the selection / compaction kernel against
np.where, the accept / update kernel against a NumPy restatement of
processor/flow.py:785-828, estimate_missing_flow against what the reference's
EstimateMissingFlow.process produced (tests/golden/missing_flow.npz) and
against the restated loop driven by this package's flow_field(), and
estimate_flow against single flow_field() calls."""
import numpy as np
import pytest

from tests import missing_flow_ref as ref

pytestmark = pytest.mark.gpu

CASES = ('fwd', 'bwd')
SELECT_GRIDS = [(1, 1), (1, 65), (1, 1024), (1, 1025), (3, 1025), (130, 3), (45, 47)]
UPDATE_SHAPES = [(1, 1), (1, 65), (130, 3), (19, 70)]


@pytest.fixture(scope='module')
def fixture(golden):
  return golden('missing_flow')


# ---------------------------------------------------------------------------
# sfm_flow_select
# ---------------------------------------------------------------------------
def _select_np(sel, batch, counts=()):
  """flow_field.py:570-589, :607, :614-618."""
  keep = sel.astype(bool).copy()
  for plane, area, max_masked in counts:
    keep[(plane / area >= max_masked)[:keep.shape[0], :keep.shape[1]]] = False
  pos = np.array(np.where(keep)).T.reshape(-1, 2)
  n = len(pos)
  total = -(-n // batch) * batch
  if n:
    pos = np.concatenate([pos, np.repeat(pos[-1:], total - n, axis=0)])
  return pos.astype(np.int32), n, total


def _select_gpu(gpu, sel, batch, pre=None, post=None, sel_pad=0, pad=(0, 0), max_masked=0.75):
  """sel: [ny, nx] uint8; pre / post: (counts, area) or None.  The planes live
  in wider allocations (`sel_pad`, `pad` extra rows / columns) and are passed as
  views, so every pitch differs from its width."""
  import torch
  from sofima_amd import processor_flow
  ny, nx = sel.shape
  wide = torch.full((ny, nx + sel_pad), 1, dtype=torch.uint8, device=gpu)
  wide[:, :nx] = torch.from_numpy(sel).to(gpu)
  kw = {}
  for side, given in (('pre', pre), ('post', post)):
    if given is None:
      continue
    plane, area = given
    store = torch.zeros((plane.shape[0] + pad[0], plane.shape[1] + pad[1]), dtype=torch.int32,
                        device=gpu)
    store[:plane.shape[0], :plane.shape[1]] = torch.from_numpy(plane).to(gpu)
    kw[side + '_counts'] = store[:plane.shape[0], :plane.shape[1]]
    kw[side + '_area'] = area
  capacity = -(-ny * nx // batch) * batch
  positions = torch.full((capacity, 2), -7, dtype=torch.int32, device=gpu)
  counts = torch.full((2,), -7, dtype=torch.int32, device=gpu)
  processor_flow.select_patches(wide[:, :nx], batch, positions, counts, max_masked=max_masked,
                                **kw)
  n, total = (int(v) for v in counts.cpu().numpy())
  return positions.cpu().numpy(), n, total


def _check_select(got, want):
  (pos, n, total), (want_pos, want_n, want_total) = got, want
  assert (n, total) == (want_n, want_total)
  assert np.array_equal(pos[:total], want_pos)
  assert np.all(pos[total:] == -7)               # nothing written past the padding


@pytest.mark.parametrize('density', [0.0, 1.0, 0.03])
@pytest.mark.parametrize('grid', SELECT_GRIDS)
def test_flow_select_equals_np_where(gpu, grid, density):
  rng = np.random.default_rng(grid[0] * 7919 + grid[1])
  sel = (rng.random(grid) < density).astype(np.uint8) * rng.integers(1, 255, grid).astype(np.uint8)
  if density == 0.03:
    sel[-1, -1] = 1                                # the last linear index takes part
  for batch in (1, 7, 64):
    _check_select(_select_gpu(gpu, sel, batch, sel_pad=5), _select_np(sel, batch))


@pytest.mark.parametrize('batch', [7, 64])
@pytest.mark.parametrize('extra', [0, 1])
def test_flow_select_whole_batches_and_one_more(gpu, batch, extra):
  rng = np.random.default_rng(batch + extra)
  sel = np.zeros(45 * 47, np.uint8)
  sel[rng.choice(sel.size, 2 * batch + extra, replace=False)] = 1
  got = _select_gpu(gpu, sel.reshape(45, 47), batch, sel_pad=3)
  assert got[1:] == (2 * batch + extra, (2 + extra) * batch)
  _check_select(got, _select_np(sel.reshape(45, 47), batch))


@pytest.mark.parametrize('grid', [(1, 65), (3, 1025), (45, 47)])
def test_flow_select_with_masked_counts(gpu, grid):
  """Pre counts on a larger grid with their own pitch, post counts on the grid
  itself; count / area == max_masked exactly is dropped, one below is kept."""
  rng = np.random.default_rng(grid[1])
  ny, nx = grid
  sel = (rng.random(grid) < 0.6).astype(np.uint8)
  pre = rng.integers(0, 17, (ny + 2, nx + 4)).astype(np.int32)       # area 16: 12 / 16 == 0.75
  post = rng.integers(0, 2305, grid).astype(np.int32)                # area 48 * 48
  sel[0, 0], pre[0, 0], post[0, 0] = 1, 12, 0                        # at the limit: dropped
  if nx > 1:
    sel[0, 1], pre[0, 1], post[0, 1] = 1, 11, 1727                   # both one below: kept
  counts = [(pre, 16, 0.75), (post, 2304, 0.75)]
  want = _select_np(sel, 7, counts)
  assert not (want[0][:want[1]] == 0).all(axis=1).any()
  assert nx == 1 or (want[0][0] == (0, 1)).all()
  assert 0 < want[1] < sel.sum()
  _check_select(_select_gpu(gpu, sel, 7, pre=(pre, 16), post=(post, 2304), sel_pad=2, pad=(1, 5)),
                want)
  _check_select(_select_gpu(gpu, sel, 7, pre=(pre, 16)), _select_np(sel, 7, counts[:1]))
  _check_select(_select_gpu(gpu, sel, 7, post=(post, 2304)), _select_np(sel, 7, counts[1:]))


def test_flow_select_refuses_a_count_plane_smaller_than_the_grid(gpu):
  from sofima_amd import _abi
  sel = np.ones((6, 9), np.uint8)
  for shape in ((5, 9), (6, 8)):
    with pytest.raises(_abi.SofimaAmdError, match='smaller than the grid'):
      _select_gpu(gpu, sel, 4, pre=(np.zeros(shape, np.int32), 16))
    with pytest.raises(_abi.SofimaAmdError, match='smaller than the grid'):
      _select_gpu(gpu, sel, 4, post=(np.zeros(shape, np.int32), 16))


def test_flow_select_and_starts_equal_device_plan(gpu):
  """The plan of a round equals what device_plan() makes of the same masks."""
  import torch
  from sofima_amd import flow_field as ff, processor_flow
  rng = np.random.default_rng(3)
  pre_img = rng.integers(0, 255, (200, 216)).astype(np.uint8)
  post_img = np.ascontiguousarray(pre_img[8:184, 8:200])
  pre_mask, post_mask = rng.random((200, 216)) < 0.3, rng.random((176, 192)) < 0.3
  pre_mask[40:120, 30:150] = True
  sel = rng.random((10, 11)) < 0.7
  calc = ff.JAXMaskedXCorrWithStatsCalculator()
  res = ff._Resident(pre_img, post_img, pre_mask, post_mask, gpu)
  plan = calc.device_plan(res, (48, 48), (16, 16), sel, 0.75, 16, (32, 32))
  positions = torch.empty((112, 2), dtype=torch.int32, device=gpu)
  counts = torch.empty((2,), dtype=torch.int32, device=gpu)
  processor_flow.select_patches(
      torch.from_numpy(sel.astype(np.uint8)).to(gpu), 16, positions, counts,
      pre_counts=ff._masked_counts(pre_mask, (48, 48), (16, 16), on_device=True), pre_area=48 * 48,
      post_counts=ff._masked_counts(post_mask, (32, 32), (16, 16), on_device=True),
      post_area=32 * 32)
  n, total = (int(v) for v in counts.cpu().numpy())
  assert 0 < n == plan['n'] < sel.sum() and total == plan['positions'].shape[0]
  assert torch.equal(positions[:total], plan['positions'])
  starts = processor_flow.patch_starts(positions, total, (48, 48), (32, 32), (16, 16),
                                       pre_img.shape, post_img.shape)
  assert torch.equal(starts, plan['starts'])


# ---------------------------------------------------------------------------
# sfm_missing_flow_update
# ---------------------------------------------------------------------------
def _below(v):
  return np.nextafter(np.float32(v), np.float32(0))


def _thresholds(kind):
  """(ratio, sharpness, magnitude) limits that float32 rounds DOWN to a float32
  the fields hold: compared in float32 (a Python number) the value equals the
  limit, compared in float64 (a float64 scalar) it lies below it."""
  vals = []
  for v in (1.4, 1.6, 9.3):
    lo = _below(v)
    vals.append(float(lo) + 0.4 * (float(np.float32(v)) - float(lo)))
    assert np.float32(vals[-1]) == lo
  return tuple(kind(v) for v in vals)


def _update_inputs(shape, field_shape, thresholds, max_attempts, seed):
  rng = np.random.default_rng(seed)
  ratio_t, sharp_t, mag_t = (np.float32(t) for t in thresholds)
  sy, sx = field_shape
  n = sy * sx
  field = np.stack([rng.uniform(-12, 12, field_shape), rng.uniform(-12, 12, field_shape),
                    rng.uniform(0.5, 4, field_shape), rng.uniform(0.5, 3, field_shape)]
                   ).astype(np.float32)

  def sprinkle(c, frac, value):
    field[c].reshape(-1)[rng.random(n) < frac] = value

  for c, values in ((2, (np.nan, -3.0, -0.5, sharp_t, _below(sharp_t), np.inf)),
                    (3, (np.nan, 0.0, -2.0, -0.5, ratio_t, _below(ratio_t))),
                    (0, (mag_t, -mag_t, np.nextafter(mag_t, np.float32(99)), np.nan, np.inf,
                         -np.inf)),
                    (1, (mag_t, np.nan, np.inf))):
    for v in values:
      sprinkle(c, 0.04, v)
  # f1 NaN with f0 finite beyond the limit: np.max propagates the NaN, not bad
  pick = rng.random(field_shape) < 0.05
  field[0][pick], field[1][pick] = 100.0, np.nan
  planes = rng.uniform(-2, 2, (3,) + shape).astype(np.float32)
  planes[2] = 1.0
  mask = rng.random(shape) < 0.7                   # valid nodes outside the mask exist
  planes[:2][:, mask] = np.nan
  attempts = rng.choice([0, max_attempts - 1, max_attempts, max_attempts + 1],
                        size=shape).astype(np.int32)
  return field, planes, mask, attempts


@pytest.mark.parametrize('kind', [float, np.float64, np.float32])
@pytest.mark.parametrize('no_magnitude', [False, True])
@pytest.mark.parametrize('shape', UPDATE_SHAPES)
def test_missing_flow_update_equals_numpy(gpu, shape, no_magnitude, kind):
  import torch
  from sofima_amd import flow_utils, processor_flow
  ratio_t, sharp_t, mag_t = _thresholds(kind)
  if no_magnitude:
    mag_t = kind(0)
  max_attempts = 2
  for field_shape in (shape, (max(1, shape[0] - 2), max(1, shape[1] - 1))):
    field, planes, mask, attempts = _update_inputs(shape, field_shape, _thresholds(kind),
                                                   max_attempts, shape[0] + shape[1])
    want_planes, want_mask, want_att = planes.astype(np.float64), mask.copy(), attempts.copy()
    filled0 = 5
    want_filled = filled0 + ref.update_np(
        field, want_planes, want_mask, want_att, min_peak_ratio=ratio_t,
        min_peak_sharpness=sharp_t, max_magnitude=mag_t, delta_z=-3, max_attempts=max_attempts)

    field_d = torch.from_numpy(field).to(gpu)
    planes_d = torch.from_numpy(planes).to(gpu)
    mask_d = torch.from_numpy(mask.astype(np.uint8)).to(gpu)
    att_d = torch.from_numpy(attempts).to(gpu)
    filled_d = torch.tensor([7, filled0, 9], dtype=torch.int64, device=gpu)
    processor_flow.missing_flow_update(
        field_d, tuple(planes_d), mask_d, att_d, filled_d.data_ptr() + 8, min_peak_ratio=ratio_t,
        min_peak_sharpness=sharp_t, max_magnitude=mag_t, delta_z=-3, max_attempts=max_attempts)
    got_planes = planes_d.cpu().numpy()
    assert np.array_equal(got_planes.view(np.uint32), want_planes.astype(np.float32).view(np.uint32))
    assert np.array_equal(mask_d.cpu().numpy(), want_mask.astype(np.uint8))
    assert np.array_equal(att_d.cpu().numpy(), want_att)
    assert filled_d.cpu().tolist() == [7, want_filled, 9]

    # the accepted set is this package's clean_flow on the same field
    clean = np.asarray(flow_utils.clean_flow(field[:, None], ratio_t, sharp_t, mag_t, 0.0))
    accepted = np.zeros(shape, bool)
    accepted[:field_shape[0], :field_shape[1]] = np.isfinite(clean[0, 0])
    accepted &= mask
    assert np.array_equal(accepted, mask & ~want_mask & (got_planes[2] == -3))
    assert accepted.sum() == want_filled - filled0
    if min(field_shape) > 8:
      # the sprinkled cases are there: valid outside the mask, capped, both outcomes
      valid = np.zeros(shape, bool)
      valid[:field_shape[0], :field_shape[1]] = np.isfinite(field[0])
      assert (valid & ~mask).any() and accepted.any() and (valid & mask & ~accepted).any()
      assert (mask & ~accepted & ~want_mask).any() and want_mask.any()


def test_missing_flow_update_float64_limit_differs_from_its_float32_rounding(gpu):
  """A sharpness that equals the float32 rounding of the limit passes against
  a Python number and fails against the float64 scalar, as in NumPy."""
  import torch
  from sofima_amd import processor_flow
  ratio_t, sharp_t, _ = _thresholds(float)
  field = np.array([1.0, 1.0, _below(1.6), 0.0], np.float32).reshape(4, 1, 1)
  for kind, accepted in ((float, True), (np.float64, False)):
    planes = torch.full((3, 1, 1), float('nan'), device=gpu)
    mask = torch.ones((1, 1), dtype=torch.uint8, device=gpu)
    filled = torch.zeros((1,), dtype=torch.int64, device=gpu)
    processor_flow.missing_flow_update(
        torch.from_numpy(field).to(gpu), tuple(planes), mask,
        torch.zeros((1, 1), dtype=torch.int32, device=gpu), filled.data_ptr(),
        min_peak_ratio=kind(ratio_t), min_peak_sharpness=kind(sharp_t), max_magnitude=0,
        delta_z=2, max_attempts=0)
    assert int(filled.item()) == int(accepted) and int(mask.item()) == 0
    want = ref.clean_np(field, kind(ratio_t), kind(sharp_t), 0)
    assert np.isfinite(want[0, 0, 0]) == accepted


# ---------------------------------------------------------------------------
# estimate_missing_flow
# ---------------------------------------------------------------------------
def _package_flow_fn():
  from sofima_amd import flow_field as ff
  calc = ff.JAXMaskedXCorrWithStatsCalculator()

  def flow_fn(prev, curr, patch, stride, prev_mask, curr_mask, **kw):
    return calc.flow_field(np.ascontiguousarray(prev), np.ascontiguousarray(curr), patch, stride,
                           prev_mask, curr_mask, **kw)

  return flow_fn


@pytest.fixture(scope='module')
def results(gpu, fixture):
  """Per golden case: inputs, the device result and the restated loop driven
  by this package's flow_field(), computed once."""
  from sofima_amd import processor_flow
  out = {}
  for name in CASES:
    cfg = ref.config(fixture, name)
    flow, images, kw = ref.case_kwargs(fixture, cfg, name)
    keep = [a.copy() for a in (flow, images) + tuple(v for v in kw.values()
                                                     if isinstance(v, np.ndarray))]
    got, filled = processor_flow.estimate_missing_flow(flow, images, **kw)
    after = [flow, images] + [v for v in kw.values() if isinstance(v, np.ndarray)]
    untouched = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, after))
    restated = ref.estimate_missing_flow_np(flow, images, _package_flow_fn(), **kw)
    out[name] = dict(flow=flow, images=images, kw=kw, got=got, filled=filled, restated=restated,
                     untouched=untouched)
  return out


@pytest.mark.parametrize('name', CASES)
def test_estimate_missing_flow_equals_the_reference(fixture, results, name):
  r = results[name]
  want = fixture[name + '_out']
  assert r['got'].dtype == np.float32 and r['got'].shape == want.shape
  assert r['filled'].dtype == np.int64
  assert np.array_equal(np.isnan(r['got']), np.isnan(want))
  assert np.array_equal(r['got'][2], want[2])
  assert np.array_equal(r['got'][:2], want[:2], equal_nan=True)
  assert np.array_equal(r['filled'], fixture[name + '_filled'])
  assert r['untouched']


@pytest.mark.parametrize('name', CASES)
def test_estimate_missing_flow_equals_the_restated_loop_bit_for_bit(results, name):
  r = results[name]
  want, want_filled = r['restated']
  assert np.array_equal(r['got'].view(np.uint32), want.view(np.uint32))
  assert np.array_equal(r['filled'], want_filled)


@pytest.mark.parametrize('name', CASES)
def test_estimate_missing_flow_input_kinds_and_device_output(gpu, results, name):
  import torch
  from sofima_amd import _dev, processor_flow
  r = results[name]

  def on_device(v, wrap):
    if not isinstance(v, np.ndarray):
      return v
    t = torch.from_numpy(v).to(gpu)
    return _dev.DeviceArray(t) if wrap and t.dtype in (torch.float32, torch.uint8) else t

  for wrap in (False, True):
    kw = {k: on_device(v, wrap) for k, v in r['kw'].items()}
    got, filled = processor_flow.estimate_missing_flow(
        on_device(r['flow'], wrap), on_device(r['images'], wrap), device_output=True, **kw)
    assert isinstance(got, _dev.DeviceArray) and got.tensor.is_cuda
    assert isinstance(filled, np.ndarray)
    assert np.array_equal(np.asarray(got).view(np.uint32), r['got'].view(np.uint32))
    assert np.array_equal(filled, r['filled'])


def test_estimate_missing_flow_skips_a_masked_current_section(gpu, results):
  """processor/flow.py:752-756, and float32 images; against the restated loop."""
  from sofima_amd import processor_flow
  r = results['bwd']
  kw = dict(r['kw'])
  masks = kw['masks'].copy()
  ys, xs = kw['curr_slice']
  masks[1][ys, xs] = True            # all True inside the current slice only
  kw['masks'] = masks
  images = r['images'].astype(np.float32)
  got, filled = processor_flow.estimate_missing_flow(r['flow'], images, **kw)
  want, want_filled = ref.estimate_missing_flow_np(r['flow'], images, _package_flow_fn(), **kw)
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
  assert np.array_equal(filled, want_filled)
  assert filled[1].sum() == 0 and np.array_equal(got[:2, 1], r['flow'][:, 1], equal_nan=True)


def test_estimate_missing_flow_negative_max_attempts_estimates_nothing(gpu, results):
  from sofima_amd import processor_flow
  r = results['fwd']
  got, filled = processor_flow.estimate_missing_flow(r['flow'], r['images'],
                                                     **dict(r['kw'], max_attempts=-1))
  assert filled.sum() == 0 and np.array_equal(got[:2], r['flow'], equal_nan=True)
  assert np.all(got[2] == r['kw']['delta_z'])


def test_estimate_missing_flow_refuses_a_curr_slice_of_another_grid(gpu, results):
  from sofima_amd import processor_flow
  r = results['fwd']
  ys, xs = r['kw']['curr_slice']
  with pytest.raises(ValueError, match='flow grid'):
    processor_flow.estimate_missing_flow(
        r['flow'], r['images'], **dict(r['kw'], curr_slice=(ys, slice(xs.start, xs.stop - 16))))


KAT = dict(patch_size=16, stride=16, delta_z=1, max_attempts=1, min_peak_sharpness=0.0,
           min_peak_ratio=0.0, max_magnitude=0, batch_size=10, search_radius=16)


def _kat_call(vol, box_start, max_delta_z):
  from sofima_amd import processor_flow
  geo = processor_flow.missing_flow_geometry(
      box_start, (2, 2, 1), vol.shape[::-1], patch_size=16, stride=16, search_radius=16,
      delta_z=1, max_delta_z=max_delta_z)
  (x0, y0, z0), (sx, sy, sz) = geo.load_start, geo.load_size
  flow = np.full((2, 1, 2, 2), np.nan, dtype=np.float32)[(slice(None), slice(None)) +
                                                        geo.flow_slice]
  return processor_flow.estimate_missing_flow(
      flow, vol[z0:z0 + sz, y0:y0 + sy, x0:x0 + sx], max_delta_z=max_delta_z,
      curr_slice=geo.curr_slice, z0=geo.z0, **KAT)


def test_reference_known_answer(gpu):
  """processor/flow_test.py:57-122 re-typed."""
  rng = np.random.default_rng(0)
  vol = rng.random((10, 128, 128)).astype(np.float32)
  dx, dy = 2, 3
  shifted = np.zeros_like(vol[3])
  shifted[dy:, dx:] = vol[3][:-dy, :-dx]
  shifted[:dy, :] = rng.random((dy, 128))
  shifted[:, :dx] = rng.random((128, dx))
  vol[5] = shifted
  data, filled = _kat_call(vol, (2, 2, 5), 2)
  assert data.shape == (3, 1, 2, 2)
  assert not np.any(np.isnan(data)), 'Result contains NaNs'
  np.testing.assert_allclose(data[2], 2, err_msg='delta_z incorrect')
  np.testing.assert_allclose(data[0, 0, 0, 0], -dx, atol=0.5, err_msg='Flow X incorrect')
  np.testing.assert_allclose(data[1, 0, 0, 0], -dy, atol=0.5, err_msg='Flow Y incorrect')
  assert filled.tolist() == [[4]]


def test_reference_known_answer_clipped_context(gpu):
  """processor/flow_test.py:124-170 re-typed: z = 1 has only z = 0 before it,
  which is the look-back the input covers; every further one leaves the stack."""
  vol = np.random.default_rng(1).random((10, 128, 128)).astype(np.float32)
  data, filled = _kat_call(vol, (2, 2, 1), 5)
  assert data.shape == (3, 1, 2, 2)
  assert np.all(np.isnan(data[0])) and np.all(np.isnan(data[1]))
  assert data[2, 0, 0, 0] == 1
  assert filled.shape == (1, 4) and filled.sum() == 0


# ---------------------------------------------------------------------------
# estimate_flow
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stack():
  rng = np.random.default_rng(5)
  images = rng.integers(0, 255, (5, 96, 112)).astype(np.uint8)
  masks = rng.random((5, 96, 112)) < 0.2
  masks[2, 10:70, 20:90] = True
  selection = rng.random((5, 5, 6)) < 0.8
  return images, masks, selection


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('z_stride, fixed_current', [(1, False), (-2, False), (1, True),
                                                     (-1, True)])
def test_estimate_flow_planes_equal_flow_field_calls(gpu, stack, z_stride, fixed_current, masked):
  from sofima_amd import _dev, flow_field as ff, processor_flow
  images, masks, selection = stack
  kw = dict(masks=masks, selection_mask=selection) if masked else {}
  got = processor_flow.estimate_flow(images, 32, 16, z_stride, fixed_current=fixed_current,
                                     batch_size=8, **kw)
  pairs = ref.flow_pairs_np(5, z_stride, fixed_current)
  assert got.dtype == np.float32 and got.shape == (4, len(pairs), 5, 6)
  calc = ff.JAXMaskedXCorrWithStatsCalculator()
  for i, (zp, zc) in enumerate(pairs):
    want = calc.flow_field(images[zp], images[zc], 32, 16, masks[zp] if masked else None,
                           masks[zc] if masked else None,
                           selection_mask=selection[zc] if masked else None, batch_size=8)
    assert np.array_equal(got[:, i].view(np.uint32), want.view(np.uint32)), (zp, zc)
  assert np.isfinite(got[0]).any()
  on_dev = processor_flow.estimate_flow(images, 32, 16, z_stride, fixed_current=fixed_current,
                                        batch_size=8, device_output=True, **kw)
  assert isinstance(on_dev, _dev.DeviceArray)
  assert np.array_equal(np.asarray(on_dev).view(np.uint32), got.view(np.uint32))
