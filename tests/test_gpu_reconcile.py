"""sfm_reconcile_flows on the GPU: bit-exact against the reference's golden
output and against the restatement of tests/test_reconcile.py (-m gpu)."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.test_reconcile import golden_cases, reconcile_restated

pytestmark = pytest.mark.gpu


def _run(flows, *params):
  from sofima_amd import flow_utils
  out = flow_utils.reconcile_flows(flows, *params)
  got = np.asarray(out)
  assert got.dtype == np.float32
  return out, got


def _same(got, want, what=''):
  assert got.shape == want.shape, what
  if not np.array_equal(got, want, equal_nan=True):
    diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    idx = np.argwhere(diff)[:5]
    raise AssertionError(f'{what}: {int(diff.sum())} elements differ, first at {idx.tolist()}: '
                         f'got {[got[tuple(i)] for i in idx]}, want {[want[tuple(i)] for i in idx]}')


def _noise_flow(rng, c, z, y, x, hole_frac, sigma=1.0):
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, y, x)), (0, 2, 2)) * 20
                for _ in range(c)]).astype(np.float32)
  hit = rng.random((z, y, x)) < 0.03
  f[:2, hit] += rng.uniform(-30, 30, (2, int(hit.sum()))).astype(np.float32)
  noise = ndimage.gaussian_filter(rng.standard_normal((z, y, x)), (0, sigma, sigma))
  f[:, noise < np.quantile(noise, hole_frac)] = np.nan
  return f


def test_golden(gpu, golden):
  g = golden('reconcile_flows')
  for name, flows, params, want in golden_cases(g):
    _, got = _run(flows, *params)
    _same(got, want, name)


def test_fuzz_smoothed_noise(gpu):
  rng = np.random.default_rng(2024)
  for it in range(40):
    c = int(rng.integers(2, 4))
    k = int(rng.integers(1, 4))
    z = int(rng.integers(1, 4))
    y = int(rng.integers(1, 70))
    x = int(rng.integers(1, 70))
    sigma = float(rng.uniform(0.5, 2.5))
    flows = [_noise_flow(rng, c, z, y, x, float(rng.uniform(0.2, 0.7)), sigma)
             for _ in range(k)]
    if c == 3:
      for f in flows[1:]:
        f[2][rng.random(f[2].shape) < 0.1] = np.nan
      flows[0][2][rng.random(flows[0][2].shape) < 0.02] = np.nan
    # thresholds float32 cannot hold, as Python floats or float64 scalars
    thr = np.float64 if it % 3 == 2 else float
    params = (float(rng.choice([0, 2.0, 6.0, 15.0, 0.1, 1.1, 3.3])),
              thr(rng.choice([0, 1.0, 4.0, 12.0, 0.1, 1.1, 2.7])),
              int(rng.choice([0, 1, 2, 3, 7, 20, 150])), thr(rng.choice([0, 1, 3, 0.7, 1.1])))
    _, got = _run(flows, *params)
    _same(got, reconcile_restated(flows, *params), f'case {it}: {c, k, z, y, x} {params}')


def test_section_stack_two_flows(gpu):
  """[2, 16, 205, 205]: an 8192^2 section at stride 40, 16 sections, two flows."""
  rng = np.random.default_rng(5)
  flows = [_noise_flow(rng, 2, 16, 205, 205, 0.35), _noise_flow(rng, 2, 16, 205, 205, 0.2)]
  for params in ((0, 20, 400, 0), (3.0, 4.0, 50, 0), (0, 0, 2000, 0)):
    _, got = _run(flows, *params)
    _same(got, reconcile_restated(flows, *params), str(params))


def _spiral(h, w):
  m = np.zeros((h, w), bool)
  t, b, l, r = 0, h - 1, 0, w - 1
  while t <= b and l <= r:
    m[t, l:r + 1] = True
    m[t:b + 1, r] = True
    m[b, l:r + 1] = True
    m[t + 2:b + 1, l] = True
    t, b, l, r = t + 2, b - 2, l + 2, r - 2
    if t <= b and l <= r:
      m[t, l - 2:l] = True
  return m


def _snake(h, w):
  m = np.zeros((h, w), bool)
  m[0::2] = True
  m[1::4, -1] = True
  m[3::4, 0] = True
  return m


def test_spiral_and_snake_2048(gpu):
  """One slice of 2048^2 holding a spiral and a snake: the longest chains a
  union-find meets (one component of ~10^6 vectors each)."""
  valid = np.zeros((2048, 2048), bool)
  valid[:, :1020] = _spiral(2048, 1020)
  valid[:, 1024:] = _snake(2048, 1024)
  lab, n = ndimage.label(valid)
  sizes = np.bincount(lab.ravel())[1:]
  big = np.sort(sizes)[-2:]
  assert n == 2 and big.min() > 500_000, (n, big)
  f = np.where(valid, 1.0, np.nan).astype(np.float32)[None, None].repeat(2, 0)
  f[1] *= 2
  for patch in (400, int(big.min()) + 1, int(big.max()) + 1):
    _, got = _run([f], 0, 0, patch)
    _same(got, reconcile_restated([f], 0, 0, patch), f'min_patch_size {patch}')
  # the snake survives the first two, nothing the last
  _, got = _run([f], 0, 0, int(big.max()) + 1)
  assert np.isnan(got).all()


def test_components_do_not_join_across_z(gpu):
  f = np.full((2, 4, 12, 12), np.nan, np.float32)
  for z in range(4):
    f[:, z, 2:5, 3:6] = z + 1       # 9 vectors at the same (y, x) in every slice
  f[:, 1, 8:12, 0:4] = 1            # 16 in slice 1 only
  _, got = _run([f], 0, 0, 10)
  assert np.isnan(got[:, :, 2:5, 3:6]).all()
  assert not np.isnan(got[:, 1, 8:12, 0:4]).any()
  _same(got, reconcile_restated([f], 0, 0, 10))


def test_mixed_inputs_unchanged(gpu):
  from sofima_amd import _dev
  rng = np.random.default_rng(9)
  a, b, c = (_noise_flow(rng, 3, 2, 40, 33, q) for q in (0.5, 0.4, 0.1))
  b64 = b.astype(np.float64)
  ta = torch.from_numpy(a.copy()).to(gpu)
  dc = _dev.DeviceArray(torch.from_numpy(c.copy()).to(gpu))
  keep = (ta.clone(), b64.copy(), dc.tensor.clone())
  want = reconcile_restated([a, b, c], 4.0, 3.0, 5, 1)
  out, got = _run([ta, b64, dc], 4.0, 3.0, 5, 1)
  assert isinstance(out, _dev.DeviceArray)
  assert out.tensor.device.type == 'cuda'
  _same(got, want, 'torch + float64 NumPy + DeviceArray')
  assert torch.equal(ta.isnan(), keep[0].isnan())
  assert torch.equal(torch.nan_to_num(ta), torch.nan_to_num(keep[0]))
  assert np.array_equal(b64, keep[1], equal_nan=True)
  assert torch.equal(torch.nan_to_num(dc.tensor), torch.nan_to_num(keep[2]))
  # one flow, passed without a copy, is not written either
  out, got = _run([ta], 4.0, 3.0, 5)
  assert out.tensor.data_ptr() != ta.data_ptr()
  _same(got, reconcile_restated([a], 4.0, 3.0, 5))
  assert torch.equal(torch.nan_to_num(ta), torch.nan_to_num(keep[0]))


def test_one_stacked_array_of_flows(gpu):
  """A [K, c, z, y, x] array is K flows, as in the reference (flows[0], flows[1:])."""
  from sofima_amd import _dev
  rng = np.random.default_rng(12)
  stack = np.stack([_noise_flow(rng, 2, 3, 30, 31, q) for q in (0.5, 0.3, 0.1)])
  want = reconcile_restated(list(stack), 2.5, 1.1, 6)
  keep = stack.copy()
  for arg in (stack, torch.from_numpy(stack).to(gpu),
              _dev.DeviceArray(torch.from_numpy(stack).to(gpu))):
    _, got = _run(arg, 2.5, 1.1, 6)
    _same(got, want, type(arg).__name__)
  assert np.array_equal(stack, keep, equal_nan=True)
  _, got = _run(stack[:1], 2.5, 1.1, 6)
  _same(got, reconcile_restated([stack[0]], 2.5, 1.1, 6), 'K = 1')


def test_bad_shapes_raise(gpu):
  from sofima_amd import flow_utils
  f = np.zeros((2, 1, 4, 4), np.float32)
  with pytest.raises(ValueError):
    flow_utils.reconcile_flows([], 1, 1, 1)
  with pytest.raises(ValueError):
    flow_utils.reconcile_flows([np.zeros((4, 1, 4, 4), np.float32)], 1, 1, 1)
  with pytest.raises(ValueError):
    flow_utils.reconcile_flows([np.zeros((2, 4, 4), np.float32)], 1, 1, 1)
  with pytest.raises(ValueError):
    flow_utils.reconcile_flows([f, np.zeros((2, 1, 4, 5), np.float32)], 1, 1, 1)
  with pytest.raises(ValueError):
    flow_utils.reconcile_flows([f, np.zeros((3, 1, 4, 4), np.float32)], 1, 1, 1)
  with pytest.raises(ValueError):
    flow_utils.reconcile_flows(f, 1, 1, 1)          # one flow, not a sequence of them
  with pytest.raises(ValueError):
    flow_utils.reconcile_flows(np.zeros((0, 2, 1, 4, 4), np.float32), 1, 1, 1)


def test_device_chain_flow_clean_reconcile(gpu, golden):
  """flow_field(device_output=True) -> clean_flow -> reconcile_flows on the
  device == the same chain on the host."""
  from oracle import flow_utils_oracle
  from sofima_amd import _dev, flow_field, flow_utils
  g = golden('flow2d')
  calc = flow_field.JAXMaskedXCorrWithStatsCalculator()
  host = calc.flow_field(g['pre'], g['post'], 48, 24, batch_size=8)
  devf = calc.flow_field(g['pre'], g['post'], 48, 24, batch_size=8, device_output=True)
  assert isinstance(devf, _dev.DeviceArray)
  strict = flow_utils.clean_flow(devf.tensor[:, None], 1.6, 1.6, 0, 2)
  loose = flow_utils.clean_flow(devf.tensor[:, None], 1.1, 1.1, 0, 8)
  want_strict = flow_utils_oracle.clean_flow(host[:, None], 1.6, 1.6, 0, 2)
  want_loose = flow_utils_oracle.clean_flow(host[:, None], 1.1, 1.1, 0, 8)
  for params in ((0, 2, 4, 0), (3.0, 1.0, 2, 0), (0, 0, 6, 0)):
    got = flow_utils.reconcile_flows([strict, loose], *params)
    assert isinstance(got, _dev.DeviceArray)
    want = reconcile_restated([want_strict, want_loose], *params)
    _same(np.asarray(got), want, str(params))
