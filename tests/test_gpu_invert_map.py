"""map_utils.invert_map on the device: golden cases from the unmodified
reference, the reference's KATs, a SciPy fuzz, refusals and a warp chain."""
import os

import numpy as np
import pytest
import torch

from sofima_amd import _abi, map_utils, warp
from sofima_amd._dev import DeviceArray
from tests import invert_map_scipy as ims

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'invert_map.npz')


def golden_cases():
  g = np.load(GOLDEN)
  n = len([k for k in g.files if k.endswith('_name')])
  for i in range(n):
    k = f'{i:02d}'
    yield (str(g[k + '_name']), g[k + '_map'], ims.box(*g[k + '_src']),
           ims.box(*g[k + '_dst']), tuple(float(v) for v in g[k + '_stride']), g[k + '_out'])


@pytest.mark.parametrize('case', list(golden_cases()), ids=lambda c: c[0])
def test_golden_cases_meet_the_contract(case):
  name, cm, src, dst, stride, want = case
  got = map_utils.invert_map(cm, src, dst, stride)
  assert isinstance(got, DeviceArray)
  got = np.asarray(got)
  assert got.dtype == np.float64 and got.shape == want.shape
  diag = ims.check_contract(cm, src, dst, stride, got, want)
  # the SciPy statement needs no exception against these outputs either
  # (tests/test_invert_map_cases.py::test_golden_cases_need_no_exception_on_the_host)
  assert diag == 0, f'{name}: {diag} nodes by the diagonal exception'


def test_reference_kat():
  """map_utils_test.py:205-215."""
  b = ims.box((100, 200, 10), (50, 50, 1))
  hx = np.mgrid[:50, :50][1]
  cm = np.zeros([2, 1, 50, 50])
  cm[1, 0] = np.sin(hx / 25) * 20
  inv = np.asarray(map_utils.invert_map(cm, b, b, 40.0))
  np.testing.assert_array_almost_equal(inv[:, :, 1:, 1:], -cm[:, :, 1:, 1:], decimal=5)


def test_compose_with_inverse_is_identity():
  """map_utils_test.py:298-321, through the port's compose_maps_fast."""
  b = ims.box((100, 200, 10), (50, 50, 1))
  cm = np.zeros([2, 1, 50, 50])
  hy, hx = np.mgrid[:50, :50]
  cm[0, 0] = np.sin(hx / 25)
  cm[1, 0] = np.cos(hy / 25)
  inv = map_utils.invert_map(cm, b, b, 5)
  comp = np.asarray(map_utils.compose_maps_fast(cm, b.start[::-1], 5, inv, b.start[::-1], 5))
  comp = comp[:, :, 1:-2, 1:-2]
  np.testing.assert_array_almost_equal(comp, np.zeros_like(comp), decimal=3)


def _smooth(rng, z, h, w, amp):
  from scipy import ndimage
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((z, h, w)), (0, 5, 5))
                for _ in range(2)])
  return f / np.abs(f).max() * amp


@pytest.mark.parametrize('seed,shape,holes', [(0, (1, 205, 205), 0.0), (1, (4, 96, 96), 0.05),
                                              (2, (2, 64, 80), 0.1)])
def test_scipy_fuzz(seed, shape, holes):
  pytest.importorskip('scipy')
  from scipy import ndimage
  rng = np.random.default_rng(seed)
  cm = _smooth(rng, *shape, 0.6 * 40)
  if holes:
    noise = ndimage.gaussian_filter(rng.standard_normal(shape), (0, 1.5, 1.5))
    cm[:, noise > np.quantile(noise, 1 - holes)] = np.nan
  src = ims.box((7, 3, 0), (shape[2], shape[1], shape[0]))
  dst = ims.box((6, 2, 0), (shape[2] + 2, shape[1] + 2, shape[0]))
  got = np.asarray(map_utils.invert_map(cm.astype(np.float32), src, dst, 40))
  want = ims.invert_restated(cm.astype(np.float32), src, dst, 40)
  diag = ims.check_contract(cm.astype(np.float32), src, dst, 40, got, want)
  assert diag == 0, f'seed {seed}: {diag} nodes by the diagonal exception'


def _folded():
  b = ims.box((0, 0, 0), (20, 20, 1))
  cm = np.zeros((2, 1, 20, 20))
  cm[0, 0, 10, 10] = 55.0  # node (10, 10) jumps past its right neighbour
  return cm, b


def test_fold_is_refused_then_masked_fold_meets_the_contract():
  cm, b = _folded()
  with pytest.raises(_abi.SofimaAmdError, match='slice 0.*fold'):
    map_utils.invert_map(cm, b, b, 40)
  masked = cm[:, 0].copy()
  bad = map_utils.mask_irregular(masked, (40, 40), 0.5)
  assert bad.any()
  masked = masked[:, None]
  got = np.asarray(map_utils.invert_map(masked, b, b, 40))
  want = ims.invert_restated(masked, b, b, 40)
  ims.check_contract(masked, b, b, 40, got, want)


def test_fold_in_second_slice_names_it():
  cm, b = _folded()
  cm = np.concatenate([np.zeros_like(cm), cm], axis=1)
  b = ims.box((0, 0, 0), (20, 20, 2))
  with pytest.raises(_abi.SofimaAmdError, match='slice 1'):
    map_utils.invert_map(cm, b, b, 40)


def test_boundary_cap_is_refused():
  # a checkerboard of NaN leaves no full quad: every valid node is a boundary node
  n = 130
  cm = np.zeros((2, 1, n, n))
  yy, xx = np.mgrid[:n, :n]
  cm[:, 0, (yy + xx) % 2 == 1] = np.nan
  b = ims.box((0, 0, 0), (n, n, 1))
  with pytest.raises(_abi.SofimaAmdError, match='7936 boundary nodes'):
    map_utils.invert_map(cm, b, b, 40)


def test_3d_is_not_implemented():
  b = ims.box((0, 0, 0), (4, 4, 2))
  with pytest.raises(NotImplementedError, match='3-D'):
    map_utils.invert_map(np.zeros((3, 2, 4, 4)), b, b, 40)


@pytest.mark.parametrize('kind', ['numpy32', 'numpy64', 'torch', 'device'])
def test_repeatable_and_input_untouched(kind):
  rng = np.random.default_rng(5)
  cm = _smooth(rng, 2, 40, 44, 20.0)
  cm[:, 1, 10:14, 10:30] = np.nan
  b = ims.box((0, 0, 0), (44, 40, 2))
  if kind == 'numpy32':
    x = cm.astype(np.float32)
  elif kind == 'numpy64':
    x = cm.copy()
  elif kind == 'torch':
    x = torch.from_numpy(cm.astype(np.float32)).cuda()
  else:
    x = DeviceArray(torch.from_numpy(cm).cuda())
  before = np.asarray(x.cpu() if kind == "torch" else x).copy()
  a = map_utils.invert_map(x, b, b, 40)
  c = map_utils.invert_map(x, b, b, 40)
  assert a.dtype == np.float64
  assert np.array_equal(np.asarray(a), np.asarray(c), equal_nan=True)
  after = np.asarray(x.cpu() if kind == 'torch' else x)
  assert np.array_equal(before, after, equal_nan=True)


def test_relax_invert_warp_chain():
  """mesh relaxation -> invert_map -> ndimage_warp, against the same chain on
  the SciPy-inverted map."""
  from sofima_amd import mesh
  rng = np.random.default_rng(3)
  stride = 20
  h, w = 24, 24
  flow = _smooth(rng, 1, h, w, 6.0).astype(np.float32)
  cfg = mesh.IntegrationConfig(dt=0.001, gamma=0.0, k0=0.01, k=0.1, stride=(stride, stride),
                               num_iters=200, max_iters=200, stop_v_max=0.001,
                               dt_max=100, start_cap=0.01, final_cap=10, prefer_orig_order=True)
  x, _, _ = mesh.relax_mesh(np.zeros_like(flow), flow, cfg)
  x = np.asarray(x)
  b = ims.box((0, 0, 0), (w, h, 1))
  inv = np.asarray(map_utils.invert_map(x, b, b, stride))
  ref = ims.invert_restated(x, b, b, stride)
  ims.check_contract(x, b, b, stride, inv, ref)
  img = (rng.random((h * stride, w * stride)) * 255).astype(np.float32)
  inv0 = np.nan_to_num(inv[:, 0])
  ref0 = np.nan_to_num(ref[:, 0])
  work = (img.shape[1], img.shape[0])
  a = np.asarray(warp.ndimage_warp(img, inv0, (stride, stride), work, (0, 0)))
  r = np.asarray(warp.ndimage_warp(img, ref0, (stride, stride), work, (0, 0)))
  assert a.shape == r.shape
  assert np.mean(np.abs(a - r)) < 0.5
