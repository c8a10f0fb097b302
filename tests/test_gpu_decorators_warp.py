"""`decorators_warp.warp_affine` / `warp_coord_map` on the device (-m gpu) against the
reference's own `_warp_affine` and `_warp_coord_map`, run through the golden shim
(tests/golden/warp_decorators.npz, made by make_golden_warp_decorators.py): every
array bit for bit, and the reference's error cases with its exception types."""
import numpy as np
import pytest

from sofima_amd import _abi, _spline, decorators_warp

pytestmark = pytest.mark.gpu


def assert_same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


@pytest.fixture(autouse=True)
def spline_orders():
  with _abi.option(_spline.OPTION, 1):
    yield


@pytest.fixture(scope='module')
def fixture(golden):
  return golden('warp_decorators')


def _names(kind):
  import os
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'warp_decorators.npz')
  with np.load(path) as g:
    return [str(n) for n in g['names'] if str(g[f'{n}_kind']) == kind]


@pytest.mark.parametrize('name', _names('affine'))
def test_warp_affine(gpu, fixture, name):
  g = fixture
  got = decorators_warp.warp_affine(g[f'{name}_image'], g[f'{name}_matrix'],
                                    order=int(g[f'{name}_order']),
                                    implementation=str(g[f'{name}_impl']))
  assert_same(got, g[f'{name}_out'], name)
  assert np.mean(got != 0) > 0.2


@pytest.mark.parametrize('name', _names('coord_map'))
def test_warp_coord_map(gpu, fixture, name):
  g = fixture
  scale = g[f'{name}_scale']
  kw = dict(stride=tuple(float(v) for v in g[f'{name}_stride']), overlap=(0, 0, 0),
            order=int(g[f'{name}_order']), scale_xyz=tuple(scale) if scale.size else None)
  got = decorators_warp.warp_coord_map(g[f'{name}_image'], g[f'{name}_map'],
                                       mode=str(g[f'{name}_mode']), cval=float(g[f'{name}_cval']),
                                       **kw)
  assert_same(got, g[f'{name}_out'], name)
  default = decorators_warp.warp_coord_map(g[f'{name}_image'], g[f'{name}_map'], **kw)
  assert np.mean(got != default) > 0.2


def test_the_private_names_are_aliases():
  assert decorators_warp._warp_affine is decorators_warp.warp_affine
  assert decorators_warp._warp_coord_map is decorators_warp.warp_coord_map


def test_error_cases(gpu):
  img2 = np.zeros((6, 5), np.uint8)
  img3 = np.zeros((6, 5, 4), np.uint8)
  m2 = np.eye(3)[:2]
  m3 = np.eye(4)[:3]
  with pytest.raises(ValueError, match='2 or 3 image dimensions are required, but got 1'):
    decorators_warp.warp_affine(np.zeros(5, np.uint8), m2)
  with pytest.raises(ValueError, match='2 matrix dimensions are required, but got 1'):
    decorators_warp.warp_affine(img2, np.ones(3))
  with pytest.raises(ValueError, match='3 matrix cols are required, but got 4'):
    decorators_warp.warp_affine(img2, m3)
  with pytest.raises(ValueError, match='3 or 4 matrix rows are required, but got 2'):
    decorators_warp.warp_affine(img3, np.ones((2, 4)))
  with pytest.raises(RuntimeError, match='Only 2D images are supported'):
    decorators_warp.warp_affine(img3, m3, implementation='opencv')
  with pytest.raises(NotImplementedError, match='opencv'):
    decorators_warp.warp_affine(img2, m2, implementation='opencv')
  with pytest.raises(RuntimeError, match='Only 3D images are supported with `implementation=sofima`'):
    decorators_warp.warp_affine(img2, m2, implementation='sofima')
  with pytest.raises(ValueError, match='implementation must be `opencv`, `scipy`, or `sofima`'):
    decorators_warp.warp_affine(img2, m2, implementation='cupy')
  with pytest.raises(RuntimeError, match='Only 3D images are supported.'):
    decorators_warp.warp_coord_map(img2, np.zeros((2, 2, 2)), stride=(1, 1), overlap=(0, 0))
  # identity: both implementations hand the image back
  img = np.arange(120, dtype=np.uint8).reshape(6, 5, 4)
  for impl in ('scipy', 'sofima'):
    np.testing.assert_array_equal(decorators_warp.warp_affine(img, m3, implementation=impl), img)
