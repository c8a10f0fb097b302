"""map_utils.invert_map without a GPU: the C-ABI surface, argument errors of
the reference's types and the SciPy statement against the golden file."""
import ctypes
import os
import re

import numpy as np
import pytest

from sofima_amd import _abi, _build, map_utils
from tests import invert_map_scipy as ims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sofima_amd.h')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'invert_map.npz')


def test_desc_field_order_matches_header():
  text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
  body = re.search(r'typedef struct SfmInvertMapDesc \{(.*?)\} SfmInvertMapDesc;', text,
                   re.S).group(1)
  names = [re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])*\s*$', d.strip()).group(1)
           for d in body.split(';') if d.strip()]
  assert names == [f[0] for f in _abi.SfmInvertMapDesc._fields_]
  assert 'sfm_invert_map' in _abi.SIGNATURES
  assert 'sfm_invert_map_workspace_bytes' in _abi.SIGNATURES


@pytest.fixture(scope='module')
def lib():
  if not os.path.exists(_abi.lib_path()):
    _build.build()
  return _abi.load()


def _desc(shape, dst):
  d = _abi.SfmInvertMapDesc()
  d.shape = (ctypes.c_int32 * 3)(*shape)
  d.dst_shape = (ctypes.c_int32 * 2)(*dst)
  d.stride = (ctypes.c_double * 2)(40.0, 40.0)
  return d


def test_workspace_bytes(lib):
  small = lib.sfm_invert_map_workspace_bytes(ctypes.byref(_desc((1, 8, 8), (8, 8))))
  big = lib.sfm_invert_map_workspace_bytes(ctypes.byref(_desc((16, 205, 205), (207, 207))))
  assert 0 < small < big
  # per node: positions, grid positions, B index; per query: the winning key
  assert big >= 16 * 205 * 205 * 36 + 16 * 207 * 207 * 8
  assert lib.sfm_invert_map_workspace_bytes(None) == 0
  assert lib.sfm_invert_map_workspace_bytes(ctypes.byref(_desc((0, 8, 8), (8, 8)))) == 0


def test_null_descriptor_rejected(lib):
  assert lib.sfm_invert_map(None, None) == -1
  assert b'NULL' in lib.sfm_last_error()


def test_no_gpu_raises_sofima_error():
  import torch
  if torch.cuda.is_available():
    pytest.skip('GPU present')
  b = ims.box((0, 0, 0), (4, 4, 1))
  with pytest.raises(_abi.SofimaAmdError):
    map_utils.invert_map(np.zeros((2, 1, 4, 4)), b, b, 40)


def test_argument_errors_have_the_reference_types():
  b = ims.box((0, 0, 0), (4, 4, 1))
  with pytest.raises(ValueError, match='mismatch'):
    map_utils.invert_map(np.zeros((2, 1, 4, 5)), b, b, 40)
  with pytest.raises(AssertionError):
    map_utils.invert_map(np.zeros((2, 1, 4, 4)), b, b, (40, 40, 40))
  with pytest.raises(NotImplementedError, match='3-D'):
    map_utils.invert_map(np.zeros((3, 1, 4, 4)), b, b, 40)
  with pytest.raises(NotImplementedError):
    map_utils.invert_map(np.zeros((4, 1, 4, 4)), b, b, 40)
  with pytest.raises(ValueError):
    map_utils.invert_map(np.zeros((2, 4, 4)), b, b, 40)


def test_scipy_statement_matches_reference_golden():
  pytest.importorskip('scipy')
  g = np.load(GOLDEN)
  n = len([k for k in g.files if k.endswith('_name')])
  assert n >= 18
  for i in range(n):
    k = f'{i:02d}'
    src, dst = ims.box(*g[k + '_src']), ims.box(*g[k + '_dst'])
    stride = tuple(float(v) for v in g[k + '_stride'])
    got = ims.invert_restated(g[k + '_map'], src, dst, stride)
    want = g[k + '_out']
    assert np.array_equal(np.isnan(got), np.isnan(want)), str(g[k + '_name'])
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), atol=1e-9,
                               err_msg=str(g[k + '_name']))
