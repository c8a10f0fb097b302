"""Every kernel of the map_coordinates family is launched and checked (-m gpu): the
launch table of `sfm_warp.hip` over dtype x order x dimension x map accessor x
boundary class, for `warp.ndimage_warp`, `warp.affine_transform` and the 3-D render.

A wrong table entry -- order 4 reaching the order-3 kernel, the 3-D taps reaching the
kernel without them, a float32 map read as float64 -- gives another result on these
inputs: the images are random, smaller than the 6 taps of order 5 on some axes, and
the coordinates leave them on every axis; `test_the_references_tell_the_entries_apart`
holds that on SciPy's results alone, without a device.  The expected values are
SciPy's own (`ndwarp_modes_ref.ndimage_warp_scipy`, `scipy.ndimage.affine_transform`)
and for the render `ndwarp_spline_ref.render`; equality is bit for bit.

The map values are multiples of 1/8 and the strides of 1/2, so that the absolute
node coordinates are exact in float16, float32 and float64 alike: the three map
kinds -- a float16 NumPy map, which the host makes absolute in float64, and the
relative float32 and float64 maps that the kernels read -- share one expected result.
"""
import functools
import itertools

import numpy as np
import pytest
import scipy.ndimage

from sofima_amd import _abi, _spline, processor_warp, warp
from tests import ndwarp_modes_ref as ref
from tests import ndwarp_spline_ref as spline_ref
from tests.render3d_ref import box

DTYPES = (np.uint8, np.uint16, np.float32)
ORDERS = (0, 1, 2, 3, 4, 5)
SHAPES = {2: (5, 6), 3: (3, 5, 6)}
NODES = {2: (3, 3), 3: (2, 3, 3)}
STRIDES = {2: (2.0, 2.5), 3: (2.0, 2.0, 2.5)}      # the last node lies on the last voxel
MAP_DTYPES = (np.float16, np.float32, np.float64)  # absolute on the host, relative x 2
# boundary class -> (mode, cval): the plain kernels, the mode kernels, and at orders 2 to
# 5 the taps kernels with the padded image (two modes) and without
BOUNDARIES = {'none': None, 'mirror': ('mirror', 0.0), 'nearest': ('nearest', 0.0),
              'grid-constant': ('grid-constant', 7.25), 'reflect': ('reflect', 0.0)}


def _image(dim, dtype):
  rng = np.random.default_rng(1000 * dim + np.dtype(dtype).itemsize)
  return ref.image(rng, SHAPES[dim], dtype)


def _relative_map(dim):
  """[dim, nodes] multiples of 1/8; every channel's absolute nodes leave the image on
  both sides."""
  rng = np.random.default_rng(77 + dim)
  rel = rng.integers(-32, 33, (dim,) + NODES[dim]) / 8.0
  nodes = np.mgrid[tuple(slice(0, n) for n in NODES[dim])]
  for c in range(dim):
    axis = dim - 1 - c
    absolute = rel[c] + nodes[axis] * STRIDES[dim][axis]
    assert absolute.min() < 0 and absolute.max() > SHAPES[dim][axis] - 1, (dim, c)
    assert np.array_equal(absolute.astype(np.float16), absolute)
  return rel


def _affine(dim):
  """(matrix, offset) whose coordinates leave the image on both sides of every axis."""
  rng = np.random.default_rng(55 + dim)
  matrix = 2.5 * np.eye(dim) + rng.uniform(-0.1, 0.1, (dim, dim))
  offset = rng.uniform(-1.5, -1.0, dim)
  corners = np.array(list(itertools.product(*[(0, n - 1) for n in SHAPES[dim]]))).T
  coords = matrix @ corners + offset[:, None]
  for axis in range(dim):
    assert coords[axis].min() < 0 and coords[axis].max() > SHAPES[dim][axis] - 1
  return matrix, offset


def _sampler(boundary):
  if BOUNDARIES[boundary] is None:
    return None
  mode, cval = BOUNDARIES[boundary]
  return functools.partial(scipy.ndimage.map_coordinates, mode=mode, cval=cval)


@functools.lru_cache(maxsize=None)
def warp_reference(dim, dtype, order, boundary):
  mode, cval = BOUNDARIES[boundary] or ('constant', 0.0)
  return ref.ndimage_warp_scipy(_image(dim, dtype), _relative_map(dim), STRIDES[dim], order, mode,
                                cval)


@functools.lru_cache(maxsize=None)
def affine_reference(dim, dtype, order, boundary):
  mode, cval = BOUNDARIES[boundary] or ('constant', 3.5)
  matrix, offset = _affine(dim)
  return scipy.ndimage.affine_transform(_image(dim, dtype), matrix, offset, order=order,
                                        mode=mode, cval=cval)


def assert_same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


def assert_orders_differ(results, msg):
  for lo, hi in zip(ORDERS, ORDERS[1:]):
    assert (results[lo] != results[hi]).any(), (msg, lo, hi)


@pytest.fixture
def spline_switches(gpu):
  with _abi.option(_spline.OPTION, 1), _abi.option(_spline.MODES_OPTION, 1):
    yield


def test_the_references_tell_the_entries_apart():
  """On SciPy's results alone: neighbouring orders differ, every boundary class differs
  from every other, and the 2-D and the 3-D images are not the same."""
  for dtype in DTYPES:
    assert not np.array_equal(_image(2, dtype), _image(3, dtype)[0])
    for dim, reference in itertools.product((2, 3), (warp_reference, affine_reference)):
      for boundary in BOUNDARIES:
        assert_orders_differ({o: reference(dim, dtype, o, boundary) for o in ORDERS},
                             (reference.__name__, dim, dtype, boundary))
      for order in ORDERS:
        for a, b in itertools.combinations(BOUNDARIES, 2):
          assert (reference(dim, dtype, order, a) != reference(dim, dtype, order, b)).any(), (
              reference.__name__, dim, dtype, order, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('dim', [2, 3])
def test_ndimage_warp_entries(spline_switches, dim, order):
  rel = _relative_map(dim)
  for dtype, boundary, map_dtype in itertools.product(DTYPES, BOUNDARIES, MAP_DTYPES):
    got = warp.ndimage_warp(_image(dim, dtype), rel.astype(map_dtype), STRIDES[dim],
                            SHAPES[dim][::-1], (0,) * dim, order=order,
                            map_coordinates=_sampler(boundary))
    assert_same(got, warp_reference(dim, dtype, order, boundary),
                (np.dtype(dtype).name, boundary, np.dtype(map_dtype).name))


@pytest.mark.gpu
@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('dim', [2, 3])
def test_affine_transform_entries(spline_switches, dim, order):
  matrix, offset = _affine(dim)
  for dtype, boundary in itertools.product(DTYPES, BOUNDARIES):
    mode, cval = BOUNDARIES[boundary] or ('constant', 3.5)
    got = warp.affine_transform(_image(dim, dtype), matrix, offset, order=order, mode=mode,
                                cval=cval)
    assert_same(got, affine_reference(dim, dtype, order, boundary),
                (np.dtype(dtype).name, boundary))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
def test_render_entries(spline_switches, dtype):
  """Two tiles of (4, 8, 8) side by side, 4 voxels of overlap, one plan of two items;
  orders 0 to 5, output in the tiles' dtype and in float32."""
  from tests.test_gpu_render3d import grid_montage
  m = grid_montage(90 + np.dtype(dtype).itemsize, (4, 8, 8), (2, 4, 4), (1, 2), 4, dtype=dtype)
  b = box((-1, -1, 0), (14, 10, 4))
  plan = processor_warp.plan_render(b, m['boxes'], m['inverted'], m['xy'], m['tile_shape'],
                                    m['stride'])
  assert [item[0] for item in plan] == [0, 1]
  args = (b, m['tiles'], plan, m['inverted'], m['weights'], m['stride'])
  for out_dtype in (None, np.float32):
    want = {order: spline_ref.render(*args, order, out_dtype) for order in ORDERS}
    assert_orders_differ(want, (np.dtype(dtype).name, out_dtype))
    for order in ORDERS:
      got = np.asarray(processor_warp.render(*args, order=order, out_dtype=out_dtype))
      assert_same(got, want[order], (np.dtype(dtype).name, out_dtype, order))
