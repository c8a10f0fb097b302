"""The per-element formula that `sfm_ndimage_warp_rel` reads a relative map with equals
the reference's array statements bit for bit (no GPU): float32 and float64 maps, 2-D
and 3-D, strides as Python ints, Python floats and NumPy float32 scalars, with and
without boxes, a non-trivial out_scale.  And the roundings it pins are visible: the
all-double variant differs."""
import itertools

import numpy as np
import pytest

from tests import ndwarp_rel_ref as ref

STRIDES = {
    2: [(3, 5), (10.3, 9.7), (np.float32(2.3), np.float32(7.1)), (4, 2.5)],
    3: [(2, 3, 5), (3.1, 6.3, 5.9), (np.float32(1.7), np.float32(2.3), np.float32(7.1)),
        (1, 4.25, 2)],
}
SHAPES = {2: (7, 9), 3: (4, 5, 6)}
SCALES = [(1.0, 1.0, 1.0), (2.0, 0.7, 1.3), (2, 2, 1)]
BOXES = [None, ((1000, 1000, 1000), (0, 0, 0)), ((37, -12, 5), (3, -2, 1)), ((0, 0, 0), (0, 0, 0))]


def same_bits(a, b):
  return a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def relative_map(rng, dim, dtype, big=False):
  m = rng.uniform(-2.0, 2.0, (dim,) + SHAPES[dim])
  m.flat[::7] = -0.0                      # the sign of a zero sum is part of the statement
  m.flat[3::11] = np.nan
  return ((1000.0 + m) if big else m).astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('dim', [2, 3])
def test_per_element_formula_equals_the_array_statements(dim, dtype):
  rng = np.random.default_rng(10 * dim + np.dtype(dtype).itemsize)
  for stride, scale, box, big in itertools.product(STRIDES[dim], SCALES, BOXES, (False, True)):
    cmap = relative_map(rng, dim, dtype, big)
    kw = {}
    if box is not None:
      kw = dict(image_start=np.array(box[0][:dim]), map_start=np.array(box[1][:dim]))
    want = ref.absolute_map_statements(cmap, stride, out_scale=scale, **kw)
    got = ref.absolute_map_per_element(cmap, stride, out_scale=scale, **kw)
    assert same_bits(got, want), (stride, scale, box, big)


@pytest.mark.parametrize('dim', [2, 3])
def test_the_roundings_are_visible_in_float32(dim):
  """Nodes near 1000 with fractional strides: storing as float32 twice is not the
  all-double sum on most elements; for a float64 map the two agree wherever double
  addition happens to associate."""
  rng = np.random.default_rng(dim)
  stride = STRIDES[dim][1]
  cmap = relative_map(rng, dim, np.float32, big=True)
  cmap[np.isnan(cmap)] = 1000.0
  kw = dict(image_start=np.full(dim, 1000), map_start=np.zeros(dim, np.int64))
  exact = ref.absolute_map_per_element(cmap, stride, **kw)
  naive = ref.absolute_map_per_element(cmap, stride, naive=True, **kw)
  assert np.mean(exact != naive) > 0.5
  assert same_bits(exact, ref.absolute_map_statements(cmap, stride, **kw))
