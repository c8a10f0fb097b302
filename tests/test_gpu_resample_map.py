"""map_utils.resample_map on the device: the contract against goldens of the
unmodified reference, affine data, the smallest shapes, the directions, NaN
handling, a SciPy fuzz, refusals and the methods that are not built.

The contract (tests/resample_map_scipy.py): the device interpolates over one
Delaunay triangulation of the valid lattice nodes.  Its value is the
interpolant of an admissible triangle at every query of the hull, equals the
reference wherever all admissible triangles agree, and is NaN exactly outside
the hull.  float64 values are compared to 1e-6 (the figure of the same float64
barycentric gather in invert_map); a float32 result is the float64 result
rounded, bit for bit, and lies within one float32 ulp of the reference.
"""
import os

import numpy as np
import pytest
import torch

from sofima_amd import _abi, map_utils
from sofima_amd._dev import DeviceArray
from tests import resample_map_scipy as rms

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'resample_map.npz')
TOL = 1e-6


def golden_cases():
  g = np.load(GOLDEN)
  n = len([k for k in g.files if k.endswith('_name')])
  for i in range(n):
    k = f'{i:02d}'
    s = g[k + '_strides']
    yield (str(g[k + '_name']), g[k + '_map'], rms.box(*g[k + '_src']), rms.box(*g[k + '_dst']),
           float(s[0]), float(s[1]), g[k + '_out'])


def resample(cm, src, dst, s0, s1):
  out = map_utils.resample_map(cm, src, dst, s0, s1)
  assert isinstance(out, DeviceArray)
  return np.asarray(out)


def same_bits(a, b):
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def holes_8x10(cm):
  cm[:, :, 2:4, 3:6] = np.nan          # a block hole
  cm[:, :, 6:, 7:9] = np.nan           # a notch in the border
  cm[:, :, 5, 1] = cm[:, :, 0, 0] = cm[:, :, 4, 8] = np.nan
  return cm


# -- admissibility, over all goldens -----------------------------------------


@pytest.mark.parametrize('case', list(golden_cases()), ids=lambda c: c[0])
def test_golden_cases_meet_the_contract(case):
  name, cm, src, dst, s0, s1, want = case
  got = resample(cm, src, dst, s0, s1)
  assert got.dtype == cm.dtype and got.shape == want.shape
  assert same_bits(got, resample(cm, src, dst, s0, s1)), 'two calls differ'
  got64 = got if cm.dtype == np.float64 else resample(cm.astype(np.float64), src, dst, s0, s1)
  counts, single = rms.check_contract(cm, src, dst, s0, s1, got64, want, tol=TOL)
  # strides exact in binary: no query lies on the hull to rounding only
  assert counts['hull_exception'] == 0
  assert np.array_equal(np.isnan(got), np.isnan(want))
  if cm.dtype == np.float32:
    assert same_bits(got, got64.astype(np.float32))
    ulp = np.spacing(np.abs(want[:, single]))
    assert np.all(np.abs(got[:, single] - want[:, single]) <= ulp)
  if name not in ('dst_disjoint',):
    assert counts['single'] > 0


# -- affine values: any triangulation gives the same answer -------------------


def test_affine_values_match_everywhere_in_the_hull():
  rng = np.random.default_rng(3)
  yy, xx = np.mgrid[:8, :10]
  src = rms.box((-7, -4, 0), (10, 8, 1))
  dst = rms.box((-16, -10, 0), (23, 19, 1))
  a = rng.uniform(-1, 1, (2, 3))
  x, y = (xx + src.start[0]) * 2.0, (yy + src.start[1]) * 2.0
  cm = holes_8x10(np.stack([a[c, 0] + a[c, 1] * x + a[c, 2] * y for c in range(2)])[:, None])
  got = resample(cm, src, dst, 2, 1)
  want = rms.resample_restated(cm, src, dst, 2, 1)
  assert np.array_equal(np.isnan(got), np.isnan(want))
  inside = ~np.isnan(want[0, 0])
  # the hole interiors are in the hull: node (2, 4) of the block hole is query (6, 10)
  # (19 x 15 queries over the lattice, less the three the missing corner node cuts off)
  assert np.isnan(cm[0, 0, 2, 4]) and inside[6, 10] and inside.sum() == 19 * 15 - 3
  assert np.nanmax(np.abs(got - want)) <= TOL
  ty, tx = np.mgrid[:19, :23]
  qx, qy = (tx + dst.start[0]) * 1.0, (ty + dst.start[1]) * 1.0
  for c in range(2):
    exact = a[c, 0] + a[c, 1] * qx + a[c, 2] * qy
    assert np.max(np.abs(got[c, 0][inside] - exact[inside])) <= TOL


# -- smallest shapes ---------------------------------------------------------


def test_one_quad_takes_the_documented_diagonal():
  """[2, 1, 2, 2] -> 3 x 3: the corners are the nodes, the edge midpoints the
  means of their ends, and the centre lies on the diagonal from (0, 1) to
  (1, 0), the one the tie rule picks in a full lattice quad."""
  cm = np.array([[[[1.0, 2.0], [4.0, 8.0]]], [[[-1.0, 0.5], [0.25, 16.0]]]])
  b = rms.box((0, 0, 0), (2, 2, 1))
  got = resample(cm, b, rms.box((0, 0, 0), (3, 3, 1)), 2, 1)
  assert same_bits(got[:, :, ::2, ::2], cm)
  for c in range(2):
    v = cm[c, 0]
    assert got[c, 0, 0, 1] == (v[0, 0] + v[0, 1]) / 2 and got[c, 0, 1, 0] == (v[0, 0] + v[1, 0]) / 2
    assert got[c, 0, 2, 1] == (v[1, 0] + v[1, 1]) / 2 and got[c, 0, 1, 2] == (v[0, 1] + v[1, 1]) / 2
    assert got[c, 0, 1, 1] == (v[0, 1] + v[1, 0]) / 2
    assert got[c, 0, 1, 1] != (v[0, 0] + v[1, 1]) / 2


def test_fewer_than_three_nodes_and_lines_are_nan():
  one = resample(np.ones((2, 1, 1, 1)), rms.box((0, 0, 0), (1, 1, 1)),
                 rms.box((-1, -1, 0), (3, 3, 1)), 2, 2)
  assert one.shape == (2, 1, 3, 3) and np.isnan(one).all()
  cm = np.full((2, 2, 3, 3), np.nan)
  cm[:, 1, 0, 0] = cm[:, 1, 2, 1] = 1.0          # slice 0: no node, slice 1: two nodes
  b = rms.box((0, 0, 0), (3, 3, 2))
  assert np.isnan(resample(cm, b, b, 1, 1)).all()
  rng = np.random.default_rng(0)
  for shape in ((2, 3, 1, 9), (2, 3, 9, 1)):
    cm = rng.uniform(-1, 1, shape)
    src = rms.box((0, 0, 0), shape[:0:-1])
    dst = rms.box((-1, -1, 0), (2 * shape[3] + 1, 2 * shape[2] + 1, shape[1]))
    out = resample(cm, src, dst, 2, 1)
    assert out.shape == (2, 3, 2 * shape[2] + 1, 2 * shape[3] + 1) and np.isnan(out).all()


def test_three_corner_cell():
  cm = np.array([[[[1.0, 3.0], [7.0, np.nan]]], [[[2.0, -1.0], [0.5, 9.0]]]])
  b = rms.box((0, 0, 0), (2, 2, 1))
  got = resample(cm, b, rms.box((0, 0, 0), (5, 5, 1)), 2, 0.5)
  ty, tx = np.mgrid[:5, :5] / 4.0
  inside = tx + ty <= 1
  assert np.array_equal(~np.isnan(got[0, 0]), inside) and np.array_equal(~np.isnan(got[1, 0]), inside)
  for c in range(2):
    v = cm[c, 0]
    plane = v[0, 0] + (v[0, 1] - v[0, 0]) * tx + (v[1, 0] - v[0, 0]) * ty
    assert np.max(np.abs(got[c, 0][inside] - plane[inside])) <= 1e-12


@pytest.mark.parametrize('shape', [(2, 37, 5, 7), (2, 300, 3, 3)])
def test_slices_that_share_waves_equal_themselves_alone(shape):
  """Empty, collinear and holed slices among their neighbours in one wave; a
  refused slice is out of reach at these sizes (see the boundary-cap test)."""
  rng = np.random.default_rng(shape[1])
  z, h, w = shape[1:]
  cm = rng.uniform(-2, 2, shape)
  cm[:, rng.random((z, h, w)) < 0.2] = np.nan
  cm[:, 3] = np.nan                                # an empty slice
  cm[:, 5] = np.nan
  cm[:, 5, 1, :] = 1.0                             # a line
  cm[1, 7, 0, 0] = np.nan                          # channel 1 alone
  src = rms.box((1, 2, 0), (w, h, z))
  dst = rms.box((1, 3, 0), (2 * w + 1, 2 * h, z))
  whole = resample(cm, src, dst, 2, 1)
  assert np.isnan(whole[:, 3]).all() and np.isnan(whole[:, 5]).all()
  assert np.isfinite(whole[0]).any(axis=(1, 2)).sum() > z // 2
  src1 = rms.box(src.start, (w, h, 1))
  dst1 = rms.box(dst.start, dst.size[:2] + (1,))
  for k in range(z):
    alone = resample(cm[:, k:k + 1], src1, dst1, 2, 1)
    assert same_bits(alone[:, 0], whole[:, k]), f'slice {k}'


# -- directions ---------------------------------------------------------------


def test_downsampling_returns_the_coinciding_nodes():
  rng = np.random.default_rng(1)
  cm = rng.uniform(-5, 5, (2, 1, 9, 9))
  got = resample(cm, rms.box((0, 0, 0), (9, 9, 1)), rms.box((0, 0, 0), (5, 5, 1)), 1, 2)
  assert same_bits(got, cm[:, :, ::2, ::2])
  got32 = resample(cm.astype(np.float32), rms.box((0, 0, 0), (9, 9, 1)),
                   rms.box((0, 0, 0), (5, 5, 1)), 1, 2)
  assert same_bits(got32, cm.astype(np.float32)[:, :, ::2, ::2])


def test_golden_directions_are_present():
  """Strides 3 -> 2 and 2.5 -> 1 with odd starts (queries strictly inside
  cells) and a dst box larger, smaller and disjoint from the hull run as golden
  cases above."""
  names = {c[0] for c in golden_cases()}
  assert {'stride_3_to_2', 'stride_2p5_to_1', 'up2_holes', 'dst_smaller',
          'dst_disjoint'} <= names


def test_empty_dst_box():
  cm = np.zeros((2, 3, 4, 5), np.float32)
  out = map_utils.resample_map(cm, rms.box((0, 0, 0), (5, 4, 3)), rms.box((0, 0, 0), (0, 7, 3)),
                               2, 1)
  assert out.shape == (2, 3, 7, 0) and out.dtype == np.float32


def test_stride_that_is_not_exact_in_binary():
  """Stride 0.1 -> 0.05: positions and queries round differently, so a query on
  the hull may fall on either side (the hull exception, 1e-7 * stride)."""
  rng = np.random.default_rng(4)
  cm = holes_8x10(rng.uniform(-3, 3, (2, 1, 8, 10)))
  src = rms.box((3, 5, 0), (10, 8, 1))
  dst = rms.box((4, 8, 0), (23, 19, 1))
  got = resample(cm, src, dst, 0.1, 0.05)
  want = rms.resample_restated(cm, src, dst, 0.1, 0.05)
  counts, _ = rms.check_contract(cm, src, dst, 0.1, 0.05, got, want, tol=TOL)
  assert counts['in_hull'] > 200 and counts['single'] > 100


# -- NaN handling --------------------------------------------------------------


def test_nan_in_channel_1_propagates_and_leaves_channel_0_alone():
  rng = np.random.default_rng(6)
  clean = rng.uniform(-3, 3, (2, 1, 8, 10))
  cm = clean.copy()
  cm[1, 0, 4, 5] = np.nan
  src = rms.box((0, 0, 0), (10, 8, 1))
  dst = rms.box((0, 0, 0), (19, 15, 1))
  got, base = resample(cm, src, dst, 2, 1), resample(clean, src, dst, 2, 1)
  assert same_bits(got[0], base[0])
  assert not np.isnan(base).any()
  nan = np.isnan(got[1, 0])
  assert nan[8, 10]                                # the node itself
  ty, tx = np.mgrid[:15, :19]
  near = (np.abs(ty - 8) <= 2) & (np.abs(tx - 10) <= 2)
  assert not nan[~near].any()                      # only triangles that have the node
  assert same_bits(got[1, 0][~nan], base[1, 0][~nan])
  # what SciPy does with the same map: the NaN reaches every query of a
  # triangle that has the node, zero weights included
  want = rms.resample_restated(cm, src, dst, 2, 1)
  assert np.isnan(want[1, 0, 8, 10]) and not np.isnan(want[1, 0][~near]).any()


def test_inf_in_channel_0_is_an_invalid_node():
  rng = np.random.default_rng(7)
  cm = rng.uniform(-3, 3, (2, 1, 6, 7))
  a, b = cm.copy(), cm.copy()
  a[0, 0, 2, 3], a[0, 0, 0, 0], a[0, 0, 5, 2] = np.inf, -np.inf, np.inf
  b[0, 0, 2, 3] = b[0, 0, 0, 0] = b[0, 0, 5, 2] = np.nan
  src = rms.box((0, 0, 0), (7, 6, 1))
  dst = rms.box((0, 0, 0), (13, 11, 1))
  got = resample(a, src, dst, 2, 1)
  assert same_bits(got, resample(b, src, dst, 2, 1))
  assert np.isfinite(got[~np.isnan(got)]).all()
  want = rms.resample_restated(a, src, dst, 2, 1)
  assert np.array_equal(np.isnan(got), np.isnan(want))


@pytest.mark.parametrize('kind', ['numpy32', 'numpy64', 'torch32', 'torch64', 'device'])
def test_input_kinds_and_input_untouched(kind):
  rng = np.random.default_rng(5)
  cm = holes_8x10(rng.uniform(-3, 3, (2, 2, 8, 10)))
  src = rms.box((3, 5, 0), (10, 8, 2))
  dst = rms.box((4, 8, 0), (23, 19, 2))
  dtype = np.float32 if kind.endswith('32') else np.float64
  host = cm.astype(dtype)
  if kind.startswith('numpy'):
    x = host.copy()
  elif kind.startswith('torch'):
    x = torch.from_numpy(host).cuda()
  else:
    x = DeviceArray(torch.from_numpy(host).cuda())
  out = map_utils.resample_map(x, src, dst, 2, 1)
  assert isinstance(out, DeviceArray) and out.dtype == dtype and out.tensor.is_cuda
  after = x if kind.startswith('numpy') else np.asarray(x.cpu() if kind.startswith('torch') else x)
  assert same_bits(after, host)
  assert same_bits(np.asarray(out), resample(host, src, dst, 2, 1))
  # a DeviceArray result goes back in
  again = map_utils.resample_map(out, dst, dst, 1, 1)
  assert same_bits(np.asarray(again)[0], np.asarray(out)[0])


# -- fuzz at the seeds and shapes of the invert_map fuzz -------------------------


@pytest.mark.parametrize('seed,shape,holes,max_rest', [(0, (1, 101, 101), 0.0, 0.0),
                                                      (1, (4, 96, 96), 0.05, 0.15),
                                                      (2, (2, 64, 80), 0.1, 0.15)])
def test_scipy_fuzz(seed, shape, holes, max_rest):
  from scipy import ndimage
  rng = np.random.default_rng(seed)
  z, h, w = shape
  cm = np.stack([ndimage.gaussian_filter(rng.standard_normal(shape), (0, 5, 5))
                 for _ in range(2)])
  cm = cm / np.abs(cm).max() * 24.0
  if holes:
    noise = ndimage.gaussian_filter(rng.standard_normal(shape), (0, 1.5, 1.5))
    cm[:, noise > np.quantile(noise, 1 - holes)] = np.nan
  src = rms.box((7, 3, 0), (w, h, z))
  dst = rms.box((14, 6, 0), (2 * w - 1, 2 * h - 1, z))
  got = resample(cm, src, dst, 2, 1)
  want = rms.resample_restated(cm, src, dst, 2, 1)
  assert np.array_equal(np.isnan(got), np.isnan(want))
  assert np.array_equal(np.isnan(got[0]), np.isnan(got[1]))
  assert np.isfinite(got[~np.isnan(got)]).all()
  valid = np.isfinite(cm[0])
  full = valid[:, :-1, :-1] & valid[:, :-1, 1:] & valid[:, 1:, :-1] & valid[:, 1:, 1:]
  # closed full cells on the query lattice: a query at (2 i + a, 2 j + b) with
  # a, b in 0 .. 2 lies in the closed cell (i, j)
  closed = np.zeros((z, 2 * h - 1, 2 * w - 1), bool)
  for a in range(3):
    for b in range(3):
      closed[:, a:a + 2 * h - 2:2, b:b + 2 * w - 2:2] |= full
  ty, tx = np.mgrid[:2 * h - 1, :2 * w - 1]
  centre = (ty % 2 == 1) & (tx % 2 == 1)
  shared = closed & ~centre[None]                  # nodes and edges of full cells
  assert not np.isnan(got[0][closed]).any()
  assert np.max(np.abs(got[:, shared] - want[:, shared])) <= TOL
  assert same_bits(got[:, :, ::2, ::2][:, valid & closed[:, ::2, ::2]],
                   cm[:, valid & closed[:, ::2, ::2]])
  v = cm
  bd = (v[:, :, :-1, 1:] + v[:, :, 1:, :-1]) / 2    # the diagonal (i, j + 1) - (i + 1, j)
  ac = (v[:, :, :-1, :-1] + v[:, :, 1:, 1:]) / 2
  inner, ref_inner = got[:, :, 1::2, 1::2], want[:, :, 1::2, 1::2]
  assert np.max(np.abs(inner[:, full] - bd[:, full])) <= TOL
  on_bd = np.max(np.abs(ref_inner[:, full] - bd[:, full]), axis=0) <= TOL
  on_ac = np.max(np.abs(ref_inner[:, full] - ac[:, full]), axis=0) <= TOL
  assert np.all(on_bd | on_ac), 'the reference leaves the two diagonals of a full cell'
  in_hull = ~np.isnan(want[0])
  rest = (in_hull & ~closed).sum() / in_hull.sum()
  print(f'seed {seed}: {rest:.4f} of the in-hull queries outside closed full cells')
  assert rest <= max_rest


# -- refusal and unsupported methods ---------------------------------------------


def _checkerboard(n):
  yy, xx = np.mgrid[:n, :n]
  return (yy + xx) % 2 == 1


def test_boundary_cap_is_refused_and_names_the_slice():
  """A refusal needs more than 7936 boundary nodes in one slice, so it cannot
  happen at the shapes where slices share waves ([2, 37, 5, 7], [2, 300, 3, 3]:
  those cover empty and collinear slices among their neighbours).  Here a
  refused slice of 130 x 130 sits between two answered ones, which must equal
  themselves alone bit for bit."""
  # a checkerboard of NaN leaves no full quad: every valid node is a boundary node
  n = 130
  rng = np.random.default_rng(8)
  cm = rng.uniform(-1, 1, (2, 3, n, n))
  cm[:, 1, _checkerboard(n)] = np.nan
  assert np.isfinite(cm[0, 1]).sum() > 7936
  src = rms.box((0, 0, 0), (n, n, 3))
  dst = rms.box((0, 0, 0), (2 * n - 1, 2 * n - 1, 3))
  with pytest.raises(_abi.SofimaAmdError, match='resample_map: slice 1 refused.*7936 boundary'):
    map_utils.resample_map(cm, src, dst, 2, 1)
  # its neighbours are answered as they are alone
  out, status = map_utils._resample_launch(cm, src, dst, 2.0, 1.0)
  assert status.cpu().tolist() == [0, 4, 0]
  out = out.cpu().numpy()
  for k in (0, 2):
    alone = resample(cm[:, k:k + 1], rms.box((0, 0, 0), (n, n, 1)),
                     rms.box((0, 0, 0), (2 * n - 1, 2 * n - 1, 1)), 2, 1)
    assert same_bits(alone[:, 0], out[:, k])


def test_box_starts_beyond_32_bits_are_rejected():
  cm = np.zeros((2, 1, 4, 4))
  b = rms.box((0, 0, 0), (4, 4, 1))
  with pytest.raises(ValueError, match='32 bits'):
    map_utils.resample_map(cm, rms.box((2**31, 0, 0), (4, 4, 1)), b, 1, 1)
  with pytest.raises(ValueError, match='32 bits'):
    map_utils.resample_map(cm, b, rms.box((0, -2**31 - 1, 0), (4, 4, 1)), 1, 1)


@pytest.mark.parametrize('method', ['nearest', 'cubic'])
def test_other_methods_are_not_implemented(method):
  b = rms.box((0, 0, 0), (4, 4, 1))
  with pytest.raises(NotImplementedError, match=method):
    map_utils.resample_map(np.zeros((2, 1, 4, 4)), b, b, 1, 1, method=method)
