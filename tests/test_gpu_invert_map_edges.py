"""map_utils.invert_map at its boundaries: waves shared by several slices,
the |B| cap, the node-id width, degenerate slices, per-slice status, non-finite
and huge values, the query lattice and workspace reuse.  The cases and their
host references live in tests/invmap_cases.py (checked on the host by
tests/test_invert_map_cases.py)."""
import numpy as np
import pytest
import torch

from sofima_amd import _abi, map_utils
from tests import invert_map_scipy as ims
from tests import invmap_cases as ic

pytestmark = pytest.mark.gpu

_reference = {}


def reference(name):
  """invert_restated of a case, computed once and read-only."""
  if name not in _reference:
    _, cm, src, dst, stride, _ = ic.case(name)
    want = ims.invert_restated(cm, src, dst, stride)
    want.setflags(write=False)
    _reference[name] = want
  return _reference[name]


def invert(cm, src, dst, stride):
  if isinstance(cm, np.ndarray) and not cm.flags.writeable:
    cm = cm.copy()  # the cases are read-only; the upload wants a writable array
  return np.asarray(map_utils.invert_map(cm, src, dst, stride))


def bits_equal(a, b):
  a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
  return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def meets_contract_exactly(name, got):
  """The contract with neither exception used."""
  _, cm, src, dst, stride, _ = ic.case(name)
  counts = ims.check_contract_counts(cm, src, dst, stride, got, reference(name))
  assert counts == (0, 0), f'{name}: (diagonal exceptions, mask mismatches) = {counts}'


# ---------------------------------------------------------------- shared waves


@pytest.mark.parametrize('name', ['waves_37x5x7', 'waves_300x3x3', 'waves_5x2x40'])
def test_waves_shared_by_slices(name):
  """H * W (or the quads of a slice) below a wave, so the per-lane atomics of
  prep and quad run; Z > 256 reaches the second init workgroup."""
  _, cm, src, dst, stride, _ = ic.case(name)
  got = invert(cm, src, dst, stride)
  meets_contract_exactly(name, got)
  claim = ic.CLAIMS[name]
  for k in range(cm.shape[1]):
    if claim['degenerate'][k]:
      assert np.isnan(got[:, k]).all(), f'slice {k} is degenerate and must be NaN'
      continue
    s1 = ims.box(src.start, src.size[:2] + (1,))
    d1 = ims.box(dst.start, dst.size[:2] + (1,))
    alone = invert(cm[:, k:k + 1], s1, d1, stride)
    assert bits_equal(got[:, k:k + 1], alone), f'slice {k} differs from the slice alone'


@pytest.mark.parametrize('name', ic.names_expecting('all_nan'))
def test_all_nan_cases(name):
  """Single rows and columns (no quad, collinear) and dst boxes 100000 nodes
  away from the map on each side."""
  _, cm, src, dst, stride, _ = ic.case(name)
  got = invert(cm, src, dst, stride)
  assert got.shape == (2, cm.shape[1], dst.size[1], dst.size[0])
  assert np.isnan(got).all()


def test_four_isolated_cocircular_nodes():
  """R is empty and the in-circle tie of the completion is broken symbolically;
  either diagonal interpolates the same identity."""
  name = 'four_cocircular_5_5'
  _, cm, src, dst, stride, _ = ic.case(name)
  got = invert(cm, src, dst, stride)
  meets_contract_exactly(name, got)
  # the identity, to the rounding of three barycentric weights
  assert np.abs(got[:, 0, 1:7, 1:7]).max() <= 64 * np.spacing(7.0 * stride)
  outside = np.ones((8, 8), bool)
  outside[1:7, 1:7] = False
  assert np.isnan(got[:, 0, outside]).all()


def test_dense_coincident_slice_is_refused_by_name():
  """Every node of a slice at one position: every quad is degenerate, so the
  slice is refused as folded (the sparse kind, with no full quad, is NaN; see
  the mixes of test_waves_shared_by_slices).  The verification of a refused
  slice may add reasons of its own after the first."""
  s = ic.STRIDE
  yy, xx = np.mgrid[:5, :7]
  cm = np.zeros((2, 3, 5, 7))
  cm[0, 1] = 101.25 - xx * s
  cm[1, 1] = 57.75 - yy * s
  b = ims.box((0, 0, 0), (7, 5, 3))
  with pytest.raises(_abi.SofimaAmdError,
                     match=r'^invert_map: slice 1 refused: folded or degenerate quad[^()]*$'):
    map_utils.invert_map(cm, b, b, s)


# ------------------------------------------------------- cap and node-id width


def check_affine(name, got):
  """Returns the largest error inside the hull; asserts the tolerance and the
  NaN mask."""
  _, cm, src, dst, stride, _ = ic.case(name)
  claim = ic.CLAIMS[name]
  want = ic.affine_inverse(claim['A'], claim['t'], src, dst, stride)
  assert got.shape == want.shape and got.dtype == np.float64
  valid = ic.valid_nodes(cm, src, dst, stride)[0]
  pts = ic.affine_points(claim['A'], claim['t'], valid, src, stride)
  side = ic.in_hull(pts, ic.dst_queries(dst, stride), 1e-7 * stride).reshape(want.shape[2:])
  nan = np.isnan(got[0, 0])
  assert np.array_equal(nan, np.isnan(got[1, 0]))
  assert not nan[side > 0].any(), f'{int(nan[side > 0].sum())} NaN inside the hull'
  assert nan[side < 0].all(), f'{int((~nan[side < 0]).sum())} values outside the hull'
  err = float(np.abs(got[:, 0] - want[:, 0])[:, side > 0].max())
  tol = ic.affine_tolerance(name, claim['max_coord'])
  print(f'{name}: device max error {err:.3e} px, tolerance {tol:.3e} px')
  assert err <= tol
  return err


@pytest.mark.parametrize('name', ['affine_small_holes', 'cap_strip_7936', 'cap_band_7936',
                                  'cap_strip_two_holes_7936'])
def test_cap_accepted_side(name):
  """Exactly 7936 boundary nodes (and a small map for scale), against the
  analytic inverse of the affine map."""
  _, cm, src, dst, stride, _ = ic.case(name)
  valid = ic.valid_nodes(cm, src, dst, stride)[0]
  if name.startswith('cap'):
    assert ic.boundary_count(valid) == ic.MAX_B
  check_affine(name, invert(cm, src, dst, stride))


def test_cap_refused_side():
  name = 'cap_strip_one_hole_7937'
  _, cm, src, dst, stride, expect = ic.case(name)
  assert ic.boundary_count(ic.valid_nodes(cm, src, dst, stride)[0]) == ic.MAX_B + 1
  with pytest.raises(_abi.SofimaAmdError, match=expect[1]):
    invert(cm, src, dst, stride)


def test_largest_slice_and_node_ids_near_the_width():
  """H * W == 2^21 with pockets at node ids near 0 and just under 2^21."""
  name = 'nodeid_2p21'
  _, cm, src, dst, stride, _ = ic.case(name)
  assert cm.shape[2] * cm.shape[3] == 1 << ic.NODE_BITS
  check_affine(name, invert(cm, src, dst, stride))


def test_slice_above_the_width_is_refused_before_any_launch():
  _, cm, src, dst, stride, expect = ic.case('nodeid_over_2p21')
  with pytest.raises(_abi.SofimaAmdError, match=expect[1]):
    invert(cm, src, dst, stride)


# ------------------------------------------------------------ per-slice status


def test_status_names_exactly_the_refused_slices():
  name = 'status_fold_1_4'
  _, cm, src, dst, stride, expect = ic.case(name)
  with pytest.raises(_abi.SofimaAmdError, match=expect[1]):
    invert(cm, src, dst, stride)
  fixed = cm.copy()
  for k in (1, 4):
    sl = np.ascontiguousarray(fixed[:, k])
    assert map_utils.mask_irregular(sl, (stride, stride), 0.5).any()
    fixed[:, k] = sl
  for k in (0, 3):
    assert np.array_equal(fixed[:, k], cm[:, k])
  got = invert(fixed, src, dst, stride)
  want = ims.invert_restated(fixed, src, dst, stride)
  ims.check_contract(fixed, src, dst, stride, got, want)
  assert np.isnan(got[:, 2]).all()
  for k in (0, 1, 3, 4):
    assert np.isfinite(got[:, k]).any()


def test_status_names_each_reason_on_its_slice():
  _, cm, src, dst, stride, expect = ic.case('status_cap_1_fold_2')
  with pytest.raises(_abi.SofimaAmdError, match=expect[1]):
    invert(cm, src, dst, stride)


# ---------------------------------------------------- non-finite, huge, layout


@pytest.mark.parametrize('name', ['hole_posinf_x', 'hole_neginf_y', 'hole_nan_x'])
def test_non_finite_in_one_channel_is_a_hole(name):
  _, cm, src, dst, stride, _ = ic.case(name)
  got = invert(cm, src, dst, stride)
  meets_contract_exactly(name, got)
  hole = cm.copy()
  hole[:, 0, 5, 6] = np.nan
  assert bits_equal(got, invert(hole, src, dst, stride))


def test_node_of_1e300_refuses_its_slice():
  """Outcome: refused, naming the slice.  The slice's exponent (set by 1e300)
  rounds every other node to one grid point, so every quad is degenerate.
  Qhull fails on the same points (the restatement is all NaN there), so there
  is no triangulation to agree with; the good slice beside it is not named."""
  _, cm, src, dst, stride, expect = ic.case('huge_1e300')
  want = ims.invert_restated(cm, src, dst, stride)
  assert np.isnan(want[:, 1]).all() and np.isfinite(want[:, 0]).any()
  with pytest.raises(_abi.SofimaAmdError, match=expect[1]):
    invert(cm, src, dst, stride)


def test_overflowing_position_is_a_hole():
  """rel + offset overflows to inf although rel is finite: 1.7e308 + 7 * 2^1019.
  Only a stride of this size can overflow a finite float64, and at this size
  the interpolation itself overflows, so the values are compared with those of
  the same map with a NaN at that node, not with a reference."""
  stride = 2.0**1019
  cm = np.zeros((2, 1, 8, 8))
  cm[0, 0, 4, 7] = 1.7e308
  with np.errstate(over='ignore'):
    assert np.isfinite(cm).all() and np.isinf(cm[0, 0, 4, 7] + 7 * stride)
  b = ims.box((0, 0, 0), (8, 8, 1))
  got = invert(cm, b, b, stride)
  hole = cm.copy()
  hole[:, 0, 4, 7] = np.nan
  assert bits_equal(got, invert(hole, b, b, stride))


def test_non_contiguous_float32_view_gives_the_same_bits():
  _, cm, src, dst, stride, _ = ic.case('reuse_B_20x3')
  wide = torch.from_numpy(np.ascontiguousarray(
      np.repeat(cm.astype(np.float32), 2, axis=3))).cuda()
  view = wide[..., ::2]
  assert not view.is_contiguous()
  a = invert(view, src, dst, stride)
  c = invert(view.contiguous(), src, dst, stride)
  assert bits_equal(a, c)
  assert bits_equal(a, invert(cm.astype(np.float32), src, dst, stride))


# ------------------------------------------------------------- query lattice


@pytest.mark.parametrize('size', [(0, 5), (5, 0), (0, 0)])
def test_empty_dst_box(size):
  """dst size (x, y); the result is [2, z, dst y, dst x]."""
  _, cm, src, _, stride, _ = ic.case('reuse_B_20x3')
  dst = ims.box((6, 2, 0), size + (3,))
  got = invert(cm, src, dst, stride)
  assert got.shape == (2, 3, size[1], size[0]) and got.dtype == np.float64


def test_empty_dst_box_still_reports_a_fold():
  _, cm, src, _, stride, expect = ic.case('status_fold_1_4')
  dst = ims.box((0, 0, 0), (0, 5, 5))
  with pytest.raises(_abi.SofimaAmdError, match=expect[1]):
    invert(cm, src, dst, stride)


def test_anisotropic_lattice_that_is_not_delaunay_is_refused_by_name():
  """At strides (0.3, 2.5) a deformation of 0.3 x stride makes Delaunay edges
  that leave the lattice quads (the node two rows on is nearer than the next
  column); the flips that would repair it are not built, so it is refused."""
  _, cm, src, dst, stride, expect = ic.case('stride_0.3_2.5_rough')
  assert np.isfinite(ims.invert_restated(cm, src, dst, stride)).any()
  with pytest.raises(_abi.SofimaAmdError, match=expect[1]):
    invert(cm, src, dst, stride)


@pytest.mark.parametrize('name', ['stride_0.5_0.5', 'stride_0.3_2.5', 'stride_30.5_29.25'])
def test_fractional_strides_with_negative_source_coordinates(name):
  _, cm, src, dst, stride, _ = ic.case(name)
  got = invert(cm, src, dst, stride)
  ims.check_contract(cm, src, dst, stride, got, reference(name))
  assert np.isfinite(got).sum() > got.size // 2


# ------------------------------------------------------------ workspace reuse


def test_workspace_reuse_keeps_every_result():
  """blist, tris, queue, bid and split are not cleared between calls: a large
  holey case, a smaller one, the first again, then the smaller one three
  slices deep."""
  a = ic.case('reuse_A_96')[1:5]
  b = ic.case('reuse_B_20')[1:5]
  b3 = ic.case('reuse_B_20x3')[1:5]
  first_a = invert(*a)
  first_b = invert(*b)
  meets_contract_exactly('reuse_A_96', first_a)
  meets_contract_exactly('reuse_B_20', first_b)
  for _ in range(2):
    assert bits_equal(invert(*a), first_a)
    assert bits_equal(invert(*b), first_b)
    assert bits_equal(invert(*a), first_a)
    got3 = invert(*b3)
    for k in range(3):
      assert bits_equal(got3[:, k:k + 1], first_b), k
