"""`warp.ndimage_warp`, `warp.affine_transform` and the decorator warps on resident
images and maps (-m gpu): CUDA tensors and DeviceArrays in, DeviceArrays out, and the
relative map read in its own dtype by `sfm_ndimage_warp_rel`.

Every comparison is bit for bit (`assert_same`): the reference's own outputs
(tests/golden), or the reference's NumPy statements for the absolute map followed by
scipy.ndimage.map_coordinates twice (`ndwarp_rel_ref.warp_scipy`,
`ndwarp_modes_ref.ndimage_warp_scipy`).  The double-rounding cases also build the
all-double variant of the map and require that the reference differs from it on most
outputs, so a kernel that skips a store-as-float32 step cannot pass.
"""
import contextlib
import functools
import types

import numpy as np
import pytest
import scipy.ndimage
import torch

from sofima_amd import _abi, _dev, _spline, decorators_warp, map_utils, warp
from tests import ndwarp_modes_ref as modes_ref
from tests import ndwarp_rel_ref as rel_ref
from tests import ndwarp_spline_ref as spline_ref
from tests.util import ndimage_warp_case

pytestmark = pytest.mark.gpu

ABSOLUTE_ENTRIES = ('sfm_ndimage_warp', 'sfm_ndimage_warp_spline', 'sfm_ndimage_warp_mode')


def assert_same(got, want, msg=''):
  assert got.dtype == want.dtype and got.shape == want.shape, msg
  if want.dtype.kind == 'f':
    differ = got.view(np.uint32) != want.view(np.uint32)
    assert not differ.any(), f'{msg}: {int(differ.sum())} of {differ.size} elements differ'
  else:
    np.testing.assert_array_equal(got, want, err_msg=str(msg))


def resident(a, dev):
  """A CUDA tensor of the array's dtype (uint16 uploaded through its int16 view)."""
  a = np.ascontiguousarray(a)
  if a.dtype == np.uint16:
    return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
  return torch.from_numpy(a).to(dev)


def host_of(result, dtype):
  """The contents of a DeviceArray result, which must be one of `dtype`."""
  assert isinstance(result, _dev.DeviceArray), type(result)
  assert result.dtype == np.dtype(dtype)
  assert result.tensor.is_contiguous()
  return np.asarray(result)


def box(start, size):
  return types.SimpleNamespace(start=np.asarray(start), size=np.asarray(size))


def sampler(mode, cval):
  return functools.partial(scipy.ndimage.map_coordinates, mode=mode, cval=cval)


@contextlib.contextmanager
def entries():
  """Counts the launches through the relative-map entry; the absolute-map entries
  raise while this is active."""
  lib = _abi.load()
  saved = {n: getattr(lib, n) for n in ABSOLUTE_ENTRIES + ('sfm_ndimage_warp_rel',)}
  calls = []

  def rel(desc):
    calls.append(1)
    return saved['sfm_ndimage_warp_rel'](desc)

  def absolute(*a):
    raise AssertionError('an absolute-map entry was called')

  try:
    lib.sfm_ndimage_warp_rel = rel
    for n in ABSOLUTE_ENTRIES:
      setattr(lib, n, absolute)
    yield calls
  finally:
    for n, f in saved.items():
      setattr(lib, n, f)


@contextlib.contextmanager
def no_host_copies():
  """torch.Tensor.cpu and DeviceArray.__array__ raise while this is active."""
  def refuse(*a, **k):
    raise AssertionError('a device-to-host copy was requested')
  saved = torch.Tensor.cpu, _dev.DeviceArray.__array__
  try:
    torch.Tensor.cpu = refuse
    _dev.DeviceArray.__array__ = refuse
    yield
  finally:
    torch.Tensor.cpu, _dev.DeviceArray.__array__ = saved


# -- the reference's own outputs ------------------------------------------------------------
def _golden_kw(boxes, scale=None):
  kw = {}
  if boxes is not None:
    kw = {k + '_box': box(boxes[k][0], boxes[k][1]) for k in ('image', 'map', 'out')}
  if scale is not None:
    kw['out_scale'] = scale
  return kw


def test_golden_cases_resident_and_host(gpu, golden):
  g = golden('ndimage_warp')
  for name in g['names']:
    img, cmap, stride, work, ov, order, boxes, scale, want = ndimage_warp_case(g, str(name))
    kw = _golden_kw(boxes, scale)
    with entries() as calls:
      got = warp.ndimage_warp(resident(img, gpu), resident(cmap, gpu), stride, work, ov,
                              order=order, device_output=True, **kw)
      assert_same(host_of(got, img.dtype), want, name)
      got = warp.ndimage_warp(img, cmap, stride, work, ov, order=order, **kw)
      assert isinstance(got, np.ndarray)
      assert_same(got, want, name)
      assert len(calls) == 2
    # the defaults follow the image, a DeviceArray is a resident input like a tensor
    got = warp.ndimage_warp(_dev.DeviceArray(resident(img, gpu)), cmap, stride, work, ov,
                            order=order, **kw)
    assert_same(host_of(got, img.dtype), want, name)
    got = warp.ndimage_warp(resident(img, gpu), _dev.DeviceArray(resident(cmap, gpu)), stride,
                            work, ov, order=order, device_output=False, **kw)
    assert isinstance(got, np.ndarray)
    assert_same(got, want, name)
    # a NumPy image with a resident float64 map: the widened map changes the reference
    wide = cmap.astype(np.float64)
    ref_kw = {} if scale is None else dict(out_scale=scale)
    if boxes is not None:
      ref_kw.update(image_start=boxes['image'][0], map_start=boxes['map'][0],
                    out_start=boxes['out'][0], out_shape=tuple(boxes['out'][1][::-1][-img.ndim:]))
    got = warp.ndimage_warp(img, resident(wide, gpu), stride, work, ov, order=order,
                            device_output=True, **kw)
    assert_same(host_of(got, img.dtype), rel_ref.warp_scipy(img, wide, stride, order=order,
                                                            **ref_kw), name)


def test_golden_spline_cases_resident_and_host(gpu, golden):
  with _abi.option(_spline.OPTION, 1):
    for c in spline_ref.warp_cases(golden('ndimage_warp_spline')):
      kw = _golden_kw(c['boxes'])
      args = (c['stride'], c['work'], c['overlap'])
      with entries() as calls:
        got = warp.ndimage_warp(resident(c['image'], gpu), resident(c['map'], gpu), *args,
                                order=c['order'], device_output=True, **kw)
        assert_same(host_of(got, c['image'].dtype), c['warped'], c['name'])
        got = warp.ndimage_warp(c['image'], c['map'], *args, order=c['order'], **kw)
        assert isinstance(got, np.ndarray)
        assert_same(got, c['warped'], c['name'])
        assert len(calls) == 2


# -- the roundings of the absolute map --------------------------------------------------------
@pytest.mark.parametrize('dim', [2, 3])
def test_double_rounding_is_visible(gpu, dim):
  """float32 nodes near 1000 with fractional strides and a box shift of -1000: both
  in-place adds round to float32, and most outputs show it."""
  rng = np.random.default_rng(20 + dim)
  shape, stride = (((40, 52), (10.3, 9.7)), ((9, 30, 36), (3.1, 6.3, 5.9)))[dim - 2]
  nodes = tuple(int(np.ceil(s / st)) + 1 for s, st in zip(shape, stride))
  img = rng.uniform(20.0, 300.0, shape).astype(np.float32)
  cmap32 = (1000.0 + rng.uniform(-2.0, 2.0, (dim,) + nodes)).astype(np.float32)
  image_start, zero = np.full(dim, 1000), np.zeros(dim, np.int64)
  size = np.array(shape[::-1])
  kw = dict(image_box=box(image_start, size), map_box=box(zero, np.array(nodes[::-1])),
            out_box=box(zero, size))
  ref_kw = dict(image_start=image_start, map_start=zero, out_start=zero)
  want32 = rel_ref.warp_scipy(img, cmap32, stride, **ref_kw)
  naive = rel_ref.warp_scipy(img, cmap32, stride, **ref_kw, absolute=functools.partial(
      rel_ref.absolute_map_per_element, naive=True))
  assert np.mean(want32 != naive) > 0.5
  assert np.mean(want32 != 0) > 0.5
  cmap64 = cmap32.astype(np.float64)
  want64 = rel_ref.warp_scipy(img, cmap64, stride, **ref_kw)
  assert np.mean(want64 != want32) > 0.5
  for cmap, want in ((cmap32, want32), (cmap64, want64)):
    with entries() as calls:
      got = warp.ndimage_warp(resident(img, gpu), resident(cmap, gpu), stride, shape[::-1],
                              (0,) * dim, device_output=True, **kw)
      assert_same(host_of(got, np.float32), want, cmap.dtype)
      assert_same(warp.ndimage_warp(img, cmap, stride, shape[::-1], (0,) * dim, **kw), want,
                  cmap.dtype)
      assert len(calls) == 2


# -- the smallest maps ----------------------------------------------------------------------
SMALL = [   # (image shape, nodes, stride)
    ((6, 7), (1, 3), (4.5, 2.5)),           # one node along y: the 2-D map of (2, 1, 3)
    ((6, 7), (3, 1), (2.0, 3.5)),
    ((6, 7), (1, 1), (3.0, 3.0)),
    ((4, 5, 6), (1, 3, 3), (2.5, 2.0, 2.5)),
    ((4, 5, 6), (2, 1, 3), (2.0, 2.5, 2.0)),
    ((4, 5, 6), (2, 3, 1), (1.5, 2.0, 3.0)),
    ((4, 5, 6), (1, 1, 1), (2.0, 2.0, 2.0)),
    ((12, 15), (3, 4), (3.0, 2.5)),         # the output is larger than the node grid
    ((5, 9, 11), (2, 3, 3), (2.0, 2.0, 3.5)),
]
SMALL_MODES = [None, ('nearest', 0.0), ('mirror', 0.0), ('constant', 7.25)]


@pytest.mark.parametrize('boxes', [False, True])
@pytest.mark.parametrize('case', range(len(SMALL)))
def test_smallest_maps(gpu, case, boxes):
  """Single nodes along one axis and along all, outputs beyond the node grid under the
  modes that fold or fill its taps, NaN nodes, and with boxes an out_box that starts
  before the map on one axis and after it on another."""
  shape, nodes, stride = SMALL[case]
  dim = len(shape)
  rng = np.random.default_rng(300 + 2 * case + boxes)
  for k, mode in enumerate(SMALL_MODES):
    dtype = (np.float32, np.uint8, np.uint16)[(case + k) % 3]
    map_dtype = (np.float32, np.float64)[(case + k) % 2]
    img = modes_ref.image(rng, shape, dtype)
    cmap = rng.uniform(-1.5, 1.5, (dim,) + nodes).astype(map_dtype)
    if (mode is None or mode[0] == 'constant') and cmap[0].size > 1:
      # a NaN node, under the mode where SciPy defines a NaN coordinate (cval)
      cmap[k % dim].flat[1] = np.nan
    kw, ref_kw = {}, {}
    if boxes:
      image_start = np.array([2, -1, 1][:dim])
      map_start = np.array([1, 0, -1][:dim])
      out_start = np.array([-2, 3, 1][:dim])
      size = np.array(shape[::-1])
      kw = dict(image_box=box(image_start, size), map_box=box(map_start, np.array(nodes[::-1])),
                out_box=box(out_start, size))
      ref_kw = dict(image_start=image_start, map_start=map_start, out_start=out_start)
    if mode is not None:
      kw['map_coordinates'] = sampler(*mode)
      ref_kw.update(mode=mode[0], cval=mode[1])
    want = rel_ref.warp_scipy(img, cmap, stride, **ref_kw)
    with entries() as calls:
      got = warp.ndimage_warp(resident(img, gpu), resident(cmap, gpu), stride, shape[::-1],
                              (0,) * dim, device_output=True, **kw)
      assert_same(host_of(got, dtype), want, (shape, nodes, mode, boxes))
      assert len(calls) == 1


# -- modes and orders on the relative accessor ------------------------------------------------
MODE_SHAPES = ((5, 7), (3, 4, 6))
assert MODE_SHAPES[0] in modes_ref.SHAPES_2D and MODE_SHAPES[1] in modes_ref.SHAPES_3D
DTYPES = (np.uint8, np.uint16, np.float32)
CVAL = 7.25


def _mode_case(gpu, shape, order, mode, dtype, seed):
  rng = np.random.default_rng(seed)
  img = modes_ref.image(rng, shape, dtype)
  cmap, out_shape = modes_ref.stride1_map(modes_ref.mode_coords(rng, shape))
  dim = len(shape)
  zero = np.zeros(dim, np.int64)
  b = box(zero, np.array(out_shape[::-1], np.int64))
  with entries() as calls:
    got = warp.ndimage_warp(resident(img, gpu), resident(cmap, gpu), (1,) * dim, tuple(b.size),
                            (0,) * dim, order=order, image_box=box(zero, zero), map_box=b,
                            out_box=b, map_coordinates=sampler(mode, CVAL))
    assert len(calls) == 1
  want = modes_ref.ndimage_warp_scipy(img, cmap, (1,) * dim, order, mode, CVAL, out_shape)
  assert_same(host_of(got, dtype), want, (shape, order, mode))


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('mode', modes_ref.MODES)
def test_modes_on_resident_inputs(gpu, mode, order):
  for k, shape in enumerate(MODE_SHAPES):
    dtype = DTYPES[(modes_ref.MODES.index(mode) + order + k) % 3]
    _mode_case(gpu, shape, order, mode, dtype, 100 * modes_ref.MODES.index(mode) + order)


@pytest.mark.parametrize('order', [2, 3, 4, 5])
@pytest.mark.parametrize('mode', modes_ref.SPLINE_MODES)
def test_spline_modes_on_resident_inputs(gpu, mode, order):
  with _abi.option(_spline.OPTION, 1):
    for k, shape in enumerate(MODE_SHAPES):
      _mode_case(gpu, shape, order, mode, DTYPES[(order + k) % 3],
                 1000 + 10 * modes_ref.MODES.index(mode) + order)


# -- nothing comes back to the host -----------------------------------------------------------
def test_resident_calls_copy_nothing_to_the_host(gpu, golden):
  g = golden('ndimage_warp')
  img, cmap, stride, work, ov, order, boxes, scale, want = ndimage_warp_case(g, 'u8_3d_boxes')
  kw = _golden_kw(boxes, scale)
  img_t, map_t = resident(img, gpu), resident(cmap, gpu)
  d = golden('warp_decorators')
  sof_t = resident(d['sof3_u8_o1_image'], gpu)
  cm_t = resident(d['cm_u8_nearest_scaled_image'], gpu)
  cm_map = _dev.DeviceArray(resident(d['cm_u8_nearest_scaled_map'], gpu))
  aff_t = resident(d['aff3_f32_o1_image'], gpu)
  with no_host_copies():
    out = [warp.ndimage_warp(img_t, map_t, stride, work, ov, order=order, device_output=True,
                             **kw)]
    with _abi.option(_spline.OPTION, 1):
      out.append(warp.ndimage_warp(img_t, map_t, stride, work, ov, order=3, **kw))
    out.append(warp.affine_transform(aff_t, d['aff3_f32_o1_matrix'], order=1))
    out.append(decorators_warp.warp_affine(sof_t, d['sof3_u8_o1_matrix'], order=1,
                                           implementation='sofima'))
    out.append(decorators_warp.warp_coord_map(
        cm_t, cm_map, mode='nearest', cval=float(d['cm_u8_nearest_scaled_cval']),
        scale_xyz=tuple(d['cm_u8_nearest_scaled_scale']),
        stride=tuple(float(v) for v in d['cm_u8_nearest_scaled_stride']), overlap=(0, 0, 0),
        order=int(d['cm_u8_nearest_scaled_order'])))
    with pytest.raises(AssertionError, match='device-to-host'):
      np.asarray(out[0])
  assert all(isinstance(o, _dev.DeviceArray) for o in out)
  assert_same(np.asarray(out[0]), want)
  assert_same(np.asarray(out[3]), d['sof3_u8_o1_out'])
  assert_same(np.asarray(out[4]), d['cm_u8_nearest_scaled_out'])


# -- the decorator warps and affine_transform -------------------------------------------------
def _decorator_names(prefix):
  import os
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'warp_decorators.npz')
  with np.load(path) as g:
    return [str(n) for n in g['names'] if str(n).startswith(prefix)]


@pytest.mark.parametrize('name', _decorator_names('sof3_') + _decorator_names('aff'))
def test_warp_affine_resident(gpu, golden, name):
  g = golden('warp_decorators')
  img = g[f'{name}_image']
  with _abi.option(_spline.OPTION, 1), entries():
    got = decorators_warp.warp_affine(resident(img, gpu), g[f'{name}_matrix'],
                                      order=int(g[f'{name}_order']),
                                      implementation=str(g[f'{name}_impl']))
    assert_same(host_of(got, img.dtype), g[f'{name}_out'], name)
    if name.startswith('aff'):
      got = warp.affine_transform(_dev.DeviceArray(resident(img, gpu)),
                                  np.linalg.inv(np.vstack([g[f'{name}_matrix'][:img.ndim],
                                                           np.eye(img.ndim + 1)[-1]])),
                                  order=int(g[f'{name}_order']))
      assert_same(host_of(got, img.dtype), g[f'{name}_out'], name)
      got = warp.affine_transform(resident(img, gpu), np.eye(img.ndim), device_output=False)
      assert isinstance(got, np.ndarray)
      assert_same(got, img, name)


@pytest.mark.parametrize('name', _decorator_names('cm_'))
def test_warp_coord_map_resident(gpu, golden, name):
  g = golden('warp_decorators')
  img, scale = g[f'{name}_image'], g[f'{name}_scale']
  kw = dict(stride=tuple(float(v) for v in g[f'{name}_stride']), overlap=(0, 0, 0),
            order=int(g[f'{name}_order']), scale_xyz=tuple(scale) if scale.size else None,
            mode=str(g[f'{name}_mode']), cval=float(g[f'{name}_cval']))
  with _abi.option(_spline.OPTION, 1), entries() as calls:
    got = decorators_warp.warp_coord_map(resident(img, gpu), resident(g[f'{name}_map'], gpu), **kw)
    assert_same(host_of(got, img.dtype), g[f'{name}_out'], name)
    got = decorators_warp.warp_coord_map(img, _dev.DeviceArray(resident(g[f'{name}_map'], gpu)),
                                         **kw)
    assert isinstance(got, np.ndarray)
    assert_same(got, g[f'{name}_out'], name)
    assert len(calls) == 2


def test_device_chain_from_make_affine_map(gpu):
  """make_affine_map -> ndimage_warp with the DeviceArray map equals the same call on
  the downloaded map."""
  rng = np.random.default_rng(5)
  img = modes_ref.image(rng, (6, 20, 24), np.uint16)
  matrix = np.hstack([np.eye(3) + rng.uniform(-0.05, 0.05, (3, 3)), [[0.4], [-0.8], [0.3]]])
  cmap = map_utils.make_affine_map(matrix, box(np.zeros(3, np.int64), np.array([12, 10, 3])),
                                   [2, 2, 2])
  assert isinstance(cmap, _dev.DeviceArray)
  host = np.asarray(cmap)
  want = rel_ref.warp_scipy(img, host, (2, 2, 2))
  assert np.mean(want != 0) > 0.5
  with entries() as calls:
    got = warp.ndimage_warp(resident(img, gpu), cmap, (2, 2, 2), img.shape[::-1], (0, 0, 0))
    assert len(calls) == 1
  assert_same(host_of(got, np.uint16), want)


# -- what is refused ------------------------------------------------------------------------
def test_what_is_refused(gpu):
  rng = np.random.default_rng(8)
  img = modes_ref.image(rng, (8, 9), np.uint8)
  cmap = rng.uniform(-1.5, 1.5, (2, 3, 3)).astype(np.float32)
  args = ((4, 4), (9, 8), (0, 0))
  want = rel_ref.warp_scipy(img, cmap, (4, 4))
  # resident maps are float32 or float64
  for bad in (torch.float16, torch.int32, torch.int64):
    with pytest.raises(TypeError, match='device maps'):
      warp.ndimage_warp(img, resident(cmap, gpu).to(bad), *args)
  # NumPy maps of other dtypes are prepared on the host, as they always were
  lib = _abi.load()
  saved = lib.sfm_ndimage_warp_rel
  try:
    def refuse(desc):
      raise AssertionError('the relative-map entry was called')
    lib.sfm_ndimage_warp_rel = refuse
    half = cmap.astype(np.float16)
    assert_same(warp.ndimage_warp(img, half, *args), rel_ref.warp_scipy(img, half, (4, 4)))
    whole = np.rint(cmap).astype(np.int64)
    assert_same(warp.ndimage_warp(resident(img, gpu), whole, *args, device_output=False),
                rel_ref.warp_scipy(img, whole, (4, 4)))
  finally:
    lib.sfm_ndimage_warp_rel = saved
  # a CPU tensor is host data
  got = warp.ndimage_warp(torch.from_numpy(img), torch.from_numpy(cmap), *args)
  assert isinstance(got, np.ndarray)
  assert_same(got, want)
  got = warp.affine_transform(torch.from_numpy(img), np.eye(2))
  assert isinstance(got, np.ndarray)
  assert_same(got, img)
  # label volumes, other image types and the orders behind the switch
  labels = img.astype(np.uint64)
  for image in (labels, torch.from_numpy(labels).to(gpu)):
    with pytest.raises(NotImplementedError, match='uint64'):
      warp.ndimage_warp(image, cmap, *args)
    with pytest.raises(NotImplementedError, match='uint64'):
      warp.affine_transform(image, np.eye(2))
  with pytest.raises(NotImplementedError):
    warp.ndimage_warp(resident(img, gpu).to(torch.int32), cmap, *args)
  for order in _spline.ORDERS:
    with pytest.raises(NotImplementedError, match=_spline.OPTION):
      warp.ndimage_warp(resident(img, gpu), resident(cmap, gpu), *args, order=order)
    with pytest.raises(NotImplementedError, match=_spline.OPTION):
      warp.affine_transform(resident(img, gpu), np.eye(2), order=order)
  with pytest.raises(ValueError, match='Dimension mismatch'):
    warp.ndimage_warp(resident(img, gpu)[0], resident(cmap, gpu), *args)
