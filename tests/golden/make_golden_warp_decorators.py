"""Generates tests/golden/warp_decorators.npz from the UNMODIFIED reference
`decorators/warp.py`: its `_warp_affine` (implementation 'scipy' in 2-D and 3-D,
'sofima' in 3-D) and `_warp_coord_map` (modes 'constant' with cval 3, 'nearest',
'mirror'; with and without scale_xyz) run as they are, on NumPy / SciPy, with the
reference's own `map_utils.make_affine_map` and `warp.ndimage_warp`.

Build-container only.  `_refshim` makes `import sofima` and the connectomics box
types resolve; the module imports four more packages that are not in this
container and that the two functions never touch on these paths.  Their
stand-ins are declared HERE:

  tensorstore      an empty module (annotations of the decorator classes only)
  gin              gin.register returns the class it decorates
  connectomics.volume.decorators   Decorator: an empty base class;
                   adjust_schema_for_virtual_chunked: never called
  connectomics.common.opencv_utils   an empty module ('opencv' is not run)

Stored -- data only, per case `name` of `names`:
  {name}_kind     'affine' | 'coord_map'
  {name}_image    img_xyz; {name}_out: the function's result
  affine:     {name}_matrix, {name}_order, {name}_impl
  coord_map:  {name}_map ([3, z, y, x] relative), {name}_mode, {name}_cval,
              {name}_scale (xyz, or empty for None), {name}_stride (zyx),
              {name}_order
Volumes are at most [6, 20, 24].  The generator asserts its own coverage: more
than 20 % of every output is non-zero, and more than 20 % of every coord_map
output differs from the same call under the default mode.
Run:
  python tests/golden/make_golden_warp_decorators.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '_refshim'))
import refshim  # noqa: E402

refshim.install()

# -- stand-ins (see the module docstring) ----------------------------------------
sys.modules['tensorstore'] = types.ModuleType('tensorstore')
for _name in ('TensorStore', 'IndexDomain', 'VirtualChunkedReadParameters', 'Schema'):
  setattr(sys.modules['tensorstore'], _name, type(_name, (), {}))
sys.modules['gin'] = types.ModuleType('gin')
sys.modules['gin'].register = lambda cls: cls
_dec = types.ModuleType('connectomics.volume.decorators')
_dec.Decorator = type('Decorator', (), {})
_dec.adjust_schema_for_virtual_chunked = None
sys.modules['connectomics.volume.decorators'] = _dec
sys.modules['connectomics.volume'].decorators = _dec
_cv = types.ModuleType('connectomics.common.opencv_utils')
sys.modules['connectomics.common.opencv_utils'] = _cv
sys.modules['connectomics.common'].opencv_utils = _cv

from sofima.decorators import warp as ref_warp  # noqa: E402


def image(rng, shape_xyz, dtype):
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    return rng.uniform(20.0, 300.0, shape_xyz).astype(dtype)
  return rng.integers(20, np.iinfo(dtype).max + 1, shape_xyz).astype(dtype)


def forward_matrix(dim, angle, scale, shift):
  """Rotation in the xy plane about the image centre-ish point, anisotropic scale,
  a little shear, a shift: [dim, dim + 1]."""
  m = np.eye(dim)
  m[:2, :2] = [[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]
  m = m @ np.diag(scale[:dim])
  m[0, 1] += 0.05
  if dim == 3:
    m[2, 0] += 0.02
  return np.concatenate([m, np.asarray(shift, np.float64)[:dim, None]], axis=1)


def main():
  rng = np.random.default_rng(20240607)
  out = {}
  names = []

  def affine(name, shape_xyz, dtype, order, impl, homogeneous=False):
    dim = len(shape_xyz)
    img = image(rng, shape_xyz, dtype)
    m = forward_matrix(dim, 0.12, (1.05, 0.95, 1.1), (1.5, -0.75, 0.4))
    if homogeneous:
      m = np.vstack([m, [[0.0] * dim + [1.0]]])
    res = ref_warp._warp_affine(img, m, order=order, implementation=impl)
    assert res.shape == img.shape and res.dtype == img.dtype
    assert np.mean(res != 0) > 0.2, (name, np.mean(res != 0))
    names.append(name)
    out.update({f'{name}_kind': 'affine', f'{name}_image': img, f'{name}_matrix': m,
                f'{name}_order': order, f'{name}_impl': impl, f'{name}_out': res})

  affine('aff2_u8_o1', (24, 20), np.uint8, 1, 'scipy')
  affine('aff2_f32_o3', (24, 20), np.float32, 3, 'scipy', homogeneous=True)
  affine('aff2_u16_o0', (7, 5), np.uint16, 0, 'scipy')
  affine('aff3_u8_o1', (24, 20, 6), np.uint8, 1, 'scipy')
  affine('aff3_f32_o1', (12, 9, 4), np.float32, 1, 'scipy', homogeneous=True)
  affine('aff3_u16_o3', (12, 9, 4), np.uint16, 3, 'scipy')
  affine('sof3_u8_o1', (24, 20, 6), np.uint8, 1, 'sofima')
  affine('sof3_u16_o0', (24, 20, 6), np.uint16, 0, 'sofima', homogeneous=True)
  affine('sof3_f32_o1', (12, 9, 4), np.float32, 1, 'sofima')

  def coord_map(name, shape_xyz, dtype, stride_zyx, nodes_zyx, mode, cval, scale, order):
    img = image(rng, shape_xyz, dtype)
    cmap = rng.uniform(-1.5, 1.5, (3,) + nodes_zyx)
    kw = dict(stride=stride_zyx, overlap=(0, 0, 0), order=order)
    res = ref_warp._warp_coord_map(img, cmap, mode=mode, cval=cval, scale_xyz=scale, **kw)
    default = ref_warp._warp_coord_map(img, cmap, scale_xyz=scale, **kw)
    assert res.shape == img.shape and res.dtype == img.dtype
    assert np.mean(res != 0) > 0.2, (name, np.mean(res != 0))
    assert np.mean(res != default) > 0.2, (name, np.mean(res != default))
    names.append(name)
    out.update({f'{name}_kind': 'coord_map', f'{name}_image': img, f'{name}_map': cmap,
                f'{name}_mode': mode, f'{name}_cval': float(cval),
                f'{name}_scale': np.asarray([] if scale is None else scale, np.float64),
                f'{name}_stride': np.asarray(stride_zyx, np.float64),
                f'{name}_order': order, f'{name}_out': res})

  # the node grids cover (nodes - 1) * stride voxels: less than the volume, so the map
  # step itself leaves the grid on most of the output
  big = ((24, 20, 6), (2.0, 4.0, 4.0), (2, 3, 4))
  small = ((13, 9, 4), (1.0, 3.0, 2.5), (3, 2, 4))
  for dtype, tag, (shape, stride, nodes) in ((np.uint8, 'u8', big), (np.float32, 'f32', small)):
    coord_map(f'cm_{tag}_constant3', shape, dtype, stride, nodes, 'constant', 3, None, 1)
    coord_map(f'cm_{tag}_nearest', shape, dtype, stride, nodes, 'nearest', 0.0, None, 1)
    coord_map(f'cm_{tag}_mirror', shape, dtype, stride, nodes, 'mirror', 0.0, None, 1)
    coord_map(f'cm_{tag}_nearest_scaled', shape, dtype, stride, nodes, 'nearest', 0.0,
              (1.5, -0.5, 0.75), 1)
    coord_map(f'cm_{tag}_mirror_scaled_o0', (13, 9, 4), dtype, small[1], small[2], 'mirror', 0.0,
              (0.5, 2.0, 1.0), 0)
  coord_map('cm_u16_constant3_scaled', (13, 9, 4), np.uint16, (1.0, 3.0, 2.5), (3, 2, 4),
            'constant', 3, (2.0, 1.0, -1.0), 1)

  out['names'] = np.array(names)
  path = os.path.join(HERE, 'warp_decorators.npz')
  np.savez_compressed(path, **out)
  print(path, os.path.getsize(path), 'bytes,', len(names), 'cases')


if __name__ == '__main__':
  main()
