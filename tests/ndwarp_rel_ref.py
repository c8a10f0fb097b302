"""The absolute source map of `warp.ndimage_warp`, two ways (no GPU, no package code).

`absolute_map_statements` is the reference's array arithmetic (warp.py:249-262), as
`sofima_amd.warp._absolute_map` restates it: map_utils.to_absolute adds node x stride
in place, the box shift is a second in-place add, the out_scale product is float64.

`absolute_map_per_element` is the statement the kernel is written from
(sfm_ndsample.h, RelativeMap): per element, for channel c of axis
ax = ndim - 1 - c, node index n and map dtype M,

  v = (double) rel[c][node]
  v = (double)(M)(v + (double) n[ax] * stride[ax])
  v = (double)(M)(v + shift[c])              only with a map_box
  v = v * out_scale[c]

with shift[c] = map_box.start[c] * stride[::-1][c] - image_box.start[c] / out_scale[c]
formed in float64 by the host.  tests/test_ndwarp_rel_ref.py holds the two equal bit
for bit; the GPU tests build their references from the first.

`warp_scipy` is the whole function on one work box: the statements, then
scipy.ndimage.map_coordinates twice with one mode and fill value (warp.py:296-314).
"""
import numpy as np


def shift_of(stride, image_start, map_start, out_scale, dim):
  """The float64 box shift per channel, the reference's expression."""
  return np.asarray(np.asarray(map_start)[:dim] * np.asarray(stride)[::-1] -
                    np.asarray(image_start)[:dim] / np.asarray(out_scale)[:dim], np.float64)


def absolute_map_statements(coord_map, stride, image_start=None, map_start=None,
                            out_scale=(1.0, 1.0, 1.0)):
  """float64 [ndim, ...]: the reference's statements on whole arrays."""
  shape = coord_map.shape[1:]
  dim = len(shape)
  src = np.array(coord_map, copy=True)
  idx = np.mgrid[tuple(slice(0, s) for s in shape)]
  off_zyx = [h * st for h, st in zip(idx, stride)]
  for i in range(dim):
    src[i, ...] += off_zyx[-(i + 1)]
  if map_start is not None:
    src += (np.asarray(map_start)[:dim] * np.asarray(stride)[::-1] -
            np.asarray(image_start)[:dim] / np.asarray(out_scale)[:dim]).reshape(
                (dim,) + (1,) * dim)
  reshaper = (slice(None),) + (np.newaxis,) * dim
  return np.ascontiguousarray(src.copy() * np.array(out_scale[:dim])[reshaper], dtype=np.float64)


def absolute_map_per_element(coord_map, stride, image_start=None, map_start=None,
                             out_scale=(1.0, 1.0, 1.0), naive=False):
  """float64 [ndim, ...]: the kernel's formula, one element at a time in Python
  scalars of exactly the stated types.  naive: everything in double, rounded to
  nothing in between -- what a kernel that skips the stores as M computes."""
  m = coord_map.dtype.type
  assert m in (np.float32, np.float64)
  shape = coord_map.shape[1:]
  dim = len(shape)
  shift = None
  if map_start is not None:
    shift = shift_of(stride, image_start, map_start, out_scale, dim)
  out = np.empty(coord_map.shape, np.float64)
  for c in range(dim):
    ax = dim - 1 - c
    st = np.float64(float(stride[ax]))
    sc = np.float64(float(out_scale[c]))
    for node in np.ndindex(*shape):
      v = np.float64(coord_map[(c,) + node])
      off = np.float64(node[ax]) * st
      v = v + off if naive else np.float64(m(v + off))
      if shift is not None:
        v = v + shift[c] if naive else np.float64(m(v + shift[c]))
      out[(c,) + node] = v * sc
  return out


def warp_scipy(image, coord_map, stride, order=1, mode='constant', cval=0.0, image_start=None,
               map_start=None, out_start=None, out_shape=None, out_scale=(1.0, 1.0, 1.0),
               absolute=absolute_map_statements):
  """warp.ndimage_warp on one work box with SciPy on both steps.  Boxes are given
  by their starts in xyz; out_shape is z, y, x (the image's by default)."""
  from scipy import ndimage
  dim = coord_map.ndim - 1
  src = absolute(coord_map, stride, image_start, map_start, out_scale)
  out_shape = image.shape if out_shape is None else tuple(out_shape)
  out_start = np.zeros(3, np.int64) if out_start is None else np.asarray(out_start)
  if map_start is not None:
    offset = (np.asarray(map_start) * np.asarray(stride)[::-1] - out_start[:len(map_start)])[::-1]
  else:
    offset = (0,) * dim
  pos = np.mgrid[tuple(slice(0, s) for s in out_shape)]
  pos = [(c - o) / s for c, o, s in zip(pos, offset[-dim:], stride)]
  with np.errstate(all='ignore'):
    dense = [ndimage.map_coordinates(ev, pos, order=1, mode=mode, cval=cval) for ev in src[::-1]]
    return ndimage.map_coordinates(image, dense, order=order, mode=mode, cval=cval)
