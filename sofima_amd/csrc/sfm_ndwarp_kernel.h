// The kernels of the map_coordinates family and their launch templates.  A unit
// sfm_ndwarp_o*.hip includes this and instantiates the launches of one entry of
// SFM_NDWARP_UNITS (the macros at the end); sfm_ndwarp.h lists the other units of
// the family.  Double arithmetic in SciPy's operation order: every unit is built
// with -ffp-contract=off.
#ifndef SFM_NDWARP_KERNEL_H_
#define SFM_NDWARP_KERNEL_H_

#include "sfm_ndwarp.h"

#include <cmath>

namespace sfm {
namespace {

// The output voxel o (z, y, x) of this thread, i its linear index; false past the end.
__device__ __forceinline__ bool thread_voxel(const int* shape, long long& i, int* o) {
  const long long n = (long long)shape[0] * shape[1] * shape[2];
  i = blockIdx.x * (long long)kNdBlock + threadIdx.x;
  if (i >= n) return false;
  o[2] = static_cast<int>(i % shape[2]);
  o[1] = static_cast<int>((i / shape[2]) % shape[1]);
  o[0] = static_cast<int>(i / ((long long)shape[2] * shape[1]));
  return true;
}

// The shared statements below are macros, not device functions, on purpose: a helper
// between a kernel and the samplers is simplified on its own before it is inlined,
// and the kernels then come out with other instructions and registers (measured: 282
// of the 335 kernels).  Expanded inside the kernel they compile as if written there.

// The image step of every kernel of the family: `out` = the value at `coord` as the
// output type T, like NI's CASE_INTERP_OUT_*.  ORDER 0: `order` (0 or 1) on the image
// of type T; ORDER 2 .. 5: `image` holds the float64 B-spline coefficients of the
// image (sfm_spline_prefilter).  MODES: SciPy's boundary mode and fill value `b`, else
// mode "constant" with cval 0.  TAPS: orders 2 .. 5 under the modes beyond "constant",
// "mirror" and "wrap" (spline_sample<.., TAPS>); under "nearest" and "grid-constant"
// `image` holds the coefficients of the padded image and `ishape` its shape, and
// `coord`, which is unpadded, is shifted in place (its magnitude limit is that of the
// caller's coordinate).  `pitch`: see sfm_ndsample.h.
#define SFM_IMAGE_SAMPLE(out, DIM, T, ORDER, MODES, TAPS, image, ishape, order, coord, b, pitch) \
  do {                                                                                       \
    double v_;                                                                               \
    if constexpr (ORDER >= 2) {                                                              \
      if constexpr (TAPS) {                                                                  \
        if ((b).pad) {                                                                       \
          _Pragma("unroll") for (int d_ = 0; d_ < DIM; ++d_)                                 \
            (coord)[d_] = fabs((coord)[d_]) < 2147483648.0                                   \
                              ? (coord)[d_] + static_cast<double>((b).pad)                   \
                              : static_cast<double>(NAN);                                    \
        }                                                                                    \
      }                                                                                      \
      v_ = spline_sample<DIM, ORDER, MODES, TAPS>(static_cast<const double*>(image), ishape, \
                                                  coord, pitch, b);                          \
    } else {                                                                                 \
      const T* img_ = static_cast<const T*>(image);                                          \
      v_ = (order) == 0 ? nearest_sample<DIM, MODES>(img_, ishape, coord, pitch, b)          \
                        : linear_sample<DIM, MODES>(img_, ishape, coord, pitch, b);          \
    }                                                                                        \
    constexpr double vmax_ = sizeof(T) == 1 ? 255.0 : 65535.0;                               \
    out = nd_convert<T>(v_, vmax_);                                                          \
  } while (0)

// ---------------------------------------------------------------------------
// warp.ndimage_warp (warp.py:189-335): scipy.ndimage.map_coordinates twice --
// order 1 on the float64 source map at the node-space position of the output
// voxel, then the image step at the resulting coordinates.  The source map is
// either the float64 absolute map a caller prepared, or the relative map in its
// own type, made absolute on every read (sfm_ndimage_warp_rel): one body, three
// map accessors.
//
// MODES: SciPy's boundary mode and fill value `b` on BOTH steps, as the reference
// hands one map_coordinates callable to both (warp.py:308-314): outside the node
// grid the dense coordinate is cval (in source voxels) or the folded node value,
// and the image sample follows the same rule; an integer image takes cval through
// nd_convert like a sampled value.  The map step is order 1 and never padded.
//
// The body of both kernels, for their argument `a` and template parameters:
// node-space position (warp.py:300-301), then the dense coordinates z, y, x =
// channels DIM - 1 ... 0 of the map (warp.py:304-307), then the image step.
// ---------------------------------------------------------------------------
#define SFM_NDWARP_BODY(MODES, TAPS, b)                                                      \
  do {                                                                                       \
    long long i;                                                                             \
    int o[3];                                                                                \
    if (!thread_voxel(a.oshape, i, o)) return;                                               \
    double pos[DIM];                                                                         \
    _Pragma("unroll") for (int d = 0; d < DIM; ++d) {                                        \
      const int ax = 3 - DIM + d;                                                            \
      pos[d] = (static_cast<double>(o[ax]) - a.offset[ax]) / a.stride[ax];                   \
    }                                                                                        \
    const long long nodes = (long long)a.mshape[0] * a.mshape[1] * a.mshape[2];              \
    double dense[DIM];                                                                       \
    _Pragma("unroll") for (int d = 0; d < DIM; ++d)                                          \
      dense[d] = linear_sample<DIM, MODES>(a.map.template channel<DIM>(d, nodes, a.stride),  \
                                           a.mshape, pos, nullptr, b);                       \
    SFM_IMAGE_SAMPLE(static_cast<T*>(a.out)[i], DIM, T, ORDER, MODES, TAPS, a.image,         \
                     a.ishape, a.order, dense, b, nullptr);                                  \
  } while (0)

// ORDER 0: a.order (0 or 1) on the image; ORDER 2 .. 5: on its coefficients.
template <int DIM, typename T, int ORDER, typename MAP>
__global__ void __launch_bounds__(kNdBlock) ndimage_warp_kernel(NdWarpArgs<MAP> a) {
  SFM_NDWARP_BODY(false, false, Boundary());
}

// (the TAPS kernels are kernels of their own, which the three mirroring modes never run)
template <int DIM, typename T, int ORDER, typename MAP, bool TAPS = false>
__global__ void __launch_bounds__(kNdBlock)
ndimage_warp_mode_kernel(NdWarpArgs<MAP> a, Boundary b) {
  SFM_NDWARP_BODY(true, TAPS, b);
}

// ---------------------------------------------------------------------------
// scipy.ndimage.affine_transform with a [dim, dim] matrix: the source coordinate
// of an output voxel is a matrix product and an offset, formed in double from
// kernel arguments (scalar registers) -- products added in axis order onto 0,
// the offset last, which is SciPy's rounding -- and handed to the image step (the
// pad shift comes after the offset, as SciPy adds it).  No coordinate map exists.
// One thread per output voxel, a wave per 64 contiguous voxels, as in ndimage_warp.
// ---------------------------------------------------------------------------
template <int DIM, typename T, int ORDER = 0, bool TAPS = false>
__global__ void __launch_bounds__(kNdBlock) affine_warp_kernel(AffineArgs a) {
  long long i;
  int o[3];
  if (!thread_voxel(a.shape, i, o)) return;
  double c[DIM];
#pragma unroll
  for (int h = 0; h < DIM; ++h) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k)
      acc = acc + static_cast<double>(o[3 - DIM + k]) * a.m[3 - DIM + h][3 - DIM + k];
    c[h] = acc + a.off[3 - DIM + h];
  }
  SFM_IMAGE_SAMPLE(static_cast<T*>(a.out)[i], DIM, T, ORDER, true, TAPS, a.image, a.ishape,
                   a.order, c, a.b, nullptr);
}

// ---------------------------------------------------------------------------
// processor/warp.py: StitchAndRender3dTiles.process (:292-343): per tile two
// ndimage_warp calls (image, blend weights) and a float32 weighted sum, then
// the normalisation and the cast -- here one kernel per output box.  A
// workgroup takes a brick of kBrickY lines of kBrickX voxels in one z plane
// (one wave per line, so stores are whole lines), walks the tile table in
// ascending order, drops a tile whose sub_box misses the brick (a test on
// block indices and table entries only: a scalar branch) and only then tests
// its own voxel.  The dense coordinates are computed once per (voxel, tile)
// and serve both samples; img and norm live in registers.
// ---------------------------------------------------------------------------

// NumPy's astype from float32: integers truncate toward zero
template <typename O>
__device__ __forceinline__ O render_cast(float v) {
  return static_cast<O>(static_cast<int>(v));
}
template <>
__device__ __forceinline__ float render_cast<float>(float v) {
  return v;
}

// ORDER 0: a.order (0 or 1), the data_box region of the tile read in place;
// ORDER 2 .. 5: the region's B-spline coefficients, a.coeffs + the sizes of the
// regions of the table entries before it.
template <typename T, typename O, int ORDER = 0>
__global__ void __launch_bounds__(kBrickX* kBrickY) render_tiles_kernel(RenderArgs a) {
  const int bx0 = blockIdx.x * kBrickX, by0 = blockIdx.y * kBrickY;
  const int bx1 = min(bx0 + kBrickX, a.oshape[2]), by1 = min(by0 + kBrickY, a.oshape[1]);
  const int z = blockIdx.z;
  const int x = bx0 + threadIdx.x, y = by0 + threadIdx.y;
  const bool live = x < bx1 && y < by1;
  float img = 0.f, norm = 0.f;
  long long next_region = 0;
  for (int t = 0; t < a.n_tiles; ++t) {
    const SfmRenderTile& r = a.tiles[t];
    const long long region = next_region;
    if constexpr (ORDER >= 2)
      next_region += (long long)r.data_size[0] * r.data_size[1] * r.data_size[2];
    // the brick against sub_box
    const int sz = r.sub_start[0], sy = r.sub_start[1], sx = r.sub_start[2];
    const int ez = sz + r.sub_size[0], ey = sy + r.sub_size[1], ex = sx + r.sub_size[2];
    if (z < sz || z >= ez || by1 <= sy || by0 >= ey || bx1 <= sx || bx0 >= ex) continue;
    // the voxel against sub_box
    if (!live || y < sy || y >= ey || x < sx || x >= ex) continue;
    // node-space position (warp.py:305), o relative to local_warp_box
    const int o[3] = {z - sz, y - sy, x - sx};
    double pos[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) pos[d] = (static_cast<double>(o[d]) - r.offset[d]) / a.stride[d];
    // dense coordinates z, y, x = channels 2, 1, 0 of the absolute map (warp.py:308-311)
    const long long nodes = (long long)r.map_shape[0] * r.map_shape[1] * r.map_shape[2];
    double dense[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const ShiftedMap m = {r.abs_map + (long long)(2 - d) * nodes, r.shift[2 - d]};
      dense[d] = linear_sample<3>(m, r.map_shape, pos);
    }
    // the image region data_box, read in place; the coefficients are dense
    const long long ipitch[3] = {(long long)r.tile_shape[1] * r.tile_shape[2], r.tile_shape[2], 1};
    const long long wpitch[3] = {0, r.tile_shape[2], 1};
    const long long worg = (long long)r.data_start[1] * r.tile_shape[2] + r.data_start[2];
    const void* im;
    if constexpr (ORDER >= 2)
      im = a.coeffs + region;
    else
      im = static_cast<const T*>(r.image) + r.data_start[0] * ipitch[0] + worg;
    T iv;
    SFM_IMAGE_SAMPLE(iv, 3, T, ORDER, false, false, im, r.data_size, a.order, dense, Boundary(),
                     (ORDER >= 2 ? nullptr : ipitch));
    // the weights: the 2-D array repeated over data_size[0] planes, order 1
    const float w = nd_convert<float>(
        linear_sample<3>(r.weights + worg, r.data_size, dense, wpitch), 0.0);
    img = img + static_cast<float>(iv) * w;
    norm = norm + w;
  }
  if (!live) return;
  if (norm > 0.f) img = img / norm;
  static_cast<O*>(a.out)[((long long)z * a.oshape[1] + y) * a.oshape[2] + x] = render_cast<O>(img);
}

// The kernel choice that every launch shares: f(T()) with the element type of dtype.
template <typename F>
void for_dtype(int dtype, F&& f) {
  switch (dtype) {
    case SFM_DTYPE_U8: f(static_cast<unsigned char>(0)); break;
    case SFM_DTYPE_U16: f(static_cast<unsigned short>(0)); break;
    default: f(0.f); break;
  }
}

}  // namespace

template <int ORDER, int DIM, typename MAP>
int launch_ndwarp(const NdWarpArgs<MAP>& a, const Boundary* bnd, bool taps, const NdLaunch& l) {
  for_dtype(l.dtype, [&](auto t) {
    using T = decltype(t);
    if (taps)
      hipLaunchKernelGGL((ndimage_warp_mode_kernel<DIM, T, ORDER, MAP, (ORDER >= 2)>), l.grid,
                         l.block, 0, l.stream, a, *bnd);
    else if (bnd)
      hipLaunchKernelGGL((ndimage_warp_mode_kernel<DIM, T, ORDER, MAP>), l.grid, l.block, 0,
                         l.stream, a, *bnd);
    else
      hipLaunchKernelGGL((ndimage_warp_kernel<DIM, T, ORDER, MAP>), l.grid, l.block, 0, l.stream,
                         a);
  });
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

template <int ORDER, int DIM>
int launch_affine(const AffineArgs& a, bool taps, const NdLaunch& l) {
  for_dtype(l.dtype, [&](auto t) {
    using T = decltype(t);
    if (taps)
      hipLaunchKernelGGL((affine_warp_kernel<DIM, T, ORDER, (ORDER >= 2)>), l.grid, l.block, 0,
                         l.stream, a);
    else
      hipLaunchKernelGGL((affine_warp_kernel<DIM, T, ORDER>), l.grid, l.block, 0, l.stream, a);
  });
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

template <int ORDER>
int launch_render(const RenderArgs& a, bool out_f32, const NdLaunch& l) {
  for_dtype(l.dtype, [&](auto t) {
    using T = decltype(t);
    if (out_f32)
      hipLaunchKernelGGL((render_tiles_kernel<T, float, ORDER>), l.grid, l.block, 0, l.stream, a);
    else
      hipLaunchKernelGGL((render_tiles_kernel<T, T, ORDER>), l.grid, l.block, 0, l.stream, a);
  });
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace sfm

// What a unit instantiates.  SFM_NDWARP_MAP_UNIT: the nd-warp kernels of one map
// accessor; SFM_NDWARP_IMAGE_UNIT: the kernels without a map of their own (affine,
// and in 3-D the render); SFM_NDWARP_UNIT: the whole of an entry of SFM_NDWARP_UNITS.
#define SFM_NDWARP_MAP_UNIT(ORDER, DIM, MAP)                                                  \
  template int sfm::launch_ndwarp<ORDER, DIM, sfm::MAP>(const sfm::NdWarpArgs<sfm::MAP>&,     \
                                                        const sfm::Boundary*, bool,           \
                                                        const sfm::NdLaunch&);
#define SFM_NDWARP_RENDER_2(ORDER)
#define SFM_NDWARP_RENDER_3(ORDER) \
  template int sfm::launch_render<ORDER>(const sfm::RenderArgs&, bool, const sfm::NdLaunch&);
#define SFM_NDWARP_IMAGE_UNIT(ORDER, DIM)                                                     \
  template int sfm::launch_affine<ORDER, DIM>(const sfm::AffineArgs&, bool,                   \
                                              const sfm::NdLaunch&);                          \
  SFM_NDWARP_RENDER_##DIM(ORDER)
#define SFM_NDWARP_UNIT(ORDER, DIM)                     \
  SFM_NDWARP_MAP_UNIT(ORDER, DIM, AbsoluteMap)          \
  SFM_NDWARP_MAP_UNIT(ORDER, DIM, RelativeMapArgs<float>)  \
  SFM_NDWARP_MAP_UNIT(ORDER, DIM, RelativeMapArgs<double>) \
  SFM_NDWARP_IMAGE_UNIT(ORDER, DIM)

#endif  // SFM_NDWARP_KERNEL_H_
