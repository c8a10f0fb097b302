// Image warping by an inverse coordinate map on the device (SURVEY.md 8f, rank 4:
// the rendering step that follows mesh relaxation).
//
//   sfm_warp_section  <->  warp.warp_subvolume._warp_section (warp.py:145-167)
//
// The reference does, per section: (1) scipy RegularGridInterpolator (linear,
// extrapolating) of the node coordinates to every output pixel, in float64,
// cast to float32; (2) cv2.convertMaps to the fixed-point CV_16SC2 format
// (1/32 pixel); (3) cv2.remap with constant (0) border.  This kernel fuses the
// three steps: one thread per output pixel, the dense coordinate maps never
// exist in memory.  Interpolation weights come from caller-built tables (the
// host side builds them like OpenCV's initInterTab2D: 32 x 32 sub-pixel phases,
// ksize x ksize taps; 15-bit fixed point for 8-bit images).
#include "sfm_common.h"
#include "sfm_ndsample.h"

#include <cmath>

namespace {

constexpr int kBlock = 256;
constexpr int kTabBits = 5, kTabSize = 1 << kTabBits;

struct WarpArgs {
  const void* image;
  const void* map;      // [2, my, mx] absolute source coordinates (x, y), float or double
  int map_f64;
  void* out;
  const void* tab;      // [32 * 32, ks * ks] short (u8 images) or float
  int dtype, nearest, ks;
  int iy, ix, my, mx, oy, ox;
  double org_y, org_x, stride;
};

// saturate_cast<short>
__device__ __forceinline__ int sat_short(long long v) {
  return v < -32768 ? -32768 : (v > 32767 ? 32767 : static_cast<int>(v));
}

// cvRound: round half to even; NaN / out of range -> INT_MIN like cvtss2si
__device__ __forceinline__ long long cv_round(double v) {
  if (!(v > -2147483648.0 && v < 2147483647.0)) return -2147483648LL;
  return static_cast<long long>(rint(v));
}

// Linear interpolation (with extrapolation) of one map component at grid
// position (gy, gx) in node units (RegularGridInterpolator, method "linear",
// fill_value None).
template <typename M>
__device__ __forceinline__ double map_at(const M* m, int my, int mx, double gy,
                                         double gx) {
  int i = static_cast<int>(floor(gy)), j = static_cast<int>(floor(gx));
  i = i < 0 ? 0 : (i > my - 2 ? my - 2 : i);
  j = j < 0 ? 0 : (j > mx - 2 ? mx - 2 : j);
  const double t = gy - i, u = gx - j;
  const double v00 = m[i * mx + j], v01 = m[i * mx + j + 1];
  const double v10 = m[(i + 1) * mx + j], v11 = m[(i + 1) * mx + j + 1];
  return (1.0 - t) * (1.0 - u) * v00 + (1.0 - t) * u * v01 + t * (1.0 - u) * v10 +
         t * u * v11;
}

template <typename T>
__device__ __forceinline__ T pixel(const T* img, int iy, int ix, int y, int x) {
  return (y >= 0 && y < iy && x >= 0 && x < ix) ? img[(long long)y * ix + x] : T(0);
}

template <typename T, bool FIXED>
__global__ void __launch_bounds__(kBlock) warp_kernel(WarpArgs a) {
  const long long n = (long long)a.oy * a.ox;
  const long long idx = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (idx >= n) return;
  const int py = static_cast<int>(idx / a.ox), px = static_cast<int>(idx % a.ox);
  const double gy = (py - a.org_y) / a.stride, gx = (px - a.org_x) / a.stride;
  const long long plane = (long long)a.my * a.mx;
  float sx, sy;   // dense coordinates: interpolated in the map's dtype, cast to float32
  if (a.map_f64) {
    const double* m = static_cast<const double*>(a.map);
    sx = static_cast<float>(map_at(m, a.my, a.mx, gy, gx));
    sy = static_cast<float>(map_at(m + plane, a.my, a.mx, gy, gx));
  } else {
    const float* m = static_cast<const float*>(a.map);
    sx = static_cast<float>(map_at(m, a.my, a.mx, gy, gx));
    sy = static_cast<float>(map_at(m + plane, a.my, a.mx, gy, gx));
  }
  const T* img = static_cast<const T*>(a.image);
  T* out = static_cast<T*>(a.out);
  if (a.nearest) {
    const int x = sat_short(cv_round(sx)), y = sat_short(cv_round(sy));
    out[idx] = pixel(img, a.iy, a.ix, y, x);
    return;
  }
  // fixed-point map: integer part and 5-bit fraction
  const long long fx = cv_round(static_cast<double>(sx) * kTabSize);
  const long long fy = cv_round(static_cast<double>(sy) * kTabSize);
  const int x0 = sat_short(fx >> kTabBits), y0 = sat_short(fy >> kTabBits);
  const int phase = static_cast<int>(fy & (kTabSize - 1)) * kTabSize +
                    static_cast<int>(fx & (kTabSize - 1));
  const int ks = a.ks, ofs = ks / 2 - 1;
  if (FIXED) {
    const short* w = static_cast<const short*>(a.tab) + (long long)phase * ks * ks;
    int acc = 0;
    for (int k1 = 0; k1 < ks; ++k1)
      for (int k2 = 0; k2 < ks; ++k2)
        acc += static_cast<int>(w[k1 * ks + k2]) *
               static_cast<int>(pixel(img, a.iy, a.ix, y0 + k1 - ofs, x0 + k2 - ofs));
    int v = (acc + (1 << 14)) >> 15;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    out[idx] = static_cast<T>(v);
  } else {
    const float* w = static_cast<const float*>(a.tab) + (long long)phase * ks * ks;
    float acc = 0.f;
    for (int k1 = 0; k1 < ks; ++k1)
      for (int k2 = 0; k2 < ks; ++k2)
        acc += w[k1 * ks + k2] *
               static_cast<float>(pixel(img, a.iy, a.ix, y0 + k1 - ofs, x0 + k2 - ofs));
    if (sizeof(T) == 2) {  // uint16: saturate_cast<ushort>(cvRound)
      const long long r = cv_round(acc);
      out[idx] = static_cast<T>(r < 0 ? 0 : (r > 65535 ? 65535 : r));
    } else {
      out[idx] = static_cast<T>(acc);
    }
  }
}

}  // namespace

extern "C" int sfm_warp_section(const SfmWarpDesc* d) {
  if (!d || !d->image || !d->coord_map || !d->out)
    return sfm::fail(SFM_ERR_INVALID, "warp: NULL argument");
  if (d->map_shape[0] < 2 || d->map_shape[1] < 2)
    return sfm::fail(SFM_ERR_INVALID, "warp: the coordinate map needs 2 x 2 nodes");
  for (int i = 0; i < 2; ++i)
    if (d->image_shape[i] < 1 || d->out_shape[i] < 1)
      return sfm::fail(SFM_ERR_INVALID, "warp: bad shape");
  const bool nearest = d->interpolation == SFM_WARP_NEAREST;
  if (!nearest && (!d->weights || (d->ksize != 2 && d->ksize != 4 && d->ksize != 8)))
    return sfm::fail(SFM_ERR_INVALID, "warp: weight table / ksize");
  if (!(d->stride > 0.f)) return sfm::fail(SFM_ERR_INVALID, "warp: stride");
  WarpArgs a;
  a.image = d->image;
  a.map = d->coord_map;
  a.map_f64 = d->coord_map_f64 ? 1 : 0;
  a.out = d->out;
  a.tab = d->weights;
  a.dtype = d->dtype;
  a.nearest = nearest ? 1 : 0;
  a.ks = d->ksize;
  a.iy = d->image_shape[0];
  a.ix = d->image_shape[1];
  a.my = d->map_shape[0];
  a.mx = d->map_shape[1];
  a.oy = d->out_shape[0];
  a.ox = d->out_shape[1];
  a.org_y = d->map_origin[0];
  a.org_x = d->map_origin[1];
  a.stride = d->stride;
  const long long n = (long long)a.oy * a.ox;
  const long long grid = (n + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "warp: too large");
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const dim3 g(static_cast<unsigned>(grid)), b(kBlock);
  switch (d->dtype) {
    case SFM_DTYPE_U8:
      hipLaunchKernelGGL((warp_kernel<unsigned char, true>), g, b, 0, st, a);
      break;
    case SFM_DTYPE_U16:
      hipLaunchKernelGGL((warp_kernel<unsigned short, false>), g, b, 0, st, a);
      break;
    case SFM_DTYPE_F32:
      hipLaunchKernelGGL((warp_kernel<float, false>), g, b, 0, st, a);
      break;
    case SFM_DTYPE_I32:
      if (!nearest) return sfm::fail(SFM_ERR_INVALID, "warp: int32 labels are nearest only");
      hipLaunchKernelGGL((warp_kernel<int, false>), g, b, 0, st, a);
      break;
    default:
      return sfm::fail(SFM_ERR_INVALID, "warp: dtype %d", d->dtype);
  }
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// warp.ndimage_warp (warp.py:189-335): scipy.ndimage.map_coordinates twice --
// order 1 on the float64 source map at the node-space position of the output
// voxel, then order 0 / 1 on the image at the resulting coordinates, or order
// 2 .. 5 on its B-spline coefficients (sfm_spline_prefilter).  Double arithmetic
// in SciPy's order (this file is built with -ffp-contract=off).  The source map
// is either the float64 absolute map a caller prepared, or the relative map in
// its own type, made absolute on every read (sfm_ndimage_warp_rel): one kernel
// template, two map accessors.
// ---------------------------------------------------------------------------
namespace {

// The map of a launch, as the kernels read it: channel<DIM>(d, nodes, stride) is
// the accessor of the channel that gives the dense coordinate of axis d (channel
// DIM - 1 - d: channels are x, y[, z]) for sfm::linear_sample.
//
// AbsoluteMap: the float64 absolute source map that the caller prepared.
struct AbsoluteMap {
  const double* m;
  template <int DIM>
  __device__ __forceinline__ const double* channel(int d, long long nodes, const double*) const {
    return m + (long long)(DIM - 1 - d) * nodes;
  }
};
// RelativeMapArgs: the relative map in its own type; the absolute value of a node
// is formed on every read (sfm::RelativeMap).  shift and scale are per channel.
template <typename M>
struct RelativeMapArgs {
  const M* m;
  int has_shift;
  double shift[3], scale[3];
  template <int DIM>
  __device__ __forceinline__ sfm::RelativeMap<M, DIM> channel(int d, long long nodes,
                                                              const double* stride) const {
    const int c = DIM - 1 - d;
    return {m + (long long)c * nodes, d, has_shift != 0, stride[3 - DIM + d], shift[c], scale[c]};
  }
};

template <typename MAP>
struct NdWarpArgs {
  const void* image;
  MAP map;
  void* out;
  int order;
  int ishape[3], mshape[3], oshape[3];
  double stride[3], offset[3];
};

// ORDER 0: a.order (0 or 1) on the image; ORDER 2 .. 5: a.image holds the float64
// B-spline coefficients of the image (sfm_spline_prefilter).
template <int DIM, typename T, int ORDER, typename MAP>
__global__ void __launch_bounds__(kBlock) ndimage_warp_kernel(NdWarpArgs<MAP> a) {
  const long long n = (long long)a.oshape[0] * a.oshape[1] * a.oshape[2];
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  int o[3];
  o[2] = static_cast<int>(i % a.oshape[2]);
  o[1] = static_cast<int>((i / a.oshape[2]) % a.oshape[1]);
  o[0] = static_cast<int>(i / ((long long)a.oshape[2] * a.oshape[1]));
  // node-space position (warp.py:300-301)
  double pos[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const int ax = 3 - DIM + d;
    pos[d] = (static_cast<double>(o[ax]) - a.offset[ax]) / a.stride[ax];
  }
  // dense coordinates z, y, x = channels DIM - 1 ... 0 of the map (warp.py:304-307)
  const long long nodes = (long long)a.mshape[0] * a.mshape[1] * a.mshape[2];
  double dense[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d)
    dense[d] = sfm::linear_sample<DIM>(a.map.template channel<DIM>(d, nodes, a.stride), a.mshape,
                                       pos);
  double v;
  if constexpr (ORDER >= 2) {
    v = sfm::spline_sample<DIM, ORDER>(static_cast<const double*>(a.image), a.ishape, dense);
  } else {
    const T* img = static_cast<const T*>(a.image);
    v = a.order == 0 ? sfm::nearest_sample<DIM>(img, a.ishape, dense)
                     : sfm::linear_sample<DIM>(img, a.ishape, dense);
  }
  constexpr double vmax = sizeof(T) == 1 ? 255.0 : 65535.0;
  static_cast<T*>(a.out)[i] = sfm::nd_convert<T>(v, vmax);
}

// The same with SciPy's boundary mode and fill value on BOTH steps, as the
// reference hands one map_coordinates callable to both (warp.py:308-314): outside
// the node grid the dense coordinate is cval (in source voxels) or the folded
// node value, and the image sample follows the same rule; an integer image takes
// cval through nd_convert like a sampled value.
//
// TAPS: orders 2 .. 5 under the modes beyond "constant", "mirror" and "wrap"
// (spline_sample<.., TAPS>): kernels of their own, which the three modes never run.
template <int DIM, typename T, int ORDER, typename MAP, bool TAPS = false>
__global__ void __launch_bounds__(kBlock)
ndimage_warp_mode_kernel(NdWarpArgs<MAP> a, sfm::Boundary b) {
  const long long n = (long long)a.oshape[0] * a.oshape[1] * a.oshape[2];
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  int o[3];
  o[2] = static_cast<int>(i % a.oshape[2]);
  o[1] = static_cast<int>((i / a.oshape[2]) % a.oshape[1]);
  o[0] = static_cast<int>(i / ((long long)a.oshape[2] * a.oshape[1]));
  double pos[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const int ax = 3 - DIM + d;
    pos[d] = (static_cast<double>(o[ax]) - a.offset[ax]) / a.stride[ax];
  }
  const long long nodes = (long long)a.mshape[0] * a.mshape[1] * a.mshape[2];
  double dense[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d)
    dense[d] = sfm::linear_sample<DIM, true>(a.map.template channel<DIM>(d, nodes, a.stride),
                                             a.mshape, pos, nullptr, b);
  double v;
  if constexpr (ORDER >= 2) {
    if constexpr (TAPS) {
      // "nearest" / "grid-constant": a.image holds the coefficients of the padded image
      // and a.ishape its shape; the map step above is order 1 and unpadded
      if (b.pad) {
#pragma unroll
        for (int d = 0; d < DIM; ++d)     // (the magnitude limit is that of the caller's coordinate)
        dense[d] = fabs(dense[d]) < 2147483648.0 ? dense[d] + static_cast<double>(b.pad)
                                                 : static_cast<double>(NAN);
      }
    }
    v = sfm::spline_sample<DIM, ORDER, true, TAPS>(static_cast<const double*>(a.image),
                                                   a.ishape, dense, nullptr, b);
  } else {
    const T* img = static_cast<const T*>(a.image);
    v = a.order == 0 ? sfm::nearest_sample<DIM, true>(img, a.ishape, dense, nullptr, b)
                     : sfm::linear_sample<DIM, true>(img, a.ishape, dense, nullptr, b);
  }
  constexpr double vmax = sizeof(T) == 1 ? 255.0 : 65535.0;
  static_cast<T*>(a.out)[i] = sfm::nd_convert<T>(v, vmax);
}

// What the samplers take: a mode of the list; orders 2 .. 5 only the modes whose
// coefficients sfm_spline_prefilter computes, and with the switch SFM_SPLINE_MODES
// the others, on the coefficients of sfm_spline_prefilter_mode; a finite fill value
// for integers (the conversion of NaN or an infinity to an integer is undefined).
int check_boundary(const char* what, int mode, double cval, int order, int dtype) {
  if (mode < 0 || mode >= sfm::kModeCount)
    return sfm::fail(SFM_ERR_INVALID, "%s: boundary mode %d", what, mode);
  if (order >= 2 && mode != sfm::kModeConstant && mode != sfm::kModeMirror &&
      mode != sfm::kModeWrap && !sfm::spline_modes_enabled())
    return sfm::fail(SFM_ERR_INVALID,
                     "%s: boundary mode %d at order %d (constant, mirror and wrap are built; "
                     "the others need the switch SFM_SPLINE_MODES=1)",
                     what, mode, order);
  if (dtype != SFM_DTYPE_F32 && !std::isfinite(cval))
    return sfm::fail(SFM_ERR_INVALID, "%s: non-finite cval for an integer image", what);
  return SFM_OK;
}

// orders 2 .. 5: the modes whose taps do not mirror (the TAPS kernels)
bool spline_taps(int mode) {
  return mode != sfm::kModeConstant && mode != sfm::kModeMirror && mode != sfm::kModeWrap;
}

// The Boundary of a checked mode: orders 2 .. 5 under "nearest" and "grid-constant"
// read the coefficients of the padded image.
sfm::Boundary make_boundary(int mode, double cval, int order) {
  sfm::Boundary b;
  b.mode = mode;
  b.cval = cval;
  b.pad = order >= 2 ? sfm_spline_mode_pad(mode) : 0;
  return b;
}

}  // namespace

namespace {

// the checks and the launch of sfm_ndimage_warp (orders 0, 1 on the image),
// sfm_ndimage_warp_spline (orders 2 .. 5 on coefficients) and, with a Boundary,
// sfm_ndimage_warp_mode (either)
//
// D is SfmNdWarpDesc with MAP = AbsoluteMap, or SfmNdWarpRelDesc (sfm_ndimage_warp_rel)
// with MAP = RelativeMapArgs<float | double>: the two descriptors name the fields
// read here alike, and `map` is checked and filled by the caller.
template <typename D, typename MAP>
int ndimage_warp_launch(const D* d, const MAP& map, bool spline,
                        const sfm::Boundary* bnd = nullptr) {
  if (!d || !d->image || !map.m || !d->out)
    return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: NULL argument");
  if (d->ndim != 2 && d->ndim != 3) return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: ndim %d", d->ndim);
  if (!spline && d->order != 0 && d->order != 1)
    return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: interpolation order %d (0 and 1 are built)",
                     d->order);
  if (spline && (d->order < 2 || d->order > 5))
    return sfm::fail(SFM_ERR_INVALID, "ndimage_warp_spline: interpolation order %d (2 .. 5)",
                     d->order);
  NdWarpArgs<MAP> a;
  a.image = d->image;
  a.map = map;
  a.out = d->out;
  a.order = d->order;
  long long n = 1;
  for (int k = 0; k < 3; ++k) {
    if (d->image_shape[k] < 1 || d->map_shape[k] < 1 || d->out_shape[k] < 1)
      return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: bad shape");
    if (d->ndim == 2 && k == 0 &&
        (d->image_shape[0] != 1 || d->map_shape[0] != 1 || d->out_shape[0] != 1))
      return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: 2-d arrays have shape[0] = 1");
    if (k >= 3 - d->ndim && !(d->stride[k] != 0.0))
      return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: stride");
    a.ishape[k] = d->image_shape[k];
    if (bnd && bnd->pad && k >= 3 - d->ndim) {
      if (d->image_shape[k] > 0x7fffffff - 2 * bnd->pad)
        return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: bad shape");
      a.ishape[k] += 2 * bnd->pad;
    }
    a.mshape[k] = d->map_shape[k];
    a.oshape[k] = d->out_shape[k];
    a.stride[k] = d->stride[k];
    a.offset[k] = d->offset[k];
    n *= d->out_shape[k];
  }
  const long long grid = (n + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: too large");
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const dim3 g(static_cast<unsigned>(grid)), b(kBlock);
  const bool taps = bnd && spline && spline_taps(bnd->mode);
#define SFM_NDW_ORDER(T, ORDER)                                                    \
  do {                                                                             \
    if (taps && d->ndim == 2)                                                      \
      hipLaunchKernelGGL((ndimage_warp_mode_kernel<2, T, ORDER, MAP, (ORDER >= 2)>), g, b, 0, \
                         st, a, *bnd);                                             \
    else if (taps)                                                                 \
      hipLaunchKernelGGL((ndimage_warp_mode_kernel<3, T, ORDER, MAP, (ORDER >= 2)>), g, b, 0, \
                         st, a, *bnd);                                             \
    else if (bnd && d->ndim == 2)                                                  \
      hipLaunchKernelGGL((ndimage_warp_mode_kernel<2, T, ORDER, MAP>), g, b, 0, st, a, *bnd); \
    else if (bnd)                                                                  \
      hipLaunchKernelGGL((ndimage_warp_mode_kernel<3, T, ORDER, MAP>), g, b, 0, st, a, *bnd); \
    else if (d->ndim == 2)                                                         \
      hipLaunchKernelGGL((ndimage_warp_kernel<2, T, ORDER, MAP>), g, b, 0, st, a);      \
    else                                                                           \
      hipLaunchKernelGGL((ndimage_warp_kernel<3, T, ORDER, MAP>), g, b, 0, st, a);      \
  } while (0)
#define SFM_NDW(T)                                                                 \
  do {                                                                             \
    switch (spline ? d->order : 0) {                                               \
      case 2: SFM_NDW_ORDER(T, 2); break;                                          \
      case 3: SFM_NDW_ORDER(T, 3); break;                                          \
      case 4: SFM_NDW_ORDER(T, 4); break;                                          \
      case 5: SFM_NDW_ORDER(T, 5); break;                                          \
      default: SFM_NDW_ORDER(T, 0); break;                                         \
    }                                                                              \
  } while (0)
  switch (d->dtype) {
    case SFM_DTYPE_U8: SFM_NDW(unsigned char); break;
    case SFM_DTYPE_U16: SFM_NDW(unsigned short); break;
    case SFM_DTYPE_F32: SFM_NDW(float); break;
    default: return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: dtype %d", d->dtype);
  }
#undef SFM_NDW
#undef SFM_NDW_ORDER
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace

extern "C" int sfm_ndimage_warp(const SfmNdWarpDesc* d) {
  return ndimage_warp_launch(d, AbsoluteMap{d ? d->src_map : nullptr}, false);
}

extern "C" int sfm_ndimage_warp_spline(const SfmNdWarpDesc* d) {
  return ndimage_warp_launch(d, AbsoluteMap{d ? d->src_map : nullptr}, true);
}

extern "C" int sfm_ndimage_warp_mode(const SfmNdWarpDesc* d, int32_t mode, double cval) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "ndimage_warp_mode: NULL argument");
  if (d->order < 0 || d->order > 5)
    return sfm::fail(SFM_ERR_INVALID, "ndimage_warp_mode: interpolation order %d (0 .. 5)",
                     d->order);
  if (int rc = check_boundary("ndimage_warp_mode", mode, cval, d->order, d->dtype)) return rc;
  const sfm::Boundary b = make_boundary(mode, cval, d->order);
  return ndimage_warp_launch(d, AbsoluteMap{d->src_map}, d->order >= 2, &b);
}

namespace {

template <typename M>
int ndimage_warp_rel_launch(const SfmNdWarpRelDesc* d, const sfm::Boundary* bnd) {
  RelativeMapArgs<M> map;
  map.m = static_cast<const M*>(d->rel_map);
  map.has_shift = d->has_shift ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    map.shift[c] = d->shift[c];
    map.scale[c] = d->scale[c];
  }
  return ndimage_warp_launch(d, map, d->order >= 2, bnd);
}

}  // namespace

extern "C" int sfm_ndimage_warp_rel(const SfmNdWarpRelDesc* d) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "ndimage_warp_rel: NULL argument");
  if (d->order < 0 || d->order > 5)
    return sfm::fail(SFM_ERR_INVALID, "ndimage_warp_rel: interpolation order %d (0 .. 5)",
                     d->order);
  sfm::Boundary b;
  if (d->has_boundary) {
    if (int rc = check_boundary("ndimage_warp_rel", d->mode, d->cval, d->order, d->dtype))
      return rc;
    b = make_boundary(d->mode, d->cval, d->order);
  }
  const sfm::Boundary* bnd = d->has_boundary ? &b : nullptr;
  return d->map_f64 ? ndimage_warp_rel_launch<double>(d, bnd)
                    : ndimage_warp_rel_launch<float>(d, bnd);
}

// ---------------------------------------------------------------------------
// scipy.ndimage.affine_transform with a [dim, dim] matrix: the source coordinate
// of an output voxel is a matrix product and an offset, formed in double from
// kernel arguments (scalar registers) -- products added in axis order onto 0,
// the offset last, which is SciPy's rounding -- and handed to the samplers.  No
// coordinate map exists.  One thread per output voxel, a wave per 64 contiguous
// voxels, as in ndimage_warp_kernel.
// ---------------------------------------------------------------------------
namespace {

struct AffineArgs {
  const void* image;
  void* out;
  int order;
  int shape[3];     // of out
  int ishape[3];    // of what is sampled: shape, or with b.pad the padded coefficients
  double m[3][3], off[3];
  sfm::Boundary b;
};

template <int DIM, typename T, int ORDER = 0, bool TAPS = false>
__global__ void __launch_bounds__(kBlock) affine_warp_kernel(AffineArgs a) {
  const long long n = (long long)a.shape[0] * a.shape[1] * a.shape[2];
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  int o[3];
  o[2] = static_cast<int>(i % a.shape[2]);
  o[1] = static_cast<int>((i / a.shape[2]) % a.shape[1]);
  o[0] = static_cast<int>(i / ((long long)a.shape[2] * a.shape[1]));
  double c[DIM];
#pragma unroll
  for (int h = 0; h < DIM; ++h) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k)
      acc = acc + static_cast<double>(o[3 - DIM + k]) * a.m[3 - DIM + h][3 - DIM + k];
    c[h] = acc + a.off[3 - DIM + h];
  }
  double v;
  if constexpr (ORDER >= 2) {
    if constexpr (TAPS) {
      if (a.b.pad) {                     // after the offset, as SciPy adds it
#pragma unroll
        for (int h = 0; h < DIM; ++h)     // (the magnitude limit is that of the unshifted coordinate)
        c[h] = fabs(c[h]) < 2147483648.0 ? c[h] + static_cast<double>(a.b.pad)
                                         : static_cast<double>(NAN);
      }
    }
    v = sfm::spline_sample<DIM, ORDER, true, TAPS>(static_cast<const double*>(a.image), a.ishape,
                                                   c, nullptr, a.b);
  } else {
    const T* img = static_cast<const T*>(a.image);
    v = a.order == 0 ? sfm::nearest_sample<DIM, true>(img, a.ishape, c, nullptr, a.b)
                     : sfm::linear_sample<DIM, true>(img, a.ishape, c, nullptr, a.b);
  }
  constexpr double vmax = sizeof(T) == 1 ? 255.0 : 65535.0;
  static_cast<T*>(a.out)[i] = sfm::nd_convert<T>(v, vmax);
}

}  // namespace

extern "C" int sfm_affine_warp(const SfmAffineWarpDesc* d) {
  if (!d || !d->image || !d->out) return sfm::fail(SFM_ERR_INVALID, "affine_warp: NULL argument");
  if (d->ndim != 2 && d->ndim != 3) return sfm::fail(SFM_ERR_INVALID, "affine_warp: ndim %d", d->ndim);
  if (d->order < 0 || d->order > 5)
    return sfm::fail(SFM_ERR_INVALID, "affine_warp: interpolation order %d (0 .. 5)", d->order);
  if (int rc = check_boundary("affine_warp", d->mode, d->cval, d->order, d->dtype)) return rc;
  AffineArgs a;
  a.image = d->image;
  a.out = d->out;
  a.order = d->order;
  a.b = make_boundary(d->mode, d->cval, d->order);
  long long n = 1;
  for (int k = 0; k < 3; ++k) {
    if (d->shape[k] < 1) return sfm::fail(SFM_ERR_INVALID, "affine_warp: bad shape");
    if (d->ndim == 2 && k == 0 && d->shape[0] != 1)
      return sfm::fail(SFM_ERR_INVALID, "affine_warp: 2-d arrays have shape[0] = 1");
    a.shape[k] = a.ishape[k] = d->shape[k];
    if (a.b.pad && k >= 3 - d->ndim) {
      if (d->shape[k] > 0x7fffffff - 2 * a.b.pad)
        return sfm::fail(SFM_ERR_INVALID, "affine_warp: bad shape");
      a.ishape[k] += 2 * a.b.pad;
    }
    a.off[k] = d->offset[k];
    for (int j = 0; j < 3; ++j) a.m[k][j] = d->matrix[3 * k + j];
    n *= d->shape[k];
  }
  const long long grid = (n + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "affine_warp: too large");
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const dim3 g(static_cast<unsigned>(grid)), b(kBlock);
  const bool taps = d->order >= 2 && spline_taps(d->mode);
#define SFM_AFF_ORDER(T, ORDER)                                                    \
  do {                                                                             \
    if (taps && d->ndim == 2)                                                      \
      hipLaunchKernelGGL((affine_warp_kernel<2, T, ORDER, (ORDER >= 2)>), g, b, 0, st, a); \
    else if (taps)                                                                 \
      hipLaunchKernelGGL((affine_warp_kernel<3, T, ORDER, (ORDER >= 2)>), g, b, 0, st, a); \
    else if (d->ndim == 2)                                                         \
      hipLaunchKernelGGL((affine_warp_kernel<2, T, ORDER>), g, b, 0, st, a);       \
    else                                                                           \
      hipLaunchKernelGGL((affine_warp_kernel<3, T, ORDER>), g, b, 0, st, a);       \
  } while (0)
#define SFM_AFF(T)                                                                 \
  do {                                                                             \
    switch (d->order) {                                                            \
      case 2: SFM_AFF_ORDER(T, 2); break;                                          \
      case 3: SFM_AFF_ORDER(T, 3); break;                                          \
      case 4: SFM_AFF_ORDER(T, 4); break;                                          \
      case 5: SFM_AFF_ORDER(T, 5); break;                                          \
      default: SFM_AFF_ORDER(T, 0); break;                                         \
    }                                                                              \
  } while (0)
  switch (d->dtype) {
    case SFM_DTYPE_U8: SFM_AFF(unsigned char); break;
    case SFM_DTYPE_U16: SFM_AFF(unsigned short); break;
    case SFM_DTYPE_F32: SFM_AFF(float); break;
    default: return sfm::fail(SFM_ERR_INVALID, "affine_warp: dtype %d", d->dtype);
  }
#undef SFM_AFF
#undef SFM_AFF_ORDER
  SFM_LAUNCH_CHECK();
  return SFM_OK;
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
namespace {

constexpr int kBrickX = 64, kBrickY = 4;

struct RenderArgs {
  const SfmRenderTile* tiles;
  const double* coeffs;   // spline orders: the crops' coefficients, back to back
  void* out;
  int n_tiles, order;
  int oshape[3];
  double stride[3];
};

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
  constexpr double vmax = sizeof(T) == 1 ? 255.0 : 65535.0;
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
      const sfm::ShiftedMap m = {r.abs_map + (long long)(2 - d) * nodes, r.shift[2 - d]};
      dense[d] = sfm::linear_sample<3>(m, r.map_shape, pos);
    }
    // the image region data_box, read in place
    const long long ipitch[3] = {(long long)r.tile_shape[1] * r.tile_shape[2], r.tile_shape[2], 1};
    const long long wpitch[3] = {0, r.tile_shape[2], 1};
    const long long worg = (long long)r.data_start[1] * r.tile_shape[2] + r.data_start[2];
    double v;
    if constexpr (ORDER >= 2) {
      v = sfm::spline_sample<3, ORDER>(a.coeffs + region, r.data_size, dense);
    } else {
      const T* im = static_cast<const T*>(r.image) + r.data_start[0] * ipitch[0] + worg;
      v = a.order == 0 ? sfm::nearest_sample<3>(im, r.data_size, dense, ipitch)
                       : sfm::linear_sample<3>(im, r.data_size, dense, ipitch);
    }
    const T iv = sfm::nd_convert<T>(v, vmax);
    // the weights: the 2-D array repeated over data_size[0] planes, order 1
    const float w = sfm::nd_convert<float>(
        sfm::linear_sample<3>(r.weights + worg, r.data_size, dense, wpitch), 0.0);
    img = img + static_cast<float>(iv) * w;
    norm = norm + w;
  }
  if (!live) return;
  if (norm > 0.f) img = img / norm;
  static_cast<O*>(a.out)[((long long)z * a.oshape[1] + y) * a.oshape[2] + x] = render_cast<O>(img);
}

}  // namespace

namespace {

// the checks and the launch of sfm_render_tiles3d (coeffs NULL: orders 0, 1) and
// sfm_render_tiles3d_spline (orders 2 .. 5)
int render_tiles_launch(const SfmRenderTilesDesc* d, const double* coeffs, bool spline) {
  if (!d || !d->out) return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: NULL argument");
  if (d->n_tiles < 0) return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: n_tiles %d", d->n_tiles);
  if (d->n_tiles > 0 && (!d->tiles || !d->tiles_host))
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: NULL tile table");
  if (!spline && d->order != 0 && d->order != 1)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: interpolation order %d (0 and 1 are built)",
                     d->order);
  if (spline && (d->order < 2 || d->order > 5))
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d_spline: interpolation order %d (2 .. 5)",
                     d->order);
  if (spline && d->n_tiles > 0 && !coeffs)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d_spline: NULL coefficients");
  if (d->dtype != SFM_DTYPE_U8 && d->dtype != SFM_DTYPE_U16 && d->dtype != SFM_DTYPE_F32)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: dtype %d", d->dtype);
  if (d->out_dtype != d->dtype && d->out_dtype != SFM_DTYPE_F32)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: out_dtype %d for tiles of dtype %d",
                     d->out_dtype, d->dtype);
  RenderArgs a;
  a.tiles = d->tiles;
  a.coeffs = coeffs;
  a.out = d->out;
  a.n_tiles = d->n_tiles;
  a.order = d->order;
  for (int k = 0; k < 3; ++k) {
    if (d->out_shape[k] < 1) return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: bad out_shape");
    if (!(d->stride[k] != 0.0)) return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: stride");
    a.oshape[k] = d->out_shape[k];
    a.stride[k] = d->stride[k];
  }
  // every box of the table lies inside the array it indexes
  for (int t = 0; t < d->n_tiles; ++t) {
    const SfmRenderTile& r = d->tiles_host[t];
    if ((!spline && !r.image) || !r.abs_map || !r.weights)
      return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: tile %d: NULL array", t);
    for (int k = 0; k < 3; ++k) {
      if (r.tile_shape[k] < 1 || r.map_shape[k] < 1 || r.data_size[k] < 1 || r.sub_size[k] < 1)
        return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: tile %d: bad shape", t);
      if (r.data_start[k] < 0 ||
          (long long)r.data_start[k] + r.data_size[k] > r.tile_shape[k])
        return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: tile %d: data_box leaves the tile", t);
      if (r.sub_start[k] < 0 || (long long)r.sub_start[k] + r.sub_size[k] > d->out_shape[k])
        return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: tile %d: sub_box leaves the output", t);
    }
  }
  const long long gx = (a.oshape[2] + kBrickX - 1) / kBrickX;
  const long long gy = (a.oshape[1] + kBrickY - 1) / kBrickY;
  if (gy > 65535 || a.oshape[0] > 65535)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: too large");
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const dim3 g(static_cast<unsigned>(gx), static_cast<unsigned>(gy),
               static_cast<unsigned>(a.oshape[0])), b(kBrickX, kBrickY);
#define SFM_RT_ORDER(T, ORDER)                                                   \
  do {                                                                           \
    if (d->out_dtype == d->dtype)                                                \
      hipLaunchKernelGGL((render_tiles_kernel<T, T, ORDER>), g, b, 0, st, a);    \
    else                                                                         \
      hipLaunchKernelGGL((render_tiles_kernel<T, float, ORDER>), g, b, 0, st, a); \
  } while (0)
#define SFM_RT(T)                                                                \
  do {                                                                           \
    switch (spline ? d->order : 0) {                                             \
      case 2: SFM_RT_ORDER(T, 2); break;                                         \
      case 3: SFM_RT_ORDER(T, 3); break;                                         \
      case 4: SFM_RT_ORDER(T, 4); break;                                         \
      case 5: SFM_RT_ORDER(T, 5); break;                                         \
      default: SFM_RT_ORDER(T, 0); break;                                        \
    }                                                                            \
  } while (0)
  switch (d->dtype) {
    case SFM_DTYPE_U8: SFM_RT(unsigned char); break;
    case SFM_DTYPE_U16: SFM_RT(unsigned short); break;
    default: SFM_RT(float); break;
  }
#undef SFM_RT
#undef SFM_RT_ORDER
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace

extern "C" int sfm_render_tiles3d(const SfmRenderTilesDesc* d) {
  return render_tiles_launch(d, nullptr, false);
}

extern "C" int sfm_render_tiles3d_spline(const SfmRenderTilesDesc* d, const double* coeffs) {
  return render_tiles_launch(d, coeffs, true);
}
