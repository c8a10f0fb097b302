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
//
// Below it: the host side of the map_coordinates family (sfm_ndwarp.h).
#include "sfm_common.h"
#include "sfm_ndwarp.h"

#include <cmath>
#include <initializer_list>
#include <type_traits>

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
// The map_coordinates family (sfm_ndwarp.h): warp.ndimage_warp, orders 0 .. 5,
// scipy.ndimage.affine_transform and the 3-D tile render.  Here the entry points
// and their checks; the kernels are in the units sfm_ndwarp_o*.hip, one per entry
// of SFM_NDWARP_UNITS.
// ---------------------------------------------------------------------------
namespace {

using sfm::kBrickX;
using sfm::kBrickY;

// f(ORDER, DIM), as integral constants, for the unit that holds the kernels of
// `order` in `ndim` dimensions: the one place that maps a launch to a unit.
template <typename F>
int for_unit(int order, int ndim, F&& f) {
  const int unit = order >= 2 ? order : 0;
#define SFM_NDWARP_CASE(ORDER, DIM)    \
  if (unit == ORDER && ndim == DIM)    \
    return f(std::integral_constant<int, ORDER>(), std::integral_constant<int, DIM>());
  SFM_NDWARP_UNITS(SFM_NDWARP_CASE)
#undef SFM_NDWARP_CASE
  return sfm::fail(SFM_ERR_INVALID, "no kernel of order %d in %d dimensions", order, ndim);
}

int check_order(const char* what, int order, int lo, int hi) {
  if (order >= lo && order <= hi) return SFM_OK;
  if (hi == 1)
    return sfm::fail(SFM_ERR_INVALID, "%s: interpolation order %d (0 and 1 are built)", what,
                     order);
  return sfm::fail(SFM_ERR_INVALID, "%s: interpolation order %d (%d .. %d)", what, order, lo, hi);
}

// Axis k of the arrays of a launch: lengths of 1 and more, and a 2-D array is
// [1, y, x].
int check_axis(const char* what, int ndim, int k, std::initializer_list<int> lens) {
  for (int len : lens)
    if (len < 1) return sfm::fail(SFM_ERR_INVALID, "%s: bad shape", what);
  if (ndim == 2 && k == 0)
    for (int len : lens)
      if (len != 1) return sfm::fail(SFM_ERR_INVALID, "%s: 2-d arrays have shape[0] = 1", what);
  return SFM_OK;
}

// The length of axis k of what the image step samples: with b.pad the coefficients
// of the padded image (the axes in use only).
int padded_len(const char* what, int ndim, int k, int len, int pad, int* padded) {
  *padded = len;
  if (pad && k >= 3 - ndim) {
    if (len > 0x7fffffff - 2 * pad) return sfm::fail(SFM_ERR_INVALID, "%s: bad shape", what);
    *padded += 2 * pad;
  }
  return SFM_OK;
}

// The launch of a kernel with one thread per output voxel, n of them.
int voxel_launch(const char* what, long long n, int dtype, void* stream, sfm::NdLaunch* l) {
  const long long grid = (n + sfm::kNdBlock - 1) / sfm::kNdBlock;
  if (grid > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "%s: too large", what);
  if (dtype != SFM_DTYPE_U8 && dtype != SFM_DTYPE_U16 && dtype != SFM_DTYPE_F32)
    return sfm::fail(SFM_ERR_INVALID, "%s: dtype %d", what, dtype);
  *l = {dim3(static_cast<unsigned>(grid)), dim3(sfm::kNdBlock), static_cast<hipStream_t>(stream),
        dtype};
  return SFM_OK;
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
bool spline_taps(int order, int mode) {
  return order >= 2 && mode != sfm::kModeConstant && mode != sfm::kModeMirror &&
         mode != sfm::kModeWrap;
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
  if (int rc = spline ? check_order("ndimage_warp_spline", d->order, 2, 5)
                      : check_order("ndimage_warp", d->order, 0, 1))
    return rc;
  sfm::NdWarpArgs<MAP> a;
  a.image = d->image;
  a.map = map;
  a.out = d->out;
  a.order = d->order;
  long long n = 1;
  for (int k = 0; k < 3; ++k) {
    if (int rc = check_axis("ndimage_warp", d->ndim, k,
                            {d->image_shape[k], d->map_shape[k], d->out_shape[k]}))
      return rc;
    if (k >= 3 - d->ndim && !(d->stride[k] != 0.0))
      return sfm::fail(SFM_ERR_INVALID, "ndimage_warp: stride");
    if (int rc = padded_len("ndimage_warp", d->ndim, k, d->image_shape[k], bnd ? bnd->pad : 0,
                            &a.ishape[k]))
      return rc;
    a.mshape[k] = d->map_shape[k];
    a.oshape[k] = d->out_shape[k];
    a.stride[k] = d->stride[k];
    a.offset[k] = d->offset[k];
    n *= d->out_shape[k];
  }
  sfm::NdLaunch l;
  if (int rc = voxel_launch("ndimage_warp", n, d->dtype, d->stream, &l)) return rc;
  const bool taps = bnd && spline_taps(d->order, bnd->mode);
  return for_unit(d->order, d->ndim, [&](auto order, auto dim) {
    return sfm::launch_ndwarp<decltype(order)::value, decltype(dim)::value>(a, bnd, taps, l);
  });
}

template <typename M>
int ndimage_warp_rel_launch(const SfmNdWarpRelDesc* d, const sfm::Boundary* bnd) {
  sfm::RelativeMapArgs<M> map;
  map.m = static_cast<const M*>(d->rel_map);
  map.has_shift = d->has_shift ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    map.shift[c] = d->shift[c];
    map.scale[c] = d->scale[c];
  }
  return ndimage_warp_launch(d, map, d->order >= 2, bnd);
}

}  // namespace

extern "C" int sfm_ndimage_warp(const SfmNdWarpDesc* d) {
  return ndimage_warp_launch(d, sfm::AbsoluteMap{d ? d->src_map : nullptr}, false);
}

extern "C" int sfm_ndimage_warp_spline(const SfmNdWarpDesc* d) {
  return ndimage_warp_launch(d, sfm::AbsoluteMap{d ? d->src_map : nullptr}, true);
}

extern "C" int sfm_ndimage_warp_mode(const SfmNdWarpDesc* d, int32_t mode, double cval) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "ndimage_warp_mode: NULL argument");
  if (int rc = check_order("ndimage_warp_mode", d->order, 0, 5)) return rc;
  if (int rc = check_boundary("ndimage_warp_mode", mode, cval, d->order, d->dtype)) return rc;
  const sfm::Boundary b = make_boundary(mode, cval, d->order);
  return ndimage_warp_launch(d, sfm::AbsoluteMap{d->src_map}, d->order >= 2, &b);
}

extern "C" int sfm_ndimage_warp_rel(const SfmNdWarpRelDesc* d) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "ndimage_warp_rel: NULL argument");
  if (int rc = check_order("ndimage_warp_rel", d->order, 0, 5)) return rc;
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

extern "C" int sfm_affine_warp(const SfmAffineWarpDesc* d) {
  if (!d || !d->image || !d->out) return sfm::fail(SFM_ERR_INVALID, "affine_warp: NULL argument");
  if (d->ndim != 2 && d->ndim != 3) return sfm::fail(SFM_ERR_INVALID, "affine_warp: ndim %d", d->ndim);
  if (int rc = check_order("affine_warp", d->order, 0, 5)) return rc;
  if (int rc = check_boundary("affine_warp", d->mode, d->cval, d->order, d->dtype)) return rc;
  sfm::AffineArgs a;
  a.image = d->image;
  a.out = d->out;
  a.order = d->order;
  a.b = make_boundary(d->mode, d->cval, d->order);
  long long n = 1;
  for (int k = 0; k < 3; ++k) {
    if (int rc = check_axis("affine_warp", d->ndim, k, {d->shape[k]})) return rc;
    a.shape[k] = d->shape[k];
    if (int rc = padded_len("affine_warp", d->ndim, k, d->shape[k], a.b.pad, &a.ishape[k]))
      return rc;
    a.off[k] = d->offset[k];
    for (int j = 0; j < 3; ++j) a.m[k][j] = d->matrix[3 * k + j];
    n *= d->shape[k];
  }
  sfm::NdLaunch l;
  if (int rc = voxel_launch("affine_warp", n, d->dtype, d->stream, &l)) return rc;
  const bool taps = spline_taps(d->order, d->mode);
  return for_unit(d->order, d->ndim, [&](auto order, auto dim) {
    return sfm::launch_affine<decltype(order)::value, decltype(dim)::value>(a, taps, l);
  });
}

namespace {

// the checks and the launch of sfm_render_tiles3d (coeffs NULL: orders 0, 1) and
// sfm_render_tiles3d_spline (orders 2 .. 5)
int render_tiles_launch(const SfmRenderTilesDesc* d, const double* coeffs, bool spline) {
  if (!d || !d->out) return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: NULL argument");
  if (d->n_tiles < 0) return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: n_tiles %d", d->n_tiles);
  if (d->n_tiles > 0 && (!d->tiles || !d->tiles_host))
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: NULL tile table");
  if (int rc = spline ? check_order("render_tiles3d_spline", d->order, 2, 5)
                      : check_order("render_tiles3d", d->order, 0, 1))
    return rc;
  if (spline && d->n_tiles > 0 && !coeffs)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d_spline: NULL coefficients");
  if (d->dtype != SFM_DTYPE_U8 && d->dtype != SFM_DTYPE_U16 && d->dtype != SFM_DTYPE_F32)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: dtype %d", d->dtype);
  if (d->out_dtype != d->dtype && d->out_dtype != SFM_DTYPE_F32)
    return sfm::fail(SFM_ERR_INVALID, "render_tiles3d: out_dtype %d for tiles of dtype %d",
                     d->out_dtype, d->dtype);
  sfm::RenderArgs a;
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
  const sfm::NdLaunch l = {dim3(static_cast<unsigned>(gx), static_cast<unsigned>(gy),
                                static_cast<unsigned>(a.oshape[0])),
                           dim3(kBrickX, kBrickY), static_cast<hipStream_t>(d->stream), d->dtype};
  return for_unit(d->order, 3, [&](auto order, auto) {
    return sfm::launch_render<decltype(order)::value>(a, d->out_dtype != d->dtype, l);
  });
}

}  // namespace

extern "C" int sfm_render_tiles3d(const SfmRenderTilesDesc* d) {
  return render_tiles_launch(d, nullptr, false);
}

extern "C" int sfm_render_tiles3d_spline(const SfmRenderTilesDesc* d, const double* coeffs) {
  return render_tiles_launch(d, coeffs, true);
}

