// scipy.ndimage.map_coordinates on the device, orders 0 to 5, mode "constant",
// cval 0: the samplers shared by ndimage_warp_kernel and render_tiles_kernel
// (sfm_warp.hip).  Orders 0 and 1 read the image, orders 2 to 5 its float64
// B-spline coefficients (sfm_spline.hip).  Double arithmetic in SciPy's operation
// order; the units that include this are built with -ffp-contract=off.
//
// `a` is anything indexable by a linear element offset whose elements widen to
// double: a pointer, or a view such as ShiftedMap below.  `shape` holds 3
// entries (z, y, x; the last DIM are used) and is what coordinates are tested
// against.  `pitch`, when given, holds the element distance per axis in the same
// layout: a region of a larger array is then sampled in place (the region's
// origin is folded into `a`), and a 2-D array is read as a stack of identical
// planes with pitch 0.  Without it the array is dense in `shape`.
#ifndef SFM_NDSAMPLE_H_
#define SFM_NDSAMPLE_H_

#include <hip/hip_runtime.h>

namespace sfm {

// scipy NI_GeometricTransform, order 1, mode "constant", cval 0: outside
// [0, len - 1] on any axis, NaN included -> 0; the tap beyond the last sample
// (coordinate exactly len - 1) carries weight 0 and is read mirrored, from
// len - 2, as SciPy's edge mapping does: 0 x inf and 0 x NaN there are NaN.
template <int DIM, typename A>
__device__ __forceinline__ double linear_sample(const A a, const int* shape, const double* c,
                                                const long long* pitch = nullptr) {
  long long base[DIM];
  double w[DIM][2];
  long long dense = 1;
  long long step[DIM];
#pragma unroll
  for (int d = DIM - 1; d >= 0; --d) {
    step[d] = pitch ? pitch[3 - DIM + d] : dense;
    dense *= shape[3 - DIM + d];
  }
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const int len = shape[3 - DIM + d];
    if (!(c[d] >= 0.0 && c[d] <= static_cast<double>(len - 1))) return 0.0;
    const double fl = floor(c[d]);
    const double t = c[d] - fl;
    w[d][0] = 1.0 - t;
    w[d][1] = 1.0 - w[d][0];
    base[d] = static_cast<long long>(fl);
  }
  double acc = 0.0;
#pragma unroll
  for (int tap = 0; tap < (1 << DIM); ++tap) {
    long long idx = 0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const int bit = (tap >> (DIM - 1 - d)) & 1;
      const int len = shape[3 - DIM + d];
      long long i = base[d] + bit;
      if (i > len - 1) i = len > 1 ? len - 2 : 0;
      idx += i * step[d];
    }
    double coeff = static_cast<double>(a[idx]);
#pragma unroll
    for (int d = 0; d < DIM; ++d) coeff = coeff * w[d][(tap >> (DIM - 1 - d)) & 1];
    acc = acc + coeff;
  }
  return acc;
}

// B-spline tap weights of NI's get_spline_interpolation_weights at offset x from
// the base sample, in tap order, statement for statement.
template <int ORDER>
__device__ __forceinline__ void spline_weights(double x, double* w);
template <>
__device__ __forceinline__ void spline_weights<2>(double x, double* w) {
  w[1] = 0.75 - x * x;
  const double y = 0.5 - x;
  w[0] = 0.5 * y * y;
  w[2] = 1.0 - w[0] - w[1];
}
template <>
__device__ __forceinline__ void spline_weights<3>(double x, double* w) {
  const double y = x, z = 1.0 - x;
  w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[0] = z * z * z / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
}
template <>
__device__ __forceinline__ void spline_weights<4>(double x, double* w) {
  const double t = x * x;
  w[2] = t * (t * 0.25 - 0.625) + 115.0 / 192.0;
  double y = 1.0 + x;
  w[1] = y * (y * (y * (5.0 - y) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
  const double z = 1.0 - x;
  w[3] = z * (z * (z * (5.0 - z) / 6.0 - 1.25) + 5.0 / 24.0) + 55.0 / 96.0;
  y = 0.5 - x;
  y = y * y;
  w[0] = y * y / 24.0;
  w[4] = 1.0 - w[0] - w[1] - w[2] - w[3];
}
template <>
__device__ __forceinline__ void spline_weights<5>(double x, double* w) {
  const double y = x, z = 1.0 - x;
  double t = y * y;
  w[2] = t * (t * (0.25 - y / 12.0) - 0.5) + 0.55;
  t = z * z;
  w[3] = t * (t * (0.25 - z / 12.0) - 0.5) + 0.55;
  const double y1 = y + 1.0;
  w[1] = y1 * (y1 * (y1 * (y1 * (y1 / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
  const double z1 = z + 1.0;
  w[4] = z1 * (z1 * (z1 * (z1 * (z1 / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
  t = 1.0 - x;
  const double t2 = t * t;
  w[0] = t * t2 * t2 / 120.0;
  w[5] = 1.0 - w[0] - w[1] - w[2] - w[3] - w[4];
}

// scipy NI_GeometricTransform, order 2 .. 5, mode "constant", cval 0, on the
// float64 B-spline coefficients `a` of the image (sfm_spline_prefilter): outside
// [0, len - 1] on any axis, NaN included -> 0; base sample floor(c) for odd
// orders, floor(c + 0.5) for even ones; ORDER + 1 taps per axis from
// base - ORDER / 2, indices outside the array mirrored without repeating the edge
// sample; coefficient x weights in axis order, taps added in row-major order.
template <int DIM, int ORDER, typename A>
__device__ __forceinline__ double spline_sample(const A a, const int* shape, const double* c,
                                                const long long* pitch = nullptr) {
  constexpr int K = ORDER + 1;
  double w[DIM][K];
  long long off[DIM][K];
  long long dense = 1;
  long long step[DIM];
#pragma unroll
  for (int d = DIM - 1; d >= 0; --d) {
    step[d] = pitch ? pitch[3 - DIM + d] : dense;
    dense *= shape[3 - DIM + d];
  }
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const int len = shape[3 - DIM + d];
    if (!(c[d] >= 0.0 && c[d] <= static_cast<double>(len - 1))) return 0.0;
    const double base = (ORDER & 1) ? floor(c[d]) : floor(c[d] + 0.5);
    spline_weights<ORDER>(c[d] - base, w[d]);
    const long long start = static_cast<long long>(base) - ORDER / 2;
    const long long period = 2LL * len - 2;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      long long i = start + k;
      if (len == 1) {
        i = 0;
      } else {
        i = i < 0 ? -i : i;
        i = i % period;
        i = i >= len ? period - i : i;
      }
      off[d][k] = i * step[d];
    }
  }
  double acc = 0.0;
  if constexpr (DIM == 2) {
#pragma unroll
    for (int k0 = 0; k0 < K; ++k0) {
#pragma unroll
      for (int k1 = 0; k1 < K; ++k1) {
        double coeff = static_cast<double>(a[off[0][k0] + off[1][k1]]);
        coeff = coeff * w[0][k0];
        coeff = coeff * w[1][k1];
        acc = acc + coeff;
      }
    }
  } else {
    static_assert(DIM == 3, "spline_sample: 2-D and 3-D");
#pragma unroll
    for (int k0 = 0; k0 < K; ++k0) {
#pragma unroll
      for (int k1 = 0; k1 < K; ++k1) {
#pragma unroll
        for (int k2 = 0; k2 < K; ++k2) {
          double coeff = static_cast<double>(a[off[0][k0] + off[1][k1] + off[2][k2]]);
          coeff = coeff * w[0][k0];
          coeff = coeff * w[1][k1];
          coeff = coeff * w[2][k2];
          acc = acc + coeff;
        }
      }
    }
  }
  return acc;
}

template <int DIM, typename A>
__device__ __forceinline__ double nearest_sample(const A a, const int* shape, const double* c,
                                                 const long long* pitch = nullptr) {
  long long idx = 0, dense = 1;
#pragma unroll
  for (int d = DIM - 1; d >= 0; --d) {
    const int len = shape[3 - DIM + d];
    if (!(c[d] >= 0.0 && c[d] <= static_cast<double>(len - 1))) return 0.0;
    long long i = static_cast<long long>(floor(c[d] + 0.5));
    i = i > len - 1 ? len - 1 : i;
    idx += i * (pitch ? pitch[3 - DIM + d] : dense);
    dense *= len;
  }
  return static_cast<double>(a[idx]);
}

// double -> output type like NI's CASE_INTERP_OUT_*: unsigned types add 0.5 to
// positive values, clip and truncate; floats are narrowed.
template <typename T>
__device__ __forceinline__ T nd_convert(double v, double vmax) {
  v = v > 0.0 ? v + 0.5 : 0.0;
  v = v > vmax ? vmax : v;
  return static_cast<T>(v);
}
template <>
__device__ __forceinline__ float nd_convert<float>(double v, double) {
  return static_cast<float>(v);
}

// One channel of a float64 coordinate map plus a scalar, added on every read:
// element + shift, one rounding.
struct ShiftedMap {
  const double* m;
  double shift;
  __device__ __forceinline__ double operator[](long long i) const { return m[i] + shift; }
};

}  // namespace sfm

#endif  // SFM_NDSAMPLE_H_
