// scipy.ndimage.map_coordinates on the device, orders 0 and 1, mode "constant",
// cval 0: the samplers shared by ndimage_warp_kernel and render_tiles_kernel
// (sfm_warp.hip).  Double arithmetic in SciPy's operation order; the units that
// include this are built with -ffp-contract=off.
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
