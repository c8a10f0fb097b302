// scipy.ndimage.map_coordinates on the device, orders 0 to 5: the samplers shared
// by the kernels of sfm_ndwarp_kernel.h.  Orders 0 and 1 read the image, orders 2 to 5
// its float64 B-spline coefficients (sfm_spline.hip).  Double arithmetic in SciPy's
// operation order; the units that include this are built with -ffp-contract=off.
//
// Every sampler has two instantiations.  MODES = false is mode "constant" with
// cval 0 and nothing else (ndimage_warp_kernel, render_tiles_kernel).  MODES =
// true takes a Boundary, SciPy's boundary mode and fill value, at run time (the
// mode is uniform over a launch): fold_coordinate and fold_tap below, restated
// from SciPy's behaviour in tests/ndwarp_modes_ref.py.
//
// `a` is anything indexable by a linear element offset whose elements widen to
// double: a pointer, or a view such as ShiftedMap below; linear_sample also takes
// a view whose value depends on the tap's node indices (RelativeMap).  `shape` holds 3
// entries (z, y, x; the last DIM are used) and is what coordinates are tested
// against.  `pitch`, when given, holds the element distance per axis in the same
// layout: a region of a larger array is then sampled in place (the region's
// origin is folded into `a`), and a 2-D array is read as a stack of identical
// planes with pitch 0.  Without it the array is dense in `shape`.
#ifndef SFM_NDSAMPLE_H_
#define SFM_NDSAMPLE_H_

#include <hip/hip_runtime.h>

namespace sfm {

// SciPy's boundary modes (SFM_MODE_* of the public header) and the fill value.
enum : int {
  kModeConstant = 0, kModeGridConstant = 1, kModeNearest = 2, kModeMirror = 3,
  kModeReflect = 4, kModeWrap = 5, kModeGridWrap = 6, kModeCount = 7
};
struct Boundary {
  int mode = kModeConstant;
  double cval = 0.0;
  // Orders 2 .. 5 under "nearest" and "grid-constant": the coefficients are those of
  // the image padded by `pad` samples per axis (sfm_spline_prefilter_mode), and the
  // kernels add it to the image-step coordinate; 0 everywhere else.
  int pad = 0;
};

// The coordinate `c` on an axis of length `len`, folded by the mode.  false: the
// sample is cval as a whole -- "constant" outside [0, len - 1] (NaN included), and
// under every other mode a NaN or a magnitude of 2^31 and above, which SciPy casts
// to an integer (undefined).  "grid-constant" and "nearest" leave the coordinate
// where it is and treat the taps; the others fold it with SciPy's periods: 2 len - 2
// "mirror", 2 len "reflect" (a coordinate within 1e-15 below 0 lands on 1e-15 - 1),
// len - 1 "wrap", len "grid-wrap"; SciPy's (npy_intp) casts are trunc().
__device__ __forceinline__ bool fold_coordinate(int mode, int len, double& c) {
  if (mode == kModeConstant) return c >= 0.0 && c <= static_cast<double>(len - 1);
  if (!(fabs(c) < 2147483648.0)) return false;
  if (mode == kModeGridConstant || mode == kModeNearest) return true;
  const bool lo = c < 0.0;
  if (!lo && !(c > static_cast<double>(len - 1))) return true;
  if (len <= 1) {
    c = 0.0;
    return true;
  }
  const double n = static_cast<double>(len);
  switch (mode) {
    case kModeMirror: {
      const double sz2 = 2.0 * n - 2.0;
      if (lo) {
        const double v = sz2 * trunc(-c / sz2) + c;
        c = v <= 1.0 - n ? v + sz2 : -v;
      } else {
        const double v = c - sz2 * trunc(c / sz2);
        c = v >= n ? sz2 - v : v;
      }
      break;
    }
    case kModeReflect: {
      const double sz2 = 2.0 * n;
      if (lo) {
        double v = c;
        if (v < -sz2) v = sz2 * trunc(-v / sz2) + v;
        c = v < -n ? v + sz2 : (v > -1e-15 ? 1e-15 : -v) - 1.0;
      } else {
        const double v = c - sz2 * trunc(c / sz2);
        c = v >= n ? sz2 - v - 1.0 : v;
      }
      break;
    }
    case kModeWrap: {
      const double sz = n - 1.0;
      c = lo ? c + sz * (trunc(-c / sz) + 1.0) : c - sz * trunc(c / sz);
      break;
    }
    default: {  // kModeGridWrap
      if (lo) {
        c = c + n * (trunc((-1.0 - c) / n) + 1.0);
      } else {
        const double v = c - n * trunc((c + 1.0) / n);
        c = v < 0.0 ? v + n : v;
      }
      break;
    }
  }
  return true;
}

// The tap index `i` folded into [0, len - 1], for every i: "nearest" clamps,
// "reflect" repeats the edge sample, "grid-wrap" has period len; "constant",
// "mirror" and "wrap" mirror without repeating the edge sample ("wrap" folds only
// its coordinate with period len - 1).  Under "grid-constant" a tap outside the
// array is not read: `fill` is set and the tap's value is cval.
__device__ __forceinline__ long long fold_tap(int mode, int len, long long i, bool& fill) {
  fill = false;
  if (i >= 0 && i < len) return i;
  if (mode == kModeGridConstant) {
    fill = true;
    return 0;
  }
  if (len <= 1) return 0;
  switch (mode) {
    case kModeNearest:
      return i < 0 ? 0 : len - 1;
    case kModeReflect: {
      const long long p = 2LL * len;
      long long j = i % p;
      j = j < 0 ? j + p : j;
      return j >= len ? p - 1 - j : j;
    }
    case kModeGridWrap: {
      const long long j = i % len;
      return j < 0 ? j + len : j;
    }
    default: {
      const long long p = 2LL * len - 2;
      long long j = i < 0 ? -i : i;
      j = j % p;
      return j >= len ? p - j : j;
    }
  }
}

// The element of `a` at linear offset `idx`, widened to double.  `node` holds the
// folded tap index per axis (DIM entries), which linear_sample has at hand: an
// accessor whose value depends on the tap's position (RelativeMap below) declares
// at(idx, node) and gets it without recovering it from `idx`; everything else is
// read as a[idx] and the indices fall away unused.
template <typename A>
__device__ __forceinline__ auto tap_value(const A& a, long long idx, const long long* node)
    -> decltype(a.at(idx, node)) {
  return a.at(idx, node);
}
template <typename A>
__device__ __forceinline__ auto tap_value(const A& a, long long idx, const long long*)
    -> decltype(static_cast<double>(a[idx])) {
  return static_cast<double>(a[idx]);
}

// scipy NI_GeometricTransform, order 1, mode "constant", cval 0: outside
// [0, len - 1] on any axis, NaN included -> 0; the tap beyond the last sample
// (coordinate exactly len - 1) carries weight 0 and is read mirrored, from
// len - 2, as SciPy's edge mapping does: 0 x inf and 0 x NaN there are NaN.
//
// MODES: the coordinate is folded first, every tap is folded after it, a tap that
// "grid-constant" finds outside the array is cval.
template <int DIM, bool MODES = false, typename A>
__device__ __forceinline__ double linear_sample(const A a, const int* shape, const double* c,
                                                const long long* pitch = nullptr,
                                                const Boundary b = Boundary()) {
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
    double cc = c[d];
    if constexpr (MODES) {
      if (!fold_coordinate(b.mode, len, cc)) return b.cval;
    } else {
      if (!(c[d] >= 0.0 && c[d] <= static_cast<double>(len - 1))) return 0.0;
    }
    const double fl = floor(cc);
    const double t = cc - fl;
    w[d][0] = 1.0 - t;
    w[d][1] = 1.0 - w[d][0];
    base[d] = static_cast<long long>(fl);
  }
  double acc = 0.0;
#pragma unroll
  for (int tap = 0; tap < (1 << DIM); ++tap) {
    long long idx = 0;
    long long node[DIM];
    bool fill = false;
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      const int bit = (tap >> (DIM - 1 - d)) & 1;
      const int len = shape[3 - DIM + d];
      long long i = base[d] + bit;
      if constexpr (MODES) {
        bool f;
        i = fold_tap(b.mode, len, i, f);
        fill = fill || f;
      } else {
        if (i > len - 1) i = len > 1 ? len - 2 : 0;
      }
      node[d] = i;
      idx += i * step[d];
    }
    double coeff = fill ? b.cval : tap_value(a, idx, node);
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
//
// MODES: "constant" with a fill value, "mirror" and "wrap", the modes whose
// coefficients are these; only the coordinate is folded, the taps mirror as above.
//
// TAPS (with MODES): the other modes.  Every tap is folded by fold_tap, as in
// linear_sample: "nearest" clamps, "reflect" and "grid-wrap" fold with their
// periods, and a tap that "grid-constant" finds outside the array is cval (its
// offset is kept as -1: offsets inside the array are never negative).  The
// coefficients are those of the mode's own prefilter, for "nearest" and
// "grid-constant" of the padded image (sfm_spline_prefilter_mode): `shape` is then
// the padded shape and `c` is shifted.  An instantiation of its own, so that the
// three modes above keep their registers.
template <int DIM, int ORDER, bool MODES = false, bool TAPS = false, typename A>
__device__ __forceinline__ double spline_sample(const A a, const int* shape, const double* c,
                                                const long long* pitch = nullptr,
                                                const Boundary b = Boundary()) {
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
    double cc = c[d];
    if constexpr (MODES) {
      if (!fold_coordinate(b.mode, len, cc)) return b.cval;
    } else {
      if (!(c[d] >= 0.0 && c[d] <= static_cast<double>(len - 1))) return 0.0;
    }
    const double base = (ORDER & 1) ? floor(cc) : floor(cc + 0.5);
    spline_weights<ORDER>(cc - base, w[d]);
    const long long start = static_cast<long long>(base) - ORDER / 2;
    const long long period = 2LL * len - 2;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      long long i = start + k;
      if constexpr (TAPS) {
        bool fill;
        i = fold_tap(b.mode, len, i, fill);
        off[d][k] = fill ? -1 : i * step[d];
        continue;
      }
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
        double coeff;
        if constexpr (TAPS)
          coeff = (off[0][k0] | off[1][k1]) < 0 ? b.cval
                                                : static_cast<double>(a[off[0][k0] + off[1][k1]]);
        else
          coeff = static_cast<double>(a[off[0][k0] + off[1][k1]]);
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
          double coeff;
          if constexpr (TAPS)
            coeff = (off[0][k0] | off[1][k1] | off[2][k2]) < 0
                        ? b.cval
                        : static_cast<double>(a[off[0][k0] + off[1][k1] + off[2][k2]]);
          else
            coeff = static_cast<double>(a[off[0][k0] + off[1][k1] + off[2][k2]]);
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

template <int DIM, bool MODES = false, typename A>
__device__ __forceinline__ double nearest_sample(const A a, const int* shape, const double* c,
                                                 const long long* pitch = nullptr,
                                                 const Boundary b = Boundary()) {
  long long idx = 0, dense = 1;
  bool fill = false;
#pragma unroll
  for (int d = DIM - 1; d >= 0; --d) {
    const int len = shape[3 - DIM + d];
    double cc = c[d];
    if constexpr (MODES) {
      if (!fold_coordinate(b.mode, len, cc)) return b.cval;
    } else {
      if (!(c[d] >= 0.0 && c[d] <= static_cast<double>(len - 1))) return 0.0;
    }
    long long i = static_cast<long long>(floor(cc + 0.5));
    if constexpr (MODES) {
      bool f;
      i = fold_tap(b.mode, len, i, f);
      fill = fill || f;
    } else {
      i = i > len - 1 ? len - 1 : i;
    }
    idx += i * (pitch ? pitch[3 - DIM + d] : dense);
    dense *= len;
  }
  return fill ? b.cval : static_cast<double>(a[idx]);
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

// One channel of a RELATIVE coordinate map of type M (float or double), read as the
// absolute source coordinate the reference's NumPy statements form from it
// (warp.py:249-262): to_absolute adds node x stride in place -- computed in
// double, stored as M --, the box shift is a second in-place add, stored as M
// again, and the out_scale product is float64:
//   v = (double)(M)(rel + (double)node[axis] * stride)
//   v = (double)(M)(v + shift)        only with a map_box (-0.0 + 0.0 is +0.0)
//   v = v * scale
// node x stride is one rounded product (no contraction with the add).  `axis` is
// the channel's own axis among the DIM entries of `node`.
template <typename M, int DIM>
struct RelativeMap {
  const M* m;
  int axis;
  bool has_shift;
  double stride, shift, scale;
  __device__ __forceinline__ double at(long long i, const long long* node) const {
    long long n = node[0];   // a select per axis, not an indexed read of registers
#pragma unroll
    for (int k = 1; k < DIM; ++k) n = axis == k ? node[k] : n;
    const double off = static_cast<double>(n) * stride;
    double v = static_cast<double>(static_cast<M>(static_cast<double>(m[i]) + off));
    if (has_shift) v = static_cast<double>(static_cast<M>(v + shift));
    return v * scale;
  }
};

}  // namespace sfm

#endif  // SFM_NDSAMPLE_H_
