// B-spline prefilter on the device: scipy.ndimage.spline_filter(image, order,
// output=float64, mode="constant") for orders 2 .. 5, the coefficients that
// spline_sample (sfm_ndsample.h) reads.
//
//   sfm_spline_prefilter  <->  ni_splines.c: apply_filter with mirror boundaries,
//                              per axis through NI_SplineFilter1D
//
// Written from tests/ndwarp_spline_ref.py, which is pinned to SciPy element for
// element.  Per line c[0 .. n-1] of an axis, in plain double and in this order
// (built with -ffp-contract=off):
//
//   c[i] *= gain                                   gain = prod (1 - z)(1 - 1/z)
//   per pole z:  zn = pow(z, n-1)  (the caller's libm value, SfmSplineItem.zn)
//     c[0] = c[0] + zn c[n-1];  c[0] += z^i (c[i] + zn c[n-1-i]), i = 1 .. n-2
//     c[0] /= 1 - zn zn
//     c[i] += z c[i-1], i = 1 .. n-1
//     c[n-1] = (z c[n-2] + c[n-1]) z / (z z - 1)
//     c[i] = z (c[i+1] - c[i]), i = n-2 .. 0
//
// The recursion of a line is sequential and splitting it would change the
// rounding, so the parallelism is over lines: one thread per line.  For the z
// and y passes neighbouring threads take neighbouring x, so the 8-byte accesses
// of a wave are one contiguous run (spline_lines_kernel).  For the x pass a
// thread per line would stride by the row length; there a workgroup of one wave
// owns kRows rows and walks them in chunks of kChunk columns staged through LDS,
// loaded and stored with the lanes along x, forward for the initialisation and
// the causal pass, backward for the anticausal one, each row's state in a
// register of its thread (spline_rows_kernel).  The initialisation sweep always
// runs the whole line: its terms are exactly zero only once z^i has underflowed,
// and not even then for float images (0 x NaN, 0 x inf).
//
// The pass of an item's first axis longer than 1 reads the image (any of the
// three types, through `pitch`, so a region of a larger array is filtered where
// it lies) and fuses the conversion and the gain; later passes run in place on
// the coefficients.  An axis of length 1 is skipped, as in SciPy.
//
// sfm_spline_prefilter_mode: SciPy's other two initialisations, and the padding
// that map_coordinates puts in front of the filter (tests/spline_modes_ref.py,
// pinned to SciPy the same way).  Both kernels take the initialisation as a
// template parameter; the mirror statements above are instantiation kInitMirror
// and are unchanged.  Per pole z, between the gain and the anticausal recursion:
//
//   reflect ("reflect", "nearest"):  zn = pow(z, n)  (the caller's libm value)
//     f = c[0];  c[0] = c[0] + zn c[n-1]
//     c[0] += z^i (c[i] + zn c[n-1-i]), i = 1 .. n-1   (i = n-1 pairs c[n-1] with
//                                                       the running c[0] itself)
//     c[0] *= z / (1 - zn zn);  c[0] += f
//     causal as above;  c[n-1] *= z / (z - 1)
//   wrap ("grid-wrap"):  no pow, zi = z^i by repeated multiplication
//     c[0] += z^i c[n-i], i = 1 .. n-1;  c[0] /= 1 - z^n
//     causal as above
//     c[n-1] += z^(i+1) c[i], i = 0 .. n-2, on the causally filtered line: one more
//     forward sweep, which cannot be folded into the causal pass without changing
//     the rounding;  c[n-1] *= z / (z^n - 1)
//
// PAD: "nearest" and "grid-constant" filter the image padded by kSplinePad samples
// on every axis the array has (the absent leading axis of a 2-D image is not
// padded; a real axis of length 1 is, and is filtered).  The coefficients of an
// item are dense in shape + 2 kSplinePad; the converting pass, that of the first
// real axis, reads the source through a clamped index or takes the pad value
// where the padded index lies outside it, so no padded image exists; later passes
// run in place on the padded coefficients.
#include "sfm_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

constexpr int kLineBlock = 256;
constexpr int kRows = 64;     // rows of a workgroup of the x pass = its threads
constexpr int kChunk = 32;    // columns staged at a time
constexpr int kPad = 1;       // tile rows are kChunk + 1 doubles: a thread walking its
                              // row and the lanes of a load both spread over the banks

struct SplineArgs {
  const SfmSplineItem* items;
  double* coeffs;
  int axis, npoles;
  double pole[2];
  double gain;
  // sfm_spline_prefilter_mode, read by the PAD instantiations alone
  int ndim, fill;        // real axes; 1: outside the source the pad value, 0: the edge sample
  double pad_value;
};

constexpr int kInitMirror = 0, kInitReflect = 1, kInitWrap = 2;
constexpr int kSplinePad = 12;   // SciPy's npad (_prepad_for_spline_filter)

// shape of an item's coefficients
template <bool PAD>
__device__ __forceinline__ void coeff_shape(const SfmSplineItem& it, int ndim, int* p) {
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = it.shape[k] + (PAD && k >= 3 - ndim ? 2 * kSplinePad : 0);
}

// the axis whose pass converts the image: the first one longer than 1 (the last
// axis when there is none: a single voxel is only converted)
__host__ __device__ inline int convert_axis(const int32_t* shape) {
  return shape[0] > 1 ? 0 : (shape[1] > 1 ? 1 : 2);
}

// axis 0 or 1: one thread per line, lanes along x
template <typename S, int INIT = kInitMirror, bool PAD = false>
__global__ void __launch_bounds__(kLineBlock) spline_lines_kernel(SplineArgs a) {
  const SfmSplineItem& it = a.items[blockIdx.y];
  const int ax = a.axis;
  int shape[3];
  coeff_shape<PAD>(it, a.ndim, shape);
  const int n = shape[ax];
  if (n == 1) return;
  const long long ny = shape[1], nx = shape[2];
  const long long lines = (ax == 0 ? ny : (long long)shape[0]) * nx;
  const long long t = blockIdx.x * (long long)kLineBlock + threadIdx.x;
  if (t >= lines) return;
  const long long outer = t / nx, x = t % nx;
  long long dbase, dstep, sbase, sstep;
  // PAD: the line's two fixed source indices, clamped into the source; `beyond`: one
  // of them lay outside it; ns, spad: source length and pad of the line's own axis
  bool beyond = false;
  int ns = n, spad = 0;
  if constexpr (PAD) {
    const int oax = ax == 0 ? 1 : 0;
    const int opad = oax >= 3 - a.ndim ? kSplinePad : 0;     // (x is always a real axis)
    long long so = outer - opad, sx = x - kSplinePad;
    beyond = so < 0 || so >= it.shape[oax] || sx < 0 || sx >= it.shape[2];
    so = min(max(so, 0LL), (long long)it.shape[oax] - 1);
    sx = min(max(sx, 0LL), (long long)it.shape[2] - 1);
    sbase = so * it.pitch[oax] + sx * it.pitch[2];
    sstep = it.pitch[ax];
    ns = it.shape[ax];
    spad = kSplinePad;                     // the converting axis is a real one
    if (ax == 0) dbase = t, dstep = ny * nx;
    else dbase = outer * ny * nx + x, dstep = nx;
  } else if (ax == 0) {
    dbase = t, dstep = ny * nx;
    sbase = outer * it.pitch[1] + x * it.pitch[2], sstep = it.pitch[0];
  } else {
    dbase = outer * ny * nx + x, dstep = nx;
    sbase = outer * it.pitch[0] + x * it.pitch[2], sstep = it.pitch[1];
  }
  double* c = a.coeffs + it.coeff_offset + dbase;
  const S* src = static_cast<const S*>(it.image) + sbase;
  const bool from_image = convert_axis(shape) == ax;
  for (int p = 0; p < a.npoles; ++p) {
    const double z = a.pole[p], zn = it.zn[ax][p];
    const bool img = from_image && p == 0;
    const double scale = p == 0 ? a.gain : 1.0;
    auto in = [&](long long i) -> double {
      if constexpr (PAD) {
        if (img) {
          long long j = i - spad;
          const bool out = beyond || j < 0 || j >= ns;
          j = min(max(j, 0LL), (long long)ns - 1);
          return (a.fill && out ? a.pad_value : static_cast<double>(src[j * sstep])) * scale;
        }
        return c[i * dstep] * scale;
      } else {
        return (img ? static_cast<double>(src[i * sstep]) : c[i * dstep]) * scale;
      }
    };
    double c0;
    if constexpr (INIT == kInitMirror) {
      c0 = in(0) + zn * in(n - 1);
      double zi = z;
      for (int i = 1; i < n - 1; ++i) {
        c0 += zi * (in(i) + zn * in(n - 1 - i));
        zi *= z;
      }
      c0 /= 1.0 - zn * zn;
    } else if constexpr (INIT == kInitReflect) {
      const double first = in(0);
      c0 = first + zn * in(n - 1);
      double zi = z;
      for (int i = 1; i < n; ++i) {
        const double partner = i == n - 1 ? c0 : in(n - 1 - i);
        c0 += zi * (in(i) + zn * partner);
        zi *= z;
      }
      c0 *= z / (1.0 - zn * zn);
      c0 += first;
    } else {
      c0 = in(0);
      double zi = z;
      for (int i = 1; i < n; ++i) {
        c0 += zi * in(n - i);
        zi *= z;
      }
      c0 /= 1.0 - zi;
    }
    double prev = c0, prev2 = c0;
    c[0] = c0;
    for (int i = 1; i < n; ++i) {
      const double v = in(i) + z * prev;
      c[i * dstep] = v;
      prev2 = prev;
      prev = v;
    }
    double next;
    if constexpr (INIT == kInitMirror) {
      next = (z * prev2 + prev) * z / (z * z - 1.0);
    } else if constexpr (INIT == kInitReflect) {
      next = prev * (z / (z - 1.0));
    } else {
      double zi = z;
      next = prev;
      for (int i = 0; i < n - 1; ++i) {
        next += zi * c[i * dstep];
        zi *= z;
      }
      next *= z / (zi - 1.0);
    }
    c[(n - 1) * dstep] = next;
    for (int i = n - 2; i >= 0; --i) {
      next = z * (next - c[i * dstep]);
      c[i * dstep] = next;
    }
  }
}

// axis 2: kRows rows per workgroup, kChunk columns at a time through LDS
// (PAD: x is never the converting axis, the pass only runs over the padded shape)
template <typename S, int INIT = kInitMirror, bool PAD = false>
__global__ void __launch_bounds__(kRows) spline_rows_kernel(SplineArgs a) {
  __shared__ double fwd[kRows][kChunk + kPad];
  __shared__ double bwd[kRows][kChunk + kPad];
  const SfmSplineItem& it = a.items[blockIdx.y];
  int shape[3];
  coeff_shape<PAD>(it, a.ndim, shape);
  const int n = shape[2];
  const bool from_image = convert_axis(shape) == 2;
  if (n == 1 && !from_image) return;
  const long long ny = shape[1];
  const long long rows = (long long)shape[0] * ny;
  const long long r0 = blockIdx.x * (long long)kRows;
  if (r0 >= rows) return;                       // (the whole workgroup)
  const int tid = threadIdx.x;
  const bool live = r0 + tid < rows;
  double* cbase = a.coeffs + it.coeff_offset;
  const S* image = static_cast<const S*>(it.image);
  if (n == 1) {                                 // one voxel: rows == 1
    if (tid == 0) cbase[0] = static_cast<double>(image[0]);
    return;
  }

  // columns [col0, col0 + kChunk) of the workgroup's rows -> tile, lanes along x
  auto load = [&](double (*tile)[kChunk + kPad], long long col0, bool img, double scale) {
    const int col = tid % kChunk;
    const long long cc = col0 + col;
    for (int rr = tid / kChunk; rr < kRows; rr += kRows / kChunk) {
      const long long row = r0 + rr;
      if (row < rows && cc >= 0 && cc < n) {
        const double v = img ? static_cast<double>(image[(row / ny) * it.pitch[0] +
                                                          (row % ny) * it.pitch[1] +
                                                          cc * it.pitch[2]])
                             : cbase[row * n + cc];
        tile[rr][col] = v * scale;
      }
    }
  };
  auto store = [&](double (*tile)[kChunk + kPad], long long col0) {
    const int col = tid % kChunk;
    const long long cc = col0 + col;
    for (int rr = tid / kChunk; rr < kRows; rr += kRows / kChunk) {
      const long long row = r0 + rr;
      if (row < rows && cc < n) cbase[row * n + cc] = tile[rr][col];
    }
  };

  for (int p = 0; p < a.npoles; ++p) {
    const double z = a.pole[p], zn = it.zn[2][p];
    const bool img = from_image && p == 0;
    const double scale = p == 0 ? a.gain : 1.0;
    // initialisation: term i pairs c[i] with c[n-1-i], i = 0 .. n-2; the mirrored
    // partner of the chunk [i0, i0 + kChunk) is the chunk that starts at m0
    double c0 = 0.0, zi = z;
    if constexpr (INIT == kInitMirror) {
      for (long long i0 = 0; i0 <= n - 2; i0 += kChunk) {
        const long long m0 = n - 1 - i0 - (kChunk - 1);
        load(fwd, i0, img, scale);
        load(bwd, m0, img, scale);
        __syncthreads();
        if (live) {
          const long long i1 = min(i0 + kChunk - 1, (long long)n - 2);
          for (long long i = i0; i <= i1; ++i) {
            const double ci = fwd[tid][i - i0], cm = bwd[tid][n - 1 - i - m0];
            if (i == 0) {
              c0 = ci + zn * cm;
            } else {
              c0 += zi * (ci + zn * cm);
              zi *= z;
            }
          }
        }
        __syncthreads();
      }
      c0 /= 1.0 - zn * zn;
    } else if constexpr (INIT == kInitReflect) {
      // the same walk one term further: i = n-1 pairs c[n-1] with the running c[0]
      double first = 0.0;
      for (long long i0 = 0; i0 <= n - 1; i0 += kChunk) {
        const long long m0 = n - 1 - i0 - (kChunk - 1);
        load(fwd, i0, img, scale);
        load(bwd, m0, img, scale);
        __syncthreads();
        if (live) {
          const long long i1 = min(i0 + kChunk - 1, (long long)n - 1);
          for (long long i = i0; i <= i1; ++i) {
            const double ci = fwd[tid][i - i0], cm = bwd[tid][n - 1 - i - m0];
            if (i == 0) {
              first = ci;
              c0 = ci + zn * cm;
            } else {
              c0 += zi * (ci + zn * (i == n - 1 ? c0 : cm));
              zi *= z;
            }
          }
        }
        __syncthreads();
      }
      c0 *= z / (1.0 - zn * zn);
      c0 += first;
    } else {
      // wrap: c[0], then c[n-1] down to c[1]: a backward-only walk
      load(fwd, 0, img, scale);
      __syncthreads();
      if (live) c0 = fwd[tid][0];
      __syncthreads();
      for (long long i0 = (long long)(n - 1) / kChunk * kChunk; i0 >= 0; i0 -= kChunk) {
        load(fwd, i0, img, scale);
        __syncthreads();
        if (live) {
          const long long i1 = min(i0 + kChunk - 1, (long long)n - 1);
          for (long long j = i1; j >= max(i0, 1LL); --j) {
            c0 += zi * fwd[tid][j - i0];
            zi *= z;
          }
        }
        __syncthreads();
      }
      c0 /= 1.0 - zi;
    }
    // causal
    double prev = c0, prev2 = c0;
    for (long long i0 = 0; i0 < n; i0 += kChunk) {
      load(fwd, i0, img, scale);
      __syncthreads();
      if (live) {
        const long long i1 = min(i0 + kChunk - 1, (long long)n - 1);
        for (long long i = i0; i <= i1; ++i) {
          const double v = i == 0 ? c0 : fwd[tid][i - i0] + z * prev;
          fwd[tid][i - i0] = v;
          prev2 = prev;
          prev = v;
        }
      }
      __syncthreads();
      store(fwd, i0);
      __syncthreads();
    }
    // anticausal, from the last chunk back
    double next;
    if constexpr (INIT == kInitMirror) {
      next = (z * prev2 + prev) * z / (z * z - 1.0);
    } else if constexpr (INIT == kInitReflect) {
      next = prev * (z / (z - 1.0));
    } else {
      // wrap: one more forward sweep, over the causally filtered c[0 .. n-2]
      next = prev;
      zi = z;
      for (long long i0 = 0; i0 <= n - 2; i0 += kChunk) {
        load(fwd, i0, false, 1.0);
        __syncthreads();
        if (live) {
          const long long i1 = min(i0 + kChunk - 1, (long long)n - 2);
          for (long long i = i0; i <= i1; ++i) {
            next += zi * fwd[tid][i - i0];
            zi *= z;
          }
        }
        __syncthreads();
      }
      next *= z / (zi - 1.0);
    }
    for (long long i0 = (long long)(n - 1) / kChunk * kChunk; i0 >= 0; i0 -= kChunk) {
      load(fwd, i0, false, 1.0);
      __syncthreads();
      if (live) {
        const long long i1 = min(i0 + kChunk - 1, (long long)n - 1);
        for (long long i = i1; i >= i0; --i) {
          if (i != n - 1) next = z * (next - fwd[tid][i - i0]);
          fwd[tid][i - i0] = next;
        }
      }
      __syncthreads();
      store(fwd, i0);
      __syncthreads();
    }
  }
}

// SciPy's literals (ni_splines.c: get_filter_poles)
const double kPoles[4][2] = {
    {-0.171572875253809902396622551580603843, 0.0},
    {-0.267949192431122706472553658494127633, 0.0},
    {-0.361341225900220177092212841325675255, -0.013725429297339121360331226939128204},
    {-0.430575347099973791851434783493520110, -0.043096288203264653822712376822550182},
};

// How sfm_spline_prefilter_mode filters: the initialisation, and for the padded
// modes the real dimensionality and what lies outside the source.
struct SplineVariant {
  int init = kInitMirror;
  bool pad = false;
  int ndim = 3, fill = 0;
  double pad_value = 0.0;
};

// the checks and the launches of sfm_spline_prefilter (the default variant) and
// sfm_spline_prefilter_mode
int prefilter_launch(const SfmSplinePrefilterDesc* d, const SplineVariant& v) {
  if (d->order < 2 || d->order > 5)
    return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: order %d (2 .. 5)", d->order);
  if (d->dtype != SFM_DTYPE_U8 && d->dtype != SFM_DTYPE_U16 && d->dtype != SFM_DTYPE_F32)
    return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: dtype %d", d->dtype);
  if (d->n_items < 0 || d->n_items > 65535)
    return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: n_items %d (0 .. 65535)", d->n_items);
  if (d->n_items == 0) return SFM_OK;
  if (!d->items_host || !d->items || !d->coeffs)
    return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: NULL table or coefficients");
  long long max_lines[3] = {0, 0, 0};
  for (int t = 0; t < d->n_items; ++t) {
    const SfmSplineItem& it = d->items_host[t];
    if (!it.image) return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: item %d: NULL image", t);
    long long size = 1;
    int32_t shape[3];      // of the coefficients
    for (int k = 0; k < 3; ++k) {
      if (it.shape[k] < 1 || (v.pad && it.shape[k] > 0x7fffffff - 2 * kSplinePad))
        return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: item %d: bad shape", t);
      shape[k] = it.shape[k] + (v.pad && k >= 3 - v.ndim ? 2 * kSplinePad : 0);
      size *= shape[k];
    }
    if (v.pad && v.ndim == 2 && it.shape[0] != 1)
      return sfm::fail(SFM_ERR_INVALID,
                       "spline_prefilter: item %d: bad shape (2-d arrays have shape[0] = 1)", t);
    if (it.coeff_offset < 0 || size > d->coeffs_len || it.coeff_offset > d->coeffs_len - size)
      return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: item %d leaves the coefficients", t);
    const long long z = shape[0], y = shape[1], x = shape[2];
    if (z > 1) max_lines[0] = std::max(max_lines[0], y * x);
    if (y > 1) max_lines[1] = std::max(max_lines[1], z * x);
    if (x > 1 || convert_axis(shape) == 2) max_lines[2] = std::max(max_lines[2], z * y);
  }
  SplineArgs a;
  a.items = d->items;
  a.coeffs = d->coeffs;
  a.ndim = v.ndim;
  a.fill = v.fill;
  a.pad_value = v.pad_value;
  const double* poles = kPoles[d->order - 2];
  a.npoles = d->order >= 4 ? 2 : 1;
  a.gain = 1.0;
  for (int p = 0; p < 2; ++p) a.pole[p] = poles[p];
  for (int p = 0; p < a.npoles; ++p) a.gain *= (1.0 - poles[p]) * (1.0 - 1.0 / poles[p]);
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  for (int ax = 0; ax < 3; ++ax) {
    if (max_lines[ax] == 0) continue;
    const int per_block = ax == 2 ? kRows : kLineBlock;
    const long long gx = (max_lines[ax] + per_block - 1) / per_block;
    if (gx > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: too large");
    const dim3 g(static_cast<unsigned>(gx), static_cast<unsigned>(d->n_items)), b(per_block);
    a.axis = ax;
#define SFM_SPL_V(S, INIT, PAD)                                                    \
  do {                                                                             \
    if (ax == 2)                                                                   \
      hipLaunchKernelGGL((spline_rows_kernel<S, INIT, PAD>), g, b, 0, st, a);      \
    else                                                                           \
      hipLaunchKernelGGL((spline_lines_kernel<S, INIT, PAD>), g, b, 0, st, a);     \
  } while (0)
#define SFM_SPL(S)                                                                 \
  do {                                                                             \
    if (v.init == kInitWrap)                                                       \
      SFM_SPL_V(S, kInitWrap, false);                                              \
    else if (v.init == kInitReflect && v.pad)                                      \
      SFM_SPL_V(S, kInitReflect, true);                                            \
    else if (v.init == kInitReflect)                                               \
      SFM_SPL_V(S, kInitReflect, false);                                           \
    else if (v.pad)                                                                \
      SFM_SPL_V(S, kInitMirror, true);                                             \
    else                                                                           \
      SFM_SPL_V(S, kInitMirror, false);                                            \
  } while (0)
    switch (d->dtype) {
      case SFM_DTYPE_U8: SFM_SPL(unsigned char); break;
      case SFM_DTYPE_U16: SFM_SPL(unsigned short); break;
      default: SFM_SPL(float); break;
    }
#undef SFM_SPL
#undef SFM_SPL_V
    SFM_LAUNCH_CHECK();
  }
  return SFM_OK;
}

}  // namespace

extern "C" int sfm_spline_prefilter(const SfmSplinePrefilterDesc* d) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: NULL argument");
  return prefilter_launch(d, SplineVariant());
}

extern "C" int sfm_spline_mode_pad(int32_t mode) {
  if (mode < 0 || mode > SFM_MODE_GRID_WRAP)
    return sfm::fail(SFM_ERR_INVALID, "spline_mode_pad: boundary mode %d", mode);
  return mode == SFM_MODE_NEAREST || mode == SFM_MODE_GRID_CONSTANT ? kSplinePad : 0;
}

extern "C" int sfm_spline_prefilter_mode(const SfmSplinePrefilterDesc* d, int32_t mode,
                                         int32_t ndim, double pad_value) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "spline_prefilter_mode: NULL argument");
  if (mode < 0 || mode > SFM_MODE_GRID_WRAP)
    return sfm::fail(SFM_ERR_INVALID, "spline_prefilter_mode: boundary mode %d", mode);
  if (ndim != 2 && ndim != 3)
    return sfm::fail(SFM_ERR_INVALID, "spline_prefilter_mode: ndim %d", ndim);
  SplineVariant v;
  v.ndim = ndim;
  switch (mode) {
    case SFM_MODE_CONSTANT: case SFM_MODE_MIRROR: case SFM_MODE_WRAP:
      return prefilter_launch(d, v);
    case SFM_MODE_REFLECT: v.init = kInitReflect; break;
    case SFM_MODE_NEAREST: v.init = kInitReflect, v.pad = true; break;
    case SFM_MODE_GRID_WRAP: v.init = kInitWrap; break;
    default: v.pad = true, v.fill = 1, v.pad_value = pad_value; break;   // GRID_CONSTANT
  }
  if (!sfm::spline_modes_enabled())
    return sfm::fail(SFM_ERR_INVALID,
                     "spline_prefilter_mode: boundary mode %d at order %d (constant, mirror and "
                     "wrap are built; the others need the switch SFM_SPLINE_MODES=1)",
                     mode, d->order);
  if (v.fill && d->dtype != SFM_DTYPE_F32 && !std::isfinite(pad_value))
    return sfm::fail(SFM_ERR_INVALID,
                     "spline_prefilter_mode: non-finite pad value for an integer image");
  return prefilter_launch(d, v);
}

