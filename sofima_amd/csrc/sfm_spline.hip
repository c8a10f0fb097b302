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
#include "sfm_common.h"

#include <algorithm>

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
};

// the axis whose pass converts the image: the first one longer than 1 (the last
// axis when there is none: a single voxel is only converted)
__host__ __device__ inline int convert_axis(const int32_t* shape) {
  return shape[0] > 1 ? 0 : (shape[1] > 1 ? 1 : 2);
}

// axis 0 or 1: one thread per line, lanes along x
template <typename S>
__global__ void __launch_bounds__(kLineBlock) spline_lines_kernel(SplineArgs a) {
  const SfmSplineItem& it = a.items[blockIdx.y];
  const int ax = a.axis;
  const int n = it.shape[ax];
  if (n == 1) return;
  const long long ny = it.shape[1], nx = it.shape[2];
  const long long lines = (ax == 0 ? ny : (long long)it.shape[0]) * nx;
  const long long t = blockIdx.x * (long long)kLineBlock + threadIdx.x;
  if (t >= lines) return;
  const long long outer = t / nx, x = t % nx;
  long long dbase, dstep, sbase, sstep;
  if (ax == 0) {
    dbase = t, dstep = ny * nx;
    sbase = outer * it.pitch[1] + x * it.pitch[2], sstep = it.pitch[0];
  } else {
    dbase = outer * ny * nx + x, dstep = nx;
    sbase = outer * it.pitch[0] + x * it.pitch[2], sstep = it.pitch[1];
  }
  double* c = a.coeffs + it.coeff_offset + dbase;
  const S* src = static_cast<const S*>(it.image) + sbase;
  const bool from_image = convert_axis(it.shape) == ax;
  for (int p = 0; p < a.npoles; ++p) {
    const double z = a.pole[p], zn = it.zn[ax][p];
    const bool img = from_image && p == 0;
    const double scale = p == 0 ? a.gain : 1.0;
    auto in = [&](long long i) -> double {
      return (img ? static_cast<double>(src[i * sstep]) : c[i * dstep]) * scale;
    };
    double c0 = in(0) + zn * in(n - 1);
    double zi = z;
    for (int i = 1; i < n - 1; ++i) {
      c0 += zi * (in(i) + zn * in(n - 1 - i));
      zi *= z;
    }
    c0 /= 1.0 - zn * zn;
    double prev = c0, prev2 = c0;
    c[0] = c0;
    for (int i = 1; i < n; ++i) {
      const double v = in(i) + z * prev;
      c[i * dstep] = v;
      prev2 = prev;
      prev = v;
    }
    double next = (z * prev2 + prev) * z / (z * z - 1.0);
    c[(n - 1) * dstep] = next;
    for (int i = n - 2; i >= 0; --i) {
      next = z * (next - c[i * dstep]);
      c[i * dstep] = next;
    }
  }
}

// axis 2: kRows rows per workgroup, kChunk columns at a time through LDS
template <typename S>
__global__ void __launch_bounds__(kRows) spline_rows_kernel(SplineArgs a) {
  __shared__ double fwd[kRows][kChunk + kPad];
  __shared__ double bwd[kRows][kChunk + kPad];
  const SfmSplineItem& it = a.items[blockIdx.y];
  const int n = it.shape[2];
  const bool from_image = convert_axis(it.shape) == 2;
  if (n == 1 && !from_image) return;
  const long long ny = it.shape[1];
  const long long rows = (long long)it.shape[0] * ny;
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
    double next = (z * prev2 + prev) * z / (z * z - 1.0);
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

}  // namespace

extern "C" int sfm_spline_prefilter(const SfmSplinePrefilterDesc* d) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: NULL argument");
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
    for (int k = 0; k < 3; ++k) {
      if (it.shape[k] < 1)
        return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: item %d: bad shape", t);
      size *= it.shape[k];
    }
    if (it.coeff_offset < 0 || size > d->coeffs_len || it.coeff_offset > d->coeffs_len - size)
      return sfm::fail(SFM_ERR_INVALID, "spline_prefilter: item %d leaves the coefficients", t);
    const long long z = it.shape[0], y = it.shape[1], x = it.shape[2];
    if (z > 1) max_lines[0] = std::max(max_lines[0], y * x);
    if (y > 1) max_lines[1] = std::max(max_lines[1], z * x);
    if (x > 1 || convert_axis(it.shape) == 2) max_lines[2] = std::max(max_lines[2], z * y);
  }
  SplineArgs a;
  a.items = d->items;
  a.coeffs = d->coeffs;
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
#define SFM_SPL(S)                                                        \
  do {                                                                    \
    if (ax == 2)                                                          \
      hipLaunchKernelGGL((spline_rows_kernel<S>), g, b, 0, st, a);        \
    else                                                                  \
      hipLaunchKernelGGL((spline_lines_kernel<S>), g, b, 0, st, a);       \
  } while (0)
    switch (d->dtype) {
      case SFM_DTYPE_U8: SFM_SPL(unsigned char); break;
      case SFM_DTYPE_U16: SFM_SPL(unsigned short); break;
      default: SFM_SPL(float); break;
    }
#undef SFM_SPL
    SFM_LAUNCH_CHECK();
  }
  return SFM_OK;
}
