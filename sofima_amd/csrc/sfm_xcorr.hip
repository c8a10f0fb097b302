// Patch cross-correlation + peak statistics for gfx950: batch driver, patch
// gather, the general shift-by-shift correlation kernel and the peak kernels.
//
// Device replacement for flow_field.py of the reference:
//   _batched_xcorr   (flow_field.py:278-371)  -> gather_kernel (clamped patch
//                     gather, per-patch (masked) mean, validity planes)
//   masked_xcorr     (flow_field.py:36-156)   -> corr_direct_kernel (+ the
//                     Padfield assembly and masked_finalize_kernel), or the
//                     int8 MFMA kernel in sfm_xcorr_mfma.hip for uint8 data
//   _batched_peaks / _peak_stats (flow_field.py:178-275)
//                                             -> peaks_first_kernel,
//                                                peaks_second_kernel
//
// The reference evaluates the full linear correlation with zero-padded FFTs;
// here every output shift is summed directly:
//     out[k] = sum_i A[i + k - (Q-1)] * B[i]      (zero shift at k = Q-1)
// which is the same quantity (oracle/flow_oracle.py checks both forms against
// the reference's own output).  The masked (Padfield) surface is assembled
// from six such sums exactly as SURVEY.md section 8a derives.
#include "sfm_xcorr_units.h"

#include <cfloat>
#include <cmath>
#include <cstring>

namespace {

constexpr int kBlock = 256;
constexpr int kCandCap = 2048;  // per-patch candidate list capacity
constexpr int kHotCap = 4096;   // per-patch hot list of the fused MFMA path
constexpr float kEps = 1.1920928955078125e-07f;  // float32 eps

struct Geo {
  int nd;
  int P[3], Q[3], S[3];  // [z]yx; S = P + Q - 1
  long long Pn, Qn, Sn;
};

int make_geo(const SfmXcorrDesc* d, Geo* g) {
  if (d->ndim != 2 && d->ndim != 3)
    return sfm::fail(SFM_ERR_INVALID, "ndim must be 2 or 3, got %d", d->ndim);
  g->nd = d->ndim;
  g->Pn = g->Qn = g->Sn = 1;
  for (int i = 0; i < 3; ++i) {
    g->P[i] = d->patch[i];
    g->Q[i] = d->post_patch[i];
    if (g->P[i] < 1 || g->Q[i] < 1)
      return sfm::fail(SFM_ERR_INVALID, "patch sizes must be >= 1");
    if (d->ndim == 2 && i == 0 && (g->P[0] != 1 || g->Q[0] != 1))
      return sfm::fail(SFM_ERR_INVALID, "2-D descriptors need patch[0] == 1");
    if (g->P[i] > d->pre_shape[i] || g->Q[i] > d->post_shape[i])
      return sfm::fail(SFM_ERR_INVALID, "patch larger than image on axis %d", i);
    g->S[i] = g->P[i] + g->Q[i] - 1;
    g->Pn *= g->P[i];
    g->Qn *= g->Q[i];
    g->Sn *= g->S[i];
  }
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// gather: clamped patch extraction, mean subtraction, mask zeroing
// ---------------------------------------------------------------------------
struct GatherArgs {
  const void* img;
  const unsigned char* mask;
  int ishape[3], mshape[3], psz[3];
  const int* starts;
  int nd;
  int use_mean;
  float mean;
  float* out;    // [B, psz]
  float* valid;  // [B, psz] or null
  long long pn;
};

template <typename T>
__global__ void __launch_bounds__(kBlock) gather_kernel(GatherArgs g0, GatherArgs g1) {
  const GatherArgs& g = blockIdx.y == 0 ? g0 : g1;
  const int b = blockIdx.x;
  __shared__ double s_sum[kBlock];
  __shared__ double s_cnt[kBlock];
  int st[3] = {0, 0, 0}, ms[3] = {0, 0, 0};
  for (int i = 0; i < g.nd; ++i) {
    const int v = g.starts[b * g.nd + i];
    const int ax = 3 - g.nd + i;
    // lax.dynamic_slice clamps the start so the slice stays in bounds; image
    // and mask are clamped against their own shapes.
    st[ax] = min(max(v, 0), g.ishape[ax] - g.psz[ax]);
    ms[ax] = min(max(v, 0), g.mshape[ax] - g.psz[ax]);
  }
  const T* img = static_cast<const T*>(g.img);
  const int py = g.psz[1], px = g.psz[2];
  const int pn = static_cast<int>(g.pn);  // < 2^16 here (larger patches: gather_big_kernel)
  // Eight elements per round, their loads issued as one straight-line group
  // (elements past the end repeat the last one and are ignored; the mask test
  // is hoisted: a branch between the loads would make each wait on its own).
  constexpr int kRound = 8;
  auto offsets = [&](int i, long long* off, long long* mo) {
    const int x = i % px;
    const int r = i / px;
    const int y = r % py;
    const int z = r / py;
    *off = ((long long)(st[0] + z) * g.ishape[1] + (st[1] + y)) * g.ishape[2] + (st[2] + x);
    *mo = ((long long)(ms[0] + z) * g.mshape[1] + (ms[1] + y)) * g.mshape[2] + (ms[2] + x);
  };
  auto fetch = [&](int i0, float* val, bool* masked) {
    if (g.mask) {
#pragma unroll
      for (int u = 0; u < kRound; ++u) {
        long long off, mo;
        offsets(min(i0 + u * kBlock, pn - 1), &off, &mo);
        val[u] = static_cast<float>(img[off]);
        masked[u] = g.mask[mo] != 0;
      }
    } else {
#pragma unroll
      for (int u = 0; u < kRound; ++u) {
        long long off, mo;
        offsets(min(i0 + u * kBlock, pn - 1), &off, &mo);
        val[u] = static_cast<float>(img[off]);
        masked[u] = false;
      }
    }
  };
  float mu = g.mean;
  if (!g.use_mean) {
    double s = 0.0, c = 0.0;
    for (int i0 = threadIdx.x; i0 < pn; i0 += kBlock * kRound) {
      float v[kRound];
      bool m[kRound];
      fetch(i0, v, m);
#pragma unroll
      for (int u = 0; u < kRound; ++u)
        if (i0 + u * kBlock < pn && !m[u]) {  // same order of additions as element by element
          s += v[u];
          c += 1.0;
        }
    }
    s_sum[threadIdx.x] = s;
    s_cnt[threadIdx.x] = c;
    __syncthreads();
    for (int k = kBlock / 2; k > 0; k >>= 1) {
      if (threadIdx.x < k) {
        s_sum[threadIdx.x] += s_sum[threadIdx.x + k];
        s_cnt[threadIdx.x] += s_cnt[threadIdx.x + k];
      }
      __syncthreads();
    }
    mu = static_cast<float>(s_sum[0] / s_cnt[0]);  // NaN when all masked
  }
  for (int i0 = threadIdx.x; i0 < pn; i0 += kBlock * kRound) {
    float v[kRound];
    bool m[kRound];
    fetch(i0, v, m);
#pragma unroll
    for (int u = 0; u < kRound; ++u) {
      const int i = i0 + u * kBlock;
      if (i < pn) {
        g.out[b * g.pn + i] = m[u] ? 0.f : v[u] - mu;
        if (g.valid) g.valid[b * g.pn + i] = m[u] ? 0.f : 1.f;
      }
    }
  }
}

// Large patches (3-D, whole overlaps): kGatherChunks workgroups per patch.
// PHASE 0 leaves per-chunk (sum, count) partials; PHASE 1 adds them in chunk
// order (every workgroup gets the identical mean) and writes its chunk.
constexpr int kGatherChunks = 32;

template <typename T, int PHASE>
__global__ void __launch_bounds__(kBlock)
gather_big_kernel(GatherArgs g0, GatherArgs g1, double* __restrict__ partial) {
  const GatherArgs& g = blockIdx.z == 0 ? g0 : g1;
  const int b = blockIdx.y, chunk = blockIdx.x;
  __shared__ double s_sum[kBlock];
  __shared__ double s_cnt[kBlock];
  int st[3] = {0, 0, 0}, ms[3] = {0, 0, 0};
  for (int i = 0; i < g.nd; ++i) {
    const int v = g.starts[b * g.nd + i];
    const int ax = 3 - g.nd + i;
    st[ax] = min(max(v, 0), g.ishape[ax] - g.psz[ax]);
    ms[ax] = min(max(v, 0), g.mshape[ax] - g.psz[ax]);
  }
  const T* img = static_cast<const T*>(g.img);
  const int py = g.psz[1], px = g.psz[2];
  const int rows = g.psz[0] * py;
  const int per = (rows + kGatherChunks - 1) / kGatherChunks;
  const int r0 = min(rows, chunk * per), r1 = min(rows, r0 + per);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* part = partial + ((long long)(blockIdx.z * gridDim.y + b) * kGatherChunks) * 2;
  float mu = g.mean;
  if (PHASE == 1 && !g.use_mean) {
    double s = 0.0, c = 0.0;
    for (int k = 0; k < kGatherChunks; ++k) {
      s += part[2 * k];
      c += part[2 * k + 1];
    }
    mu = static_cast<float>(s / c);  // NaN when all masked
  }
  double s = 0.0, c = 0.0;
  // Four rows x two 64-wide column groups per round, loads issued as one
  // straight-line group (clamped rows / columns, mask test hoisted); the sums
  // are still added in (row, column group) order.
  constexpr int kR = 4, kG = 2, kStep = kBlock / 64;
  for (int rb = r0 + wave; rb < r1; rb += kStep * kR) {
    for (int xb = 0; xb < px; xb += 64 * kG) {
      float v[kR][kG];
      bool m[kR][kG];
      long long io[kR], mo[kR];
#pragma unroll
      for (int j = 0; j < kR; ++j) {
        const int r = min(rb + j * kStep, r1 - 1);
        const int z = r / py, y = r - z * py;
        io[j] = ((long long)(st[0] + z) * g.ishape[1] + (st[1] + y)) * g.ishape[2] + st[2];
        mo[j] = ((long long)(ms[0] + z) * g.mshape[1] + (ms[1] + y)) * g.mshape[2] + ms[2];
      }
      if (g.mask) {
#pragma unroll
        for (int j = 0; j < kR; ++j)
#pragma unroll
          for (int k = 0; k < kG; ++k) {
            const int x = min(xb + lane + 64 * k, px - 1);
            v[j][k] = static_cast<float>(img[io[j] + x]);
            m[j][k] = g.mask[mo[j] + x] != 0;
          }
      } else {
#pragma unroll
        for (int j = 0; j < kR; ++j)
#pragma unroll
          for (int k = 0; k < kG; ++k) {
            v[j][k] = static_cast<float>(img[io[j] + min(xb + lane + 64 * k, px - 1)]);
            m[j][k] = false;
          }
      }
#pragma unroll
      for (int j = 0; j < kR; ++j)
#pragma unroll
        for (int k = 0; k < kG; ++k) {
          const int r = rb + j * kStep, x = xb + lane + 64 * k;
          if (r >= r1 || x >= px) continue;
          if (PHASE == 0) {
            if (!m[j][k]) {
              s += v[j][k];
              c += 1.0;
            }
          } else {
            const long long o = b * g.pn + (long long)r * px + x;
            g.out[o] = m[j][k] ? 0.f : v[j][k] - mu;
            if (g.valid) g.valid[o] = m[j][k] ? 0.f : 1.f;
          }
        }
    }
  }
  if (PHASE == 0) {
    s_sum[threadIdx.x] = s;
    s_cnt[threadIdx.x] = c;
    __syncthreads();
    for (int k = kBlock / 2; k > 0; k >>= 1) {
      if (threadIdx.x < k) {
        s_sum[threadIdx.x] += s_sum[threadIdx.x + k];
        s_cnt[threadIdx.x] += s_cnt[threadIdx.x + k];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      part[2 * chunk] = s_sum[0];
      part[2 * chunk + 1] = s_cnt[0];
    }
  }
}

// ---------------------------------------------------------------------------
// general direct correlation (any dim / dtype / masks)
// ---------------------------------------------------------------------------
struct CorrArgs {
  const float* a;   // [B, P] centred, masked pixels zeroed
  const float* b;   // [B, Q]
  const float* va;  // validity planes or null
  const float* vb;
  Geo g;
  float* out;       // unmasked: surface; masked: numerator
  float* den;       // masked only
  float* ov;        // masked only
  unsigned int* maxima;  // masked only: bits of max |den|, max overlap
};

template <bool MASKED>
__global__ void __launch_bounds__(kBlock) corr_direct_kernel(CorrArgs c) {
  const Geo& g = c.g;
  const int kx = blockIdx.x * 64 + (threadIdx.x & 63);
  const int ky = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int kz = blockIdx.z % g.S[0];
  const int bi = blockIdx.z / g.S[0];
  const bool live = kx < g.S[2] && ky < g.S[1];
  float xc = 0.f, sa = 0.f, sb = 0.f, nov = 0.f, qa = 0.f, qb = 0.f;
  if (live) {
    const int dz = kz - (g.Q[0] - 1), dy = ky - (g.Q[1] - 1),
              dx = kx - (g.Q[2] - 1);
    const int z0 = max(0, -dz), z1 = min(g.Q[0], g.P[0] - dz);
    const int y0 = max(0, -dy), y1 = min(g.Q[1], g.P[1] - dy);
    const int x0 = max(0, -dx), x1 = min(g.Q[2], g.P[2] - dx);
    const float* A = c.a + bi * g.Pn;
    const float* Bp = c.b + bi * g.Qn;
    const float* VA = MASKED ? c.va + bi * g.Pn : nullptr;
    const float* VB = MASKED ? c.vb + bi * g.Qn : nullptr;
    for (int z = z0; z < z1; ++z)
      for (int y = y0; y < y1; ++y) {
        const long long ao =
            ((long long)(z + dz) * g.P[1] + (y + dy)) * g.P[2] + dx;
        const long long bo = ((long long)z * g.Q[1] + y) * g.Q[2];
        // The product sum goes row by row: one accumulator over a whole 160 x 160
        // overlap collects 25 600 roundings at the magnitude of the total (up to 27 x
        // the deviation of the reference's float32 FFT form, measured element by
        // element against exact sums); a row sum and a sum of rows collect 160 + 160.
        // (The sums of the masked form below keep their single accumulators: their
        // consumers' tolerances are measured on that order and nothing has shown them short.)
        float row = 0.f;
        for (int x = x0; x < x1; ++x) {
          const float av = A[ao + x];
          const float bv = Bp[bo + x];
          row = fmaf(av, bv, row);
          if (MASKED) {
            const float wa = VA[ao + x];
            const float wb = VB[bo + x];
            sa = fmaf(av, wb, sa);
            sb = fmaf(wa, bv, sb);
            nov = fmaf(wa, wb, nov);
            qa = fmaf(av * av, wb, qa);
            qb = fmaf(wa, bv * bv, qb);
          }
        }
        xc += row;
      }
  }
  if (!live) return;
  const long long o =
      bi * g.Sn + ((long long)kz * g.S[1] + ky) * g.S[2] + kx;
  if (!MASKED) {
    c.out[o] = xc;
    return;
  }
  // Padfield assembly (flow_field.py:113-131).
  float ovv = fmaxf(rintf(nov), kEps);
  const float inv = 1.0f / ovv;
  const float num = xc - sa * sb * inv;
  const float pd = fmaxf(qa - sa * sa * inv, 0.f);
  const float cd = fmaxf(qb - sb * sb * inv, 0.f);
  const float den = sqrtf(pd * cd);
  c.out[o] = num;
  c.den[o] = den;
  c.ov[o] = ovv;
  // Batch-global maxima (flow_field.py:137, 151); values are >= 0 so the
  // integer order of the bit patterns is the float order.
  // (same-address atomics serialise: only the elements that raise a maximum)
  if (__float_as_uint(fabsf(den)) > __atomic_load_n(&c.maxima[0], __ATOMIC_RELAXED))
    atomicMax(&c.maxima[0], __float_as_uint(fabsf(den)));
  if (__float_as_uint(ovv) > __atomic_load_n(&c.maxima[1], __ATOMIC_RELAXED))
    atomicMax(&c.maxima[1], __float_as_uint(ovv));
}

__global__ void __launch_bounds__(kBlock)
masked_finalize_kernel(float* __restrict__ out, const float* __restrict__ den,
                       const float* __restrict__ ov,
                       const unsigned int* __restrict__ maxima, long long n) {
  const float tol = 1e3f * kEps * __uint_as_float(maxima[0]);
  const float px_thr = 0.3f * __uint_as_float(maxima[1]);
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n;
       i += (long long)gridDim.x * kBlock) {
    const float dn = den[i];
    float v = dn > tol ? out[i] / dn : 0.f;
    v = fminf(fmaxf(v, -1.f), 1.f);
    if (ov[i] < px_thr) v = 0.f;
    out[i] = v;
  }
}

// ---------------------------------------------------------------------------
// patch selection: masked-pixel count per grid patch
// ---------------------------------------------------------------------------
struct MaskCountArgs {
  const unsigned char* mask;
  int S[3], P[3], T[3], O[3];  // mask shape, patch, step, output grid
  int* out;
};

__global__ void __launch_bounds__(kBlock) mask_count_kernel(MaskCountArgs a) {
  __shared__ int red[kBlock];
  const long long o = blockIdx.x;
  const int ox = static_cast<int>(o % a.O[2]);
  const int oy = static_cast<int>((o / a.O[2]) % a.O[1]);
  const int oz = static_cast<int>(o / ((long long)a.O[2] * a.O[1]));
  const long long base =
      ((long long)oz * a.T[0] * a.S[1] + (long long)oy * a.T[1]) * a.S[2] +
      (long long)ox * a.T[2];
  const long long rows = (long long)a.P[0] * a.P[1];
  int cnt = 0;
  for (long long i = threadIdx.x; i < rows * a.P[2]; i += kBlock) {
    const int x = static_cast<int>(i % a.P[2]);
    const long long r = i / a.P[2];
    const int y = static_cast<int>(r % a.P[1]);
    const int z = static_cast<int>(r / a.P[1]);
    cnt += a.mask[base + ((long long)z * a.S[1] + y) * a.S[2] + x] != 0;
  }
  red[threadIdx.x] = cnt;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.out[o] = red[0];
}

// Same counts for patch rows that are not too wide: one workgroup per (tile of
// x outputs, oy, oz) adds the mask rows of the window column-wise (16 columns
// per thread, one 16-byte load per row), prefix-sums the column sums in LDS and
// writes every output of the tile as a difference of two prefix values.  Each
// mask byte is read P_y / T_y times instead of P_y P_x / (T_y T_x) times.
constexpr int kMcCols = 16 * kBlock;  // columns per tile

// 1 in every byte of w that is not zero
__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {
  return ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u) >> 7;
}

// `splits` > 1: few outputs with tall windows (whole-overlap patches): the window
// rows are divided among `splits` workgroups per tile, which add their partial
// counts atomically into the zeroed output (integers: order does not matter).
__global__ void __launch_bounds__(kBlock) mask_count_rows_kernel(MaskCountArgs a, int ot,
                                                                 int splits) {
  __shared__ int pref[kMcCols + 1];
  __shared__ int wsum[kBlock / 64];
  const int oy = blockIdx.y, oz = blockIdx.z;
  const int tile = blockIdx.x / splits, split = blockIdx.x - tile * splits;
  const int ox0 = tile * ot;
  const int nout = min(ot, a.O[2] - ox0);
  const int x0 = ox0 * a.T[2];
  const int ncol = (nout - 1) * a.T[2] + a.P[2];  // <= kMcCols
  const int c0 = 16 * threadIdx.x;
  const long long rows = (long long)a.P[0] * a.P[1];
  const long long per = (rows + splits - 1) / splits;
  const long long r_lo = min(rows, split * per), r_hi = min(rows, r_lo + per);
  int cs[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) cs[j] = 0;
  unsigned pk[4] = {0, 0, 0, 0};  // packed byte counters, flushed before they overflow
  int in_pk = 0;
  const bool whole = c0 + 16 <= ncol;  // x0 + ncol <= S[2] by construction
  for (long long r = r_lo; r < r_hi; ++r) {
    const int z = static_cast<int>(r / a.P[1]), y = static_cast<int>(r - (long long)z * a.P[1]);
    const unsigned char* row =
        a.mask + (((long long)oz * a.T[0] + z) * a.S[1] + (long long)oy * a.T[1] + y) * a.S[2] +
        x0 + c0;
    unsigned w[4] = {0, 0, 0, 0};
    if (whole) {
      __builtin_memcpy(w, row, 16);
    } else {
      for (int j = 0; j < 16; ++j)
        if (c0 + j < ncol) w[j >> 2] |= static_cast<unsigned>(row[j]) << (8 * (j & 3));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) pk[k] += nonzero_bytes(w[k]);
    if (++in_pk == 255 || r + 1 == r_hi) {
#pragma unroll
      for (int j = 0; j < 16; ++j) cs[j] += (pk[j >> 2] >> (8 * (j & 3))) & 0xffu;
      pk[0] = pk[1] = pk[2] = pk[3] = 0;
      in_pk = 0;
    }
  }
  // inclusive prefix over the tile's columns
  int run = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    run += cs[j];
    cs[j] = run;
  }
  int incl = run;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = incl - run;
  for (int k = 0; k < wave; ++k) base += wsum[k];
#pragma unroll
  for (int j = 0; j < 16; ++j) pref[c0 + j + 1] = base + cs[j];
  if (threadIdx.x == 0) pref[0] = 0;
  __syncthreads();
  for (int o = threadIdx.x; o < nout; o += kBlock) {
    int* dst = &a.out[((long long)oz * a.O[1] + oy) * a.O[2] + ox0 + o];
    const int cnt = pref[o * a.T[2] + a.P[2]] - pref[o * a.T[2]];
    if (splits > 1)
      atomicAdd(dst, cnt);
    else
      *dst = cnt;
  }
}

// Patches wider than a tile (whole-overlap strips): every output is cut into
// column segments of kMcCols and row ranges; a workgroup counts one piece and
// adds it atomically to the zeroed output.
__global__ void __launch_bounds__(kBlock) mask_count_wide_kernel(MaskCountArgs a, int nseg,
                                                                 int splits) {
  __shared__ int red[kBlock];
  const long long o = blockIdx.y;
  const int ox = static_cast<int>(o % a.O[2]);
  const int oy = static_cast<int>((o / a.O[2]) % a.O[1]);
  const int oz = static_cast<int>(o / ((long long)a.O[2] * a.O[1]));
  const int seg = blockIdx.x / splits, split = blockIdx.x - seg * splits;
  const int c0 = seg * kMcCols + 16 * threadIdx.x;  // first column of this thread
  const long long rows = (long long)a.P[0] * a.P[1];
  const long long per = (rows + splits - 1) / splits;
  const long long r_lo = min(rows, split * per), r_hi = min(rows, r_lo + per);
  const int nb = min(16, a.P[2] - c0);  // bytes of this thread inside the window
  int cnt = 0;
  if (nb > 0) {
    for (long long r = r_lo; r < r_hi; ++r) {
      const int z = static_cast<int>(r / a.P[1]), y = static_cast<int>(r - (long long)z * a.P[1]);
      const unsigned char* row =
          a.mask + (((long long)oz * a.T[0] + z) * a.S[1] + (long long)oy * a.T[1] + y) * a.S[2] +
          (long long)ox * a.T[2] + c0;
      unsigned w[4] = {0, 0, 0, 0};
      if (nb == 16) {
        __builtin_memcpy(w, row, 16);
      } else {
        for (int j = 0; j < nb; ++j) w[j >> 2] |= static_cast<unsigned>(row[j]) << (8 * (j & 3));
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) cnt += __builtin_popcount(nonzero_bytes(w[k]));
    }
  }
  red[threadIdx.x] = cnt;
  __syncthreads();
  for (int k = kBlock / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0]) atomicAdd(&a.out[o], red[0]);
}

// ---------------------------------------------------------------------------
// peaks
// ---------------------------------------------------------------------------
struct PeakArgs {
  const float* surf;  // [B, S] with row pitch / per-surface stride below
  int nd;
  int S[3];
  long long Sn;           // logical elements per surface
  int pitch;              // floats between consecutive x-rows (>= S[2])
  long long bstride;      // floats between consecutive surfaces
  int batch;
  float center[3];  // [z]yx
  int min_distance;
  float threshold_rel;
  int radius[3];
  // workspace
  int* idx1;               // [B]
  float* v1;               // [B]
  int* zero_is_peak;       // [B]
  int* cand_count;         // [B]
  float* cand_val;         // [B, kCandCap]
  int* cand_idx;           // [B, kCandCap]
  unsigned int* bitmap;    // [n_groups, bitmap_words]
  int group;               // rows per coupling group
  int bitmap_words;
  unsigned int* smax;        // [B] ordered bits of the surface maximum (large surfaces)
  unsigned long long* best;  // [B] packed (value, index) arg-max (large surfaces)
  float* out;              // [B, nd + 2]
  const int* skipmask;     // [B] or NULL: 16-row tiles of the surface that were never stored
  // masked matrix-core path: rows whose largest possible overlap ny * Qx is below
  // 0.3 x the batch maximum of the overlap are zero (flow_field.py:151-155); the
  // large-surface sweeps leave them out
  const unsigned int* live_ovmax;  // [groups, 2] (+1): float bits of the batch maximum of the overlap, or NULL
  // masked matrix-core path: maximum of every block of blk_rows surface rows, or NULL
  const float* blkmax;
  int blk_rows, blk_n;
  int live_py, live_qy, live_qx;
};

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

// (value, index) arg-max with first-index tie break across the block.
// (`better` is a total order on (value, -index): any reduction tree gives the same
// winner.  Butterfly over the wave on the shuffle network, then the waves' winners
// through LDS: two barriers instead of the nine of an LDS tree -- the peak kernels
// run one workgroup per surface and are priced by their chains of round trips.)
__device__ void block_argmax(float* v, int* i, float* lv, int* li) {
  float bv = *v;
  int bi = *i;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const float ov = __shfl_xor(bv, d, 64);
    const int oi = __shfl_xor(bi, d, 64);
    if (better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    lv[threadIdx.x >> 6] = bv;
    li[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  bv = lv[0];
  bi = li[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w)
    if (better(lv[w], li[w], bv, bi)) {
      bv = lv[w];
      bi = li[w];
    }
  *v = bv;
  *i = bi;
  __syncthreads();
}

// Element (z, y, x) of a surface with row pitch.
__device__ __forceinline__ float surf_at(const float* s, const PeakArgs& p, int z,
                                         int y, int x) {
  return s[((long long)z * p.S[1] + y) * p.pitch + x];
}

// img == maxfilter(img) (zero 'same' padding) for an element already known to
// exceed the threshold (flow_field.py:238-254).
// FAST: the 5 x 5 window of the default min_distance as 25 loads in flight (costs
// registers: not for kernels where this is the rare path).
template <bool FAST>
__device__ bool is_window_max(const float* s, const PeakArgs& p, int z, int y,
                              int x, float v) {
  const int m = p.min_distance;
  const int mz = p.nd == 3 ? m : 0;
  // window maximum from clamped addresses: unconditional loads (all in flight
  // together); a clamped position repeats an element of the window, which cannot
  // change the maximum
  float wm = -INFINITY;
  const bool outside = z - mz < 0 || z + mz >= p.S[0] || y - m < 0 || y + m >= p.S[1] ||
                       x - m < 0 || x + m >= p.S[2];
  if (FAST && m == 2) {  // the default min_distance: a plane's 25 loads in flight together
    for (int dz = -mz; dz <= mz; ++dz) {
      float w[25];
      const int zz = min(max(z + dz, 0), p.S[0] - 1);
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
          w[(dy + 2) * 5 + dx + 2] = surf_at(s, p, zz, min(max(y + dy, 0), p.S[1] - 1),
                                             min(max(x + dx, 0), p.S[2] - 1));
#pragma unroll
      for (int k = 0; k < 25; ++k) wm = fmaxf(wm, w[k]);
    }
  } else {
    for (int dz = -mz; dz <= mz; ++dz)
      for (int dy = -m; dy <= m; ++dy)
        for (int dx = -m; dx <= m; ++dx)
          wm = fmaxf(wm, surf_at(s, p, min(max(z + dz, 0), p.S[0] - 1),
                                 min(max(y + dy, 0), p.S[1] - 1),
                                 min(max(x + dx, 0), p.S[2] - 1)));
  }
  if (outside) wm = fmaxf(wm, 0.f);
  return v == wm;
}

// Row sweeps of the peak search: a wave takes whole rows and issues the loads of
// a piece -- G 64-wide column groups of R consecutive rows of its share, G R = 8
// -- before it looks at the first value (clamped addresses, no load under a
// per-lane condition: otherwise every load is waited for on its own).  G is the
// smallest of 1, 2, 4, 8 that covers the row, so narrow rows do not pay for
// column groups that only repeat their last element.
constexpr int kPiece = 8;

template <int G, typename Body>
__device__ __forceinline__ void sweep_rows(const float* s, const PeakArgs& p, int r0, int rows,
                                           Body body) {
  constexpr int R = kPiece / G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = p.S[2];
  constexpr int kStep = kBlock / 64;  // rows are dealt to the waves round robin
  for (int rb = r0 + wave; rb < rows; rb += kStep * R) {
    for (int xb = 0; xb < w; xb += 64 * G) {
      float v[R][G];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const float* row = s + (long long)min(rb + j * kStep, rows - 1) * p.pitch;
#pragma unroll
        for (int k = 0; k < G; ++k) v[j][k] = row[min(xb + lane + 64 * k, w - 1)];
      }
#pragma unroll
      for (int j = 0; j < R; ++j)
#pragma unroll
        for (int k = 0; k < G; ++k) {
          const int r = rb + j * kStep, x = xb + lane + 64 * k;
          if (r < rows && x < w) body(r, x, v[j][k]);
        }
    }
  }
}

template <typename Body>
__device__ __forceinline__ void sweep_rows_any(const float* s, const PeakArgs& p, int r0, int rows,
                                               Body body) {
  const int w = p.S[2];
  if (w <= 64)
    sweep_rows<1>(s, p, r0, rows, body);
  else if (w <= 128)
    sweep_rows<2>(s, p, r0, rows, body);
  else if (w <= 256)
    sweep_rows<4>(s, p, r0, rows, body);
  else
    sweep_rows<8>(s, p, r0, rows, body);
}

// NANS: a NaN element makes the maximum NaN, as the reference's img.max() does
// (fmaxf drops it).  Only the stand-alone entry asks for it: the surfaces of the
// fused producers are sums of integer products and hold none.
template <bool NANS = false>
__device__ float surface_max(const float* s, const PeakArgs& p, float* lv,
                             int* li, int r0 = 0, int r1 = -1) {
  const int rows = r1 < 0 ? p.S[0] * p.S[1] : r1;
  float mx = -INFINITY;
  int bad = 0;
  sweep_rows_any(s, p, r0, rows, [&](int, int, float v) {
    mx = fmaxf(mx, v);
    if (NANS) bad |= v != v;
  });
  int dummy = 0;
  block_argmax(&mx, &dummy, lv, li);
  if (NANS && __syncthreads_or(bad)) mx = NAN;
  return mx;
}

// Calls fn(flat_index, value) for every peak of the surface.
template <bool FAST = true, typename F>
__device__ void for_each_peak(const float* s, const PeakArgs& p, float thr, F fn,
                              int r0 = 0, int r1 = -1) {
  const int rows = r1 < 0 ? p.S[0] * p.S[1] : r1;
  const int w = p.S[2];
  sweep_rows_any(s, p, r0, rows, [&](int r, int x, float v) {
    if (v > thr) {
      const int z = r / p.S[1], y = r - z * p.S[1];
      if (is_window_max<FAST>(s, p, z, y, x, v)) fn(r * w + x, v);
    }
  });
}

// (a NaN maximum makes the threshold NaN: nothing exceeds it, the row is NaN and
// its first-peak index 0 -- the reference's arg-max of an all -inf row)
template <bool NANS>
__global__ void __launch_bounds__(kBlock) peaks_first_kernel(PeakArgs p) {
  __shared__ float lv[kBlock];
  __shared__ int li[kBlock];
  const int b = blockIdx.x;
  const float* s = p.surf + b * p.bstride;
  const float mx = surface_max<NANS>(s, p, lv, li);
  const float thr = p.threshold_rel * mx;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for_each_peak(s, p, thr, [&](int i, float v) {
    if (better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
    const int slot = atomicAdd(&p.cand_count[b], 1);
    if (slot < kCandCap) {
      p.cand_val[(long long)b * kCandCap + slot] = v;
      p.cand_idx[(long long)b * kCandCap + slot] = i;
    }
    if (i == 0) p.zero_is_peak[b] = 1;
  });
  block_argmax(&bv, &bi, lv, li);
  if (threadIdx.x == 0) {
    const int i1 = bv == -INFINITY ? 0 : bi;  // argmax of an all -inf row is 0
    p.idx1[b] = i1;
    p.v1[b] = bv;
    sfm::set_bit_once(&p.bitmap[(long long)(b / p.group) * p.bitmap_words + (i1 >> 5)],
                       1u << (i1 & 31));
  }
}

// ---- first pass over LARGE surfaces (3-D, whole-overlap patches): several
// workgroups per surface.  Floats are ordered through a monotonic uint map so
// that the surface maximum and the (value, lowest index) arg-max can be merged
// with integer atomics; the result is identical to peaks_first_kernel.
__device__ __forceinline__ unsigned ord_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_float(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ void chunk_rows(const PeakArgs& p, int b, int* r0, int* r1) {
  int lo = 0, hi = p.S[0] * p.S[1];
  if (p.live_ovmax && p.S[0] == 1) {
    // ny(ky) rises to min(Py, Qy) and falls again: the live rows are one range
    // (two maxima per reference batch: denominator, overlap)
    const float thr = 0.3f * __uint_as_float(p.live_ovmax[2 * (b / p.group)]);
    auto dead = [&](int ky) {
      const int dy = ky - (p.live_qy - 1);
      const int ny = min(p.live_py, p.live_qy + dy) - max(0, dy);
      return static_cast<float>(ny * p.live_qx) < thr;
    };
    while (lo < hi && dead(lo)) ++lo;
    while (hi > lo && dead(hi - 1)) --hi;
  }
  const int rows = hi - lo;
  const int per = (rows + gridDim.x - 1) / gridDim.x;
  *r0 = lo + min(rows, static_cast<int>(blockIdx.x) * per);
  *r1 = lo + min(rows, static_cast<int>(blockIdx.x) * per + per);
}

// (a NaN maximum travels as the largest ordered word, above +inf: it wins every
// merge and ord_float gives a NaN back)
template <bool NANS>
__global__ void __launch_bounds__(kBlock) peaks_max_kernel(PeakArgs p) {
  __shared__ float lv[kBlock];
  __shared__ int li[kBlock];
  const int b = blockIdx.y;
  int r0, r1;
  chunk_rows(p, b, &r0, &r1);
  const float mx = surface_max<NANS>(p.surf + b * p.bstride, p, lv, li, r0, r1);
  if (threadIdx.x == 0 && r1 > r0)
    atomicMax(&p.smax[b], NANS && mx != mx ? 0xffffffffu : ord_bits(mx));
}

__global__ void __launch_bounds__(kBlock) peaks_scan_kernel(PeakArgs p) {
  __shared__ float lv[kBlock];
  __shared__ int li[kBlock];
  // (with block maxima most surfaces cost a handful of loads: a workgroup walks
  // several of them, or the launch is bound by the workgroup dispatch rate)
  for (int b = blockIdx.y; b < p.batch; b += gridDim.y) {
  const float* s = p.surf + b * p.bstride;
  int r0, r1;
  chunk_rows(p, b, &r0, &r1);
  const float thr = p.threshold_rel * ord_float(p.smax[b]);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  auto found = [&](int i, float v) {
    if (better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
    const int slot = atomicAdd(&p.cand_count[b], 1);
    if (slot < kCandCap) {
      p.cand_val[(long long)b * kCandCap + slot] = v;
      p.cand_idx[(long long)b * kCandCap + slot] = i;
    }
    if (i == 0) p.zero_is_peak[b] = 1;
  };
  if (p.blkmax) {
    // a peak exceeds thr: blocks of rows whose maximum does not are not read
    // (lane k of every wave looks at block k: one round trip for the whole list)
    const int lane = threadIdx.x & 63;
    const int kc = min(lane, p.blk_n - 1);
    const bool hot = p.blkmax[(long long)b * p.blk_n + kc] > thr && lane < p.blk_n &&
                     lane * p.blk_rows < r1 && (lane + 1) * p.blk_rows > r0;
    unsigned long long todo = __ballot(hot);
    while (todo) {
      const int k = __builtin_ctzll(todo);
      todo &= todo - 1;
      for_each_peak(s, p, thr, found, max(r0, k * p.blk_rows), min(r1, (k + 1) * p.blk_rows));
    }
  } else {
    for_each_peak(s, p, thr, found, r0, r1);
  }
  block_argmax(&bv, &bi, lv, li);
  if (threadIdx.x == 0 && bv != -INFINITY)
    atomicMax(&p.best[b], (static_cast<unsigned long long>(ord_bits(bv)) << 32) |
                              (0xffffffffu - static_cast<unsigned>(bi)));
  }
}

__global__ void __launch_bounds__(kBlock) peaks_first_finish_kernel(PeakArgs p) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= p.batch) return;
  const unsigned long long k = p.best[b];
  const float bv = k ? ord_float(static_cast<unsigned>(k >> 32)) : -INFINITY;
  const int i1 = k ? static_cast<int>(0xffffffffu - static_cast<unsigned>(k)) : 0;
  p.idx1[b] = i1;
  p.v1[b] = bv;
  sfm::set_bit_once(&p.bitmap[(long long)(b / p.group) * p.bitmap_words + (i1 >> 5)],
                       1u << (i1 & 31));
}

// Second peak + sharpness of surface b.  WAVE: by one wave (lanes instead of
// threads, reductions on the shuffle network, no barrier) -- the common case, a
// candidate list that did not overflow; otherwise by the whole workgroup.
template <bool WAVE>
__device__ void second_peak_body(const PeakArgs& p, int b, float* lv, int* li) {
  constexpr int NT = WAVE ? 64 : kBlock;
  const int tid = WAVE ? static_cast<int>(threadIdx.x & 63) : static_cast<int>(threadIdx.x);
  const float* s = p.surf + b * p.bstride;
  const float v1 = p.v1[b];
  const int i1 = p.idx1[b];
  const int w = p.nd + 2;
  const unsigned int* bitmap = p.bitmap + (long long)(b / p.group) * p.bitmap_words;
  if (v1 == -INFINITY) {
    if (tid < w) p.out[b * w + tid] = NAN;
    return;
  }
  // Sharpness window (flow_field.py:186-192): its position depends on the first
  // peak only, so its loads go out first and return behind the candidate list's
  // (one round trip less in this kernel's chain).
  int pos[3], start[3], size[3];
  {
    long long r = i1;
    pos[2] = static_cast<int>(r % p.S[2]);
    r /= p.S[2];
    pos[1] = static_cast<int>(r % p.S[1]);
    pos[0] = static_cast<int>(r / p.S[1]);
  }
  long long wn = 1;
  for (int a = 0; a < 3; ++a) {
    size[a] = (a == 0 && p.nd == 2) ? 1 : 2 * p.radius[a] + 1;
    size[a] = min(size[a], p.S[a]);
    start[a] = min(max(pos[a] - size[a] / 2, 0), p.S[a] - size[a]);
    wn *= size[a];
  }
  float mn = INFINITY;
  for (long long k = tid; k < wn; k += NT) {
    const int x = static_cast<int>(k % size[2]);
    const long long r = k / size[2];
    const int y = static_cast<int>(r % size[1]);
    const int z = static_cast<int>(r / size[1]);
    mn = fminf(mn, surf_at(s, p, start[0] + z, start[1] + y, start[2] + x));
  }
  const float peak_val = surf_at(s, p, pos[0], pos[1], pos[2]);
  // Second peak: best candidate whose flat index is not a first-peak index of
  // ANY surface in the batch (flow_field.py:263-265).
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  const int cnt = p.cand_count[b];
  if (WAVE || cnt <= kCandCap) {
    for (int k = tid; k < cnt; k += NT) {
      const float v = p.cand_val[(long long)b * kCandCap + k];
      const int i = p.cand_idx[(long long)b * kCandCap + k];
      if ((bitmap[i >> 5] >> (i & 31)) & 1u) continue;
      if (better(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    }
  } else if constexpr (!WAVE) {
    // Candidate list overflowed (plateaus): rescan the surface.  Row tiles the
    // correlation kernel pruned were never stored (all their elements are below
    // the threshold): zeros for the sweep.
    const int skipped = p.skipmask ? p.skipmask[b] : 0;
    if (skipped) {
      float* sw = const_cast<float*>(s);
      for (int t = 0; t < 32; ++t) {
        if (!((skipped >> t) & 1)) continue;
        const int y1 = min(16 * t + 16, p.S[1]);
        for (int i = threadIdx.x; i < (y1 - 16 * t) * p.S[2]; i += kBlock)
          sw[(long long)(16 * t + i / p.S[2]) * p.pitch + i % p.S[2]] = 0.f;
      }
      __threadfence_block();
      __syncthreads();
    }
    const float mx = surface_max(s, p, lv, li);
    for_each_peak<false>(s, p, p.threshold_rel * mx, [&](int i, float v) {
      if (((bitmap[i >> 5] >> (i & 31)) & 1u) == 0 && better(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    });
  }
  if constexpr (WAVE) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const float ov = __shfl_xor(bv, d, 64);
      const int oi = __shfl_xor(bi, d, 64);
      if (better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
  } else {
    block_argmax(&bv, &bi, lv, li);
  }
  // The value is read from the UN-suppressed array (flow_field.py:266-268):
  // with nothing left the arg-max is index 0, whose value is the surface value
  // there if index 0 is itself a peak.
  float v2 = bv;
  if (bv == -INFINITY && p.zero_is_peak[b]) v2 = s[0];

  // Sharpness: peak / min over the clamped window (loaded above).
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) mn = fminf(mn, __shfl_xor(mn, d, 64));
  if constexpr (!WAVE) {
    if ((threadIdx.x & 63) == 0) lv[threadIdx.x >> 6] = mn;
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
      for (int w2 = 0; w2 < kBlock / 64; ++w2) mn = fminf(mn, lv[w2]);
  }
  if (tid == 0) {
    float* o = p.out + b * w;
    // x, y[, z] = reversed axis order
    for (int a = 0; a < p.nd; ++a) {
      const int ax = 2 - a;
      o[a] = static_cast<float>(pos[ax]) - p.center[ax];
    }
    o[p.nd] = peak_val / mn;
    o[p.nd + 1] = v2 == -INFINITY ? 0.f : v1 / v2;
  }
}


// Four surfaces per workgroup, a wave each (40 401 workgroups of one short chain
// of round trips were priced by their dispatch); a workgroup in which any
// candidate list overflowed takes its surfaces one after the other instead.
__global__ void __launch_bounds__(kBlock) peaks_second_kernel(PeakArgs p) {
  __shared__ float lv[kBlock];
  __shared__ int li[kBlock];
  constexpr int kPer = kBlock / 64;
  const int b = blockIdx.x * kPer + static_cast<int>(threadIdx.x >> 6);
  const bool live = b < p.batch;
  const int cnt = live ? p.cand_count[b] : 0;
  if (!__syncthreads_or(cnt > kCandCap ? 1 : 0)) {
    if (live) second_peak_body<true>(p, b, nullptr, nullptr);
    return;
  }
  for (int w2 = 0; w2 < kPer; ++w2) {
    const int bb = blockIdx.x * kPer + w2;
    if (bb < p.batch) second_peak_body<false>(p, bb, lv, li);
    __syncthreads();
  }
}

// Copies a tile-padded surface [B, rows, pitch] into the compact [B, Sy, Sx].
__global__ void __launch_bounds__(kBlock)
compact_surface_kernel(const float* __restrict__ src, float* __restrict__ dst,
                       int sy, int sx, int rows, int pitch) {
  const int b = blockIdx.y;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < sy * sx;
       i += gridDim.x * kBlock) {
    const int y = i / sx, x = i - y * sx;
    dst[(long long)b * sy * sx + i] = src[((long long)b * rows + y) * pitch + x];
  }
}

struct PeakWs {
  sfm::FusedPeaks f;   // what the fused matrix-core pass shares with the peak kernels
  unsigned int* smax;
  float* blkmax;       // masked MFMA path only: [batch, kBlkMaxN]
  unsigned long long* best;
  char* zero;          // state that clear_peak_state() clears per batch
  size_t zero_bytes;
  size_t bytes;
};

constexpr int kBlkMaxN = 16;   // blocks of sfm::kMaskedBlkRows rows: surfaces up to 512 rows

// hot: the hot lists of the fused MFMA path; blk: the block maxima of the masked one.
PeakWs carve_peaks(sfm::Carver& c, int batch, long long sn, bool hot = false,
                   int group = 0, bool blk = false) {
  PeakWs w;
  sfm::FusedPeaks& f = w.f;
  w.blkmax = blk ? c.take<float>((size_t)batch * kBlkMaxN) : nullptr;
  f.group = group > 0 && group < batch ? group : batch;
  f.bitmap_words = static_cast<int>((sn + 31) / 32);
  f.idx1 = c.take<int>(batch);
  f.v1 = c.take<float>(batch);
  f.hot_cap = kHotCap;
  f.hot_val = hot ? c.take<float>((size_t)batch * kHotCap) : nullptr;
  f.hot_idx = hot ? c.take<int>((size_t)batch * kHotCap) : nullptr;
  f.cand_cap = kCandCap;
  f.cand_val = c.take<float>((size_t)batch * kCandCap);
  f.cand_idx = c.take<int>((size_t)batch * kCandCap);
  const size_t z0 = sfm::align_up(c.off, 256);
  f.zero_is_peak = c.take<int>(batch);
  f.cand_count = c.take<int>(batch);
  f.hot_count = c.take<int>(batch);
  f.skipmask = c.take<int>(batch);
  w.smax = c.take<unsigned int>(batch);
  w.best = c.take<unsigned long long>(batch);
  f.bitmap = c.take<unsigned int>((size_t)((batch + f.group - 1) / f.group) * f.bitmap_words);
  w.zero = c.base ? c.base + z0 : nullptr;
  w.zero_bytes = c.total() - z0;
  w.bytes = c.total();
  return w;
}

// The per-batch peak state is cleared once per batch, before the first kernel that
// writes it.  That is the surface producer when it runs the first peak pass or
// delivers the surface maxima (PeakDone): the driver clears before it launches one.
// Otherwise run_peaks clears.
int clear_peak_state(const PeakWs& w, hipStream_t st) {
  SFM_HIP_CHECK(hipMemsetAsync(w.zero, 0, w.zero_bytes, st));
  return SFM_OK;
}

int check_workspace(const char* unit, const void* ws, size_t have, size_t need) {
  if (!ws || have < need)
    return sfm::fail(SFM_ERR_WORKSPACE, "%s workspace needs %zu bytes, got %zu", unit,
                     need, have);
  return SFM_OK;
}

struct SurfaceLayout {
  const float* surf;  // [batch, S] with the row pitch and per-surface stride below
  int nd;
  const int* S;       // [z]yx
  long long Sn;
  int pitch;
  long long bstride;
  int batch;
};

// Desc: SfmXcorrDesc or SfmPeaksDesc, for the peak parameters they share.
template <typename Desc>
PeakArgs make_peak_args(const PeakWs& w, const SurfaceLayout& s, const Desc& q,
                        const float* center, float* out) {
  PeakArgs p = {};  // the masked matrix-core extras (live_*, blkmax) stay off
  p.surf = s.surf;
  p.nd = s.nd;
  for (int i = 0; i < 3; ++i) {
    p.S[i] = s.S[i];
    p.center[i] = center[i];
    p.radius[i] = q.peak_radius[i];
  }
  p.Sn = s.Sn;
  p.pitch = s.pitch;
  p.bstride = s.bstride;
  p.batch = s.batch;
  p.min_distance = q.min_distance;
  p.threshold_rel = q.threshold_rel;
  p.idx1 = w.f.idx1;
  p.v1 = w.f.v1;
  p.zero_is_peak = w.f.zero_is_peak;
  p.skipmask = w.f.skipmask;
  p.cand_count = w.f.cand_count;
  p.cand_val = w.f.cand_val;
  p.cand_idx = w.f.cand_idx;
  p.bitmap = w.f.bitmap;
  p.group = w.f.group;
  p.bitmap_words = w.f.bitmap_words;
  p.smax = w.smax;
  p.best = w.best;
  p.out = out;
  p.blk_rows = sfm::kMaskedBlkRows;
  p.blk_n = (s.S[1] + sfm::kMaskedBlkRows - 1) / sfm::kMaskedBlkRows;
  return p;
}

// What the producer of the surfaces has already done for the peak search.
struct PeakDone {
  bool first_pass;  // the whole first pass
  bool smax;        // the surface maxima are in PeakWs::smax
  bool nans;        // not done, asked for: the NaN-propagating surface maximum
};

int run_peaks(const PeakArgs& p, const PeakDone& done, const PeakWs& w, hipStream_t st) {
  const int batch = p.batch;
  if (!done.first_pass) {
    if (!done.smax)
      if (int rc = clear_peak_state(w, st)) return rc;
    if (p.Sn >= (1LL << 18) || done.smax) {
      // large surfaces: ~32 K elements per workgroup
      const long long rows = (long long)p.S[0] * p.S[1];
      const int chunks = static_cast<int>(std::min<long long>(
          std::min<long long>(rows, 1024), std::max<long long>(1, p.Sn >> 15)));
      if (!done.smax) {
        if (done.nans)
          hipLaunchKernelGGL(peaks_max_kernel<true>, dim3(chunks, batch), dim3(kBlock), 0, st, p);
        else
          hipLaunchKernelGGL(peaks_max_kernel<false>, dim3(chunks, batch), dim3(kBlock), 0, st, p);
      }
      if (p.blkmax)   // one workgroup per surface, at most 4096 of them
        hipLaunchKernelGGL(peaks_scan_kernel, dim3(1, std::min(batch, 4096)), dim3(kBlock), 0, st, p);
      else
        hipLaunchKernelGGL(peaks_scan_kernel, dim3(chunks, batch), dim3(kBlock), 0, st, p);
      hipLaunchKernelGGL(peaks_first_finish_kernel, dim3((batch + kBlock - 1) / kBlock),
                         dim3(kBlock), 0, st, p);
    } else if (done.nans) {
      hipLaunchKernelGGL(peaks_first_kernel<true>, dim3(batch), dim3(kBlock), 0, st, p);
    } else {
      hipLaunchKernelGGL(peaks_first_kernel<false>, dim3(batch), dim3(kBlock), 0, st, p);
    }
    SFM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(peaks_second_kernel, dim3((batch + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, st, p);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// batch driver
// ---------------------------------------------------------------------------
enum class Path { Direct, Fft, Mfma, MfmaMasked };
enum class Entry { Size, Surface, Peaks };

// The masked matrix-core path takes kMaskedGroups groups per round of launches:
// its product surfaces are 4 GB per 1024 patches of 160^2 (SFM_MASKED_GROUPS).
constexpr int kMaskedGroups = 8;

// Everything an entry call decides before it launches (DESIGN.md has the table);
// built once by make_plan, shared by the sizing and by every round of the run.
struct XcorrPlan {
  const SfmXcorrDesc* d;
  Geo g;
  Path path;
  bool mfma, masked;        // mfma: either matrix-core path
  bool peaks;               // Entry::Surface carves no peak state
  int group;                // rows that share the batch-coupled state
  long long round;          // rows per round of launches (a multiple of the group)
  PeakDone done;            // what the producer of the surfaces does of the peak search
  bool blkmax_ws;           // the producer writes block maxima (kBlkMaxN holds them)
  bool blkmax, live_rows;   // the peak sweeps use them (SFM_MASKED_BLKMAX / _DEADROWS)
};

// `out`: the result pointer of the run entries.
int make_plan(const SfmXcorrDesc* d, Entry e, const void* out, XcorrPlan* p) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "desc is NULL");
  if (d->batch < 1) return sfm::fail(SFM_ERR_INVALID, "batch must be >= 1");
  if (d->group < 0) return sfm::fail(SFM_ERR_INVALID, "group must be >= 0");
  if (!d->pre_image || !d->post_image || !d->pre_starts || !d->post_starts)
    return sfm::fail(SFM_ERR_INVALID, "image / starts pointers must be set");
  if (d->dtype != SFM_DTYPE_U8 && d->dtype != SFM_DTYPE_F32)
    return sfm::fail(SFM_ERR_INVALID, "unsupported dtype tag %d", d->dtype);
  if (d->method < SFM_XCORR_AUTO || d->method > SFM_XCORR_FFT)
    return sfm::fail(SFM_ERR_INVALID, "unknown method %d", d->method);
  const bool mfma = (d->method == SFM_XCORR_AUTO || d->method == SFM_XCORR_MFMA_I8) &&
                    sfm::mfma_i8_eligible(d);
  if (d->method == SFM_XCORR_MFMA_I8 && !mfma)
    return sfm::fail(SFM_ERR_INVALID,
                     "MFMA_I8 needs uint8 2-D images, post patches up to 160 wide and (un-masked) pre patches up to 320 wide");
  if (e == Entry::Surface && !out) return sfm::fail(SFM_ERR_INVALID, "surface is NULL");
  if (e == Entry::Peaks && !out) return sfm::fail(SFM_ERR_INVALID, "peaks is NULL");
  if (int rc = make_geo(d, &p->g)) return rc;
  p->d = d;
  p->mfma = mfma;
  p->masked = d->pre_mask || d->post_mask;
  // FFT form: on request, or automatically for the patches the matrix-core
  // kernel does not take once they are large enough (3-D, float, wide).
  if (mfma)
    p->path = p->masked ? Path::MfmaMasked : Path::Mfma;
  else if (d->method == SFM_XCORR_FFT || (d->method == SFM_XCORR_AUTO && sfm::fft_preferred(d)))
    p->path = Path::Fft;
  else
    p->path = Path::Direct;
  // (the run leaves this check to fft_correlate, behind its workspace check)
  if (e == Entry::Size && p->path == Path::Fft)
    if (int rc = sfm::fft_check(d)) return rc;
  p->peaks = e != Entry::Surface;
  p->group = d->group > 0 && d->group < d->batch ? d->group : d->batch;
  p->done = {p->path == Path::Mfma,
             p->path == Path::MfmaMasked || (p->path == Path::Fft && !p->masked), false};
  p->blkmax_ws = p->path == Path::MfmaMasked &&
                 (p->g.S[1] + sfm::kMaskedBlkRows - 1) / sfm::kMaskedBlkRows <= kBlkMaxN;
  p->blkmax = p->blkmax_ws && sfm::option_on("SFM_MASKED_BLKMAX");
  p->live_rows = p->path == Path::MfmaMasked && sfm::option_on("SFM_MASKED_DEADROWS");
  // The fused matrix-core path keeps the coupled state per group and takes any
  // number of groups in one launch; the masked one keeps its maxima per group;
  // every other path, and every masked surface call, runs group by group.
  const bool whole = e == Entry::Surface ? !p->masked : p->path == Path::Mfma;
  p->round = whole ? d->batch : p->group;
  if (e != Entry::Surface && p->path == Path::MfmaMasked && p->group < d->batch)
    p->round = std::min<long long>(
        d->batch, p->round * std::max(1, sfm::option_int("SFM_MASKED_GROUPS", kMaskedGroups)));
  return SFM_OK;
}

struct XcorrWs {
  float *a0, *b0, *va, *vb, *surface, *den, *ov;
  unsigned int* maxima;
  void* mfma;
  void* fft;
  double* gather_part;  // large patches: per-chunk (sum, count) partials
  PeakWs peaks;
  int srows, spitch;  // layout of `surface`: [B, srows, spitch]
  size_t bytes;
};

// Rows `off` .. `off + rows` of the call.
SfmXcorrDesc sub_desc(const XcorrPlan& p, long long off, long long rows) {
  SfmXcorrDesc sub = *p.d;
  sub.batch = static_cast<int>(rows);
  sub.group = p.group;
  sub.pre_starts += off * sub.ndim;
  sub.post_starts += off * sub.ndim;
  return sub;
}

XcorrWs carve_xcorr(const XcorrPlan& p, long long rows, int group, void* base) {
  SfmXcorrDesc q = *p.d;  // what the other units size by
  q.batch = static_cast<int>(rows);
  q.group = group;
  const Geo& g = p.g;
  sfm::Carver c(base);
  XcorrWs w;
  std::memset(&w, 0, sizeof(w));
  const size_t B = rows;
  w.srows = g.S[0] * g.S[1];
  w.spitch = g.S[2];
  if (p.mfma) {
    w.mfma = c.take<char>(sfm::mfma_i8_workspace_bytes(&q));
    if (p.masked) {  // two maxima per reference batch of the call
      const size_t per = group > 0 && group < rows ? group : rows;
      w.maxima = c.take<unsigned int>(2 * ((B + per - 1) / per));
    }
    // The MFMA kernel stores whole 16 x 16 tiles: padded work surface.
    sfm::mfma_i8_padded_dims(&q, &w.srows, &w.spitch);
  } else {
    w.a0 = c.take<float>(B * g.Pn);
    w.b0 = c.take<float>(B * g.Qn);
    if (p.masked) {
      w.va = c.take<float>(B * g.Pn);
      w.vb = c.take<float>(B * g.Qn);
      w.den = c.take<float>(B * g.Sn);
      w.ov = c.take<float>(B * g.Sn);
      w.maxima = c.take<unsigned int>(2);
    }
    if (p.path == Path::Fft) w.fft = c.take<char>(sfm::fft_workspace_bytes(&q));
    if (std::max(g.Pn, g.Qn) >= (1LL << 16))
      w.gather_part = c.take<double>(B * 2 * kGatherChunks * 2);
  }
  if (p.peaks || p.mfma)
    w.surface = c.take<float>(B * (size_t)w.srows * w.spitch);
  if (p.peaks)
    w.peaks = carve_peaks(c, q.batch, g.Sn, p.done.first_pass, group, p.blkmax_ws);
  w.bytes = c.total();
  return w;
}

template <typename T>
void launch_gather(const GatherArgs* ga, int batch, bool own_mean, double* part,
                   hipStream_t st) {
  if (!part) {
    hipLaunchKernelGGL(gather_kernel<T>, dim3(batch, 2), dim3(kBlock), 0, st, ga[0], ga[1]);
    return;
  }
  const dim3 grid(kGatherChunks, batch, 2);
  if (own_mean)
    hipLaunchKernelGGL((gather_big_kernel<T, 0>), grid, dim3(kBlock), 0, st, ga[0], ga[1], part);
  hipLaunchKernelGGL((gather_big_kernel<T, 1>), grid, dim3(kBlock), 0, st, ga[0], ga[1], part);
}

int gather_patches(const XcorrPlan& p, const SfmXcorrDesc* d, const XcorrWs& w,
                   hipStream_t st) {
  const Geo& g = p.g;
  GatherArgs ga[2];
  for (int k = 0; k < 2; ++k) {
    GatherArgs& a = ga[k];
    a.img = k == 0 ? d->pre_image : d->post_image;
    a.mask = k == 0 ? d->pre_mask : d->post_mask;
    for (int i = 0; i < 3; ++i) {
      a.ishape[i] = k == 0 ? d->pre_shape[i] : d->post_shape[i];
      a.mshape[i] = k == 0 ? d->pre_mask_shape[i] : d->post_mask_shape[i];
      a.psz[i] = k == 0 ? g.P[i] : g.Q[i];
      if (a.mask && a.mshape[i] < a.psz[i])
        return sfm::fail(SFM_ERR_INVALID, "mask smaller than patch on axis %d", i);
    }
    a.starts = k == 0 ? d->pre_starts : d->post_starts;
    a.nd = d->ndim;
    a.use_mean = d->use_mean;
    a.mean = d->mean;
    a.out = k == 0 ? w.a0 : w.b0;
    a.valid = p.masked ? (k == 0 ? w.va : w.vb) : nullptr;
    a.pn = k == 0 ? g.Pn : g.Qn;
  }
  if (d->dtype == SFM_DTYPE_U8)
    launch_gather<unsigned char>(ga, d->batch, !d->use_mean, w.gather_part, st);
  else
    launch_gather<float>(ga, d->batch, !d->use_mean, w.gather_part, st);
  SFM_LAUNCH_CHECK();
  if ((long long)d->batch * g.S[0] > 65535LL * 32768)
    return sfm::fail(SFM_ERR_INVALID, "batch * S_z too large");
  // the masked correlation accumulates the batch maxima for masked_finalize
  if (p.masked) SFM_HIP_CHECK(hipMemsetAsync(w.maxima, 0, 2 * sizeof(unsigned int), st));
  return SFM_OK;
}

// Padfield normalisation of a gathered (direct / FFT) surface.
int masked_finalize(const XcorrWs& w, float* surface, long long n, hipStream_t st) {
  const int grid = static_cast<int>(std::min<long long>((n + kBlock - 1) / kBlock, 4096));
  hipLaunchKernelGGL(masked_finalize_kernel, dim3(grid), dim3(kBlock), 0, st, surface,
                     w.den, w.ov, w.maxima, n);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

// `d`: the rows of this round (sub_desc).
int compute_surface(const XcorrPlan& p, const SfmXcorrDesc* d, const XcorrWs& w,
                    float* surface, const sfm::FusedPeaks* fused, unsigned int* smax) {
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const Geo& g = p.g;
  switch (p.path) {
    case Path::MfmaMasked:
      // exact integer correlations on the matrix cores + Padfield assembly
      return sfm::mfma_i8_masked(d, w.mfma, surface, w.maxima, smax, w.peaks.blkmax);
    case Path::Mfma:
      return sfm::mfma_i8_surface(d, w.mfma, surface, fused);
    case Path::Fft: {
      if (int rc = gather_patches(p, d, w, st)) return rc;
      sfm::prof_begin(sfm::kProfXcorr, st);
      const int rc = sfm::fft_correlate(d, w.a0, w.b0, w.va, w.vb, surface, w.den, w.ov,
                                        w.maxima, w.fft, smax);
      sfm::prof_end(sfm::kProfXcorr, st);
      if (rc) return rc;
      break;
    }
    case Path::Direct: {
      if (int rc = gather_patches(p, d, w, st)) return rc;
      const CorrArgs c = {w.a0, w.b0, w.va, w.vb, g, surface, w.den, w.ov, w.maxima};
      const dim3 grid((g.S[2] + 63) / 64, (g.S[1] + 3) / 4,
                      (unsigned)((long long)d->batch * g.S[0]));  // bounded by gather_patches
      if (p.masked) {
        hipLaunchKernelGGL(corr_direct_kernel<true>, grid, dim3(kBlock), 0, st, c);
      } else {
        sfm::prof_begin(sfm::kProfXcorr, st);
        hipLaunchKernelGGL(corr_direct_kernel<false>, grid, dim3(kBlock), 0, st, c);
        sfm::prof_end(sfm::kProfXcorr, st);
      }
      SFM_LAUNCH_CHECK();
      break;
    }
  }
  return p.masked ? masked_finalize(w, surface, (long long)d->batch * g.Sn, st) : SFM_OK;
}

int surface_round(const XcorrPlan& p, long long off, long long rows, float* surface) {
  const SfmXcorrDesc sub = sub_desc(p, off, rows);
  const XcorrWs w = carve_xcorr(p, rows, p.group, sub.workspace);
  if (int rc = check_workspace("xcorr", sub.workspace, sub.workspace_bytes, w.bytes)) return rc;
  if (!p.mfma) return compute_surface(p, &sub, w, surface, nullptr, nullptr);
  if (int rc = compute_surface(p, &sub, w, w.surface, nullptr, nullptr)) return rc;
  hipLaunchKernelGGL(compact_surface_kernel, dim3(64, sub.batch), dim3(kBlock), 0,
                     static_cast<hipStream_t>(sub.stream), w.surface, surface, p.g.S[1],
                     p.g.S[2], w.srows, w.spitch);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int peaks_round(const XcorrPlan& p, long long off, long long rows, float* peaks) {
  const SfmXcorrDesc sub = sub_desc(p, off, rows);
  const Geo& g = p.g;
  hipStream_t st = static_cast<hipStream_t>(sub.stream);
  const XcorrWs w = carve_xcorr(p, rows, p.group, sub.workspace);
  if (int rc = check_workspace("xcorr", sub.workspace, sub.workspace_bytes, w.bytes)) return rc;
  const PeakDone& done = p.done;
  if (done.first_pass || done.smax)
    if (int rc = clear_peak_state(w.peaks, st)) return rc;
  if (int rc = compute_surface(p, &sub, w, w.surface, done.first_pass ? &w.peaks.f : nullptr,
                               done.smax ? w.peaks.smax : nullptr))
    return rc;
  float center[3];
  for (int i = 0; i < 3; ++i)
    center[i] = static_cast<float>((g.P[i] + g.Q[i]) / 2 - 1);
  PeakArgs pa = make_peak_args(
      w.peaks,
      {w.surface, g.nd, g.S, g.Sn, w.spitch, (long long)w.srows * w.spitch, sub.batch},
      sub, center, peaks);
  if (p.path == Path::MfmaMasked) {
    // rows below the overlap threshold are zeros (the assembly's second maximum,
    // `maxima[1]`, is the batch maximum of the overlap)
    if (p.live_rows) pa.live_ovmax = w.maxima + 1;
    pa.live_py = g.P[1];
    pa.live_qy = g.Q[1];
    pa.live_qx = g.Q[2];
    if (p.blkmax) pa.blkmax = w.peaks.blkmax;
  }
  return run_peaks(pa, done, w.peaks, st);
}

}  // namespace

extern "C" {

size_t sfm_xcorr_workspace_bytes(const SfmXcorrDesc* d) {
  XcorrPlan p;
  if (make_plan(d, Entry::Size, nullptr, &p) != SFM_OK) return 0;  // message in sfm_last_error
  return carve_xcorr(p, p.round, p.group, nullptr).bytes;
}

int sfm_xcorr_surface(const SfmXcorrDesc* d, float* surface) {
  XcorrPlan p;
  if (int rc = make_plan(d, Entry::Surface, surface, &p)) return rc;
  // masked surfaces are normalised with maxima over their reference batch
  for (long long off = 0; off < d->batch; off += p.round)
    if (int rc = surface_round(p, off, std::min<long long>(p.round, d->batch - off),
                               surface + off * p.g.Sn))
      return rc;
  return SFM_OK;
}

int sfm_xcorr_peaks(const SfmXcorrDesc* d, float* peaks) {
  XcorrPlan p;
  if (int rc = make_plan(d, Entry::Peaks, peaks, &p)) return rc;
  for (long long off = 0; off < d->batch; off += p.round)
    if (int rc = peaks_round(p, off, std::min<long long>(p.round, d->batch - off),
                             peaks + off * (p.g.nd + 2)))
      return rc;
  return SFM_OK;
}

int sfm_mask_patch_counts(const SfmMaskCountDesc* d, int32_t* counts) {
  if (!d || !d->mask || !counts)
    return sfm::fail(SFM_ERR_INVALID, "mask counts: NULL argument");
  if (d->ndim != 2 && d->ndim != 3)
    return sfm::fail(SFM_ERR_INVALID, "mask counts: ndim must be 2 or 3");
  MaskCountArgs a;
  a.mask = d->mask;
  a.out = counts;
  long long n = 1;
  for (int i = 0; i < 3; ++i) {
    a.S[i] = d->shape[i];
    a.P[i] = d->patch[i];
    a.T[i] = d->step[i];
    if (a.P[i] < 1 || a.T[i] < 1 || a.S[i] < a.P[i])
      return sfm::fail(SFM_ERR_INVALID, "mask counts: bad geometry on axis %d", i);
    a.O[i] = (a.S[i] - a.P[i]) / a.T[i] + 1;
    n *= a.O[i];
  }
  if (n > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "mask counts: grid too large");
  if (a.P[2] <= kMcCols / 2 && a.O[1] <= 65535 && a.O[0] <= 65535) {
    const int ot = (kMcCols - a.P[2]) / a.T[2] + 1;  // x outputs per tile
    const int tiles = (a.O[2] + ot - 1) / ot;
    const long long wgs = (long long)tiles * a.O[1] * a.O[0];
    const long long rows = (long long)a.P[0] * a.P[1];
    int splits = 1;
    if (wgs < 512)  // not enough workgroups to fill the chip: divide the window rows
      splits = static_cast<int>(std::max<long long>(
          1, std::min<long long>((1024 + wgs - 1) / wgs, (rows + 31) / 32)));
    hipStream_t st = static_cast<hipStream_t>(d->stream);
    if (splits > 1) SFM_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), st));
    const dim3 grid(tiles * splits, a.O[1], a.O[0]);
    hipLaunchKernelGGL(mask_count_rows_kernel, grid, dim3(kBlock), 0, st, a, ot, splits);
  } else if (n <= 65535) {
    hipStream_t st = static_cast<hipStream_t>(d->stream);
    const int nseg = (a.P[2] + kMcCols - 1) / kMcCols;
    const long long rows = (long long)a.P[0] * a.P[1];
    const long long wgs = n * nseg;
    const int splits = static_cast<int>(std::max<long long>(
        1, std::min<long long>((1024 + wgs - 1) / wgs, (rows + 31) / 32)));
    SFM_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)n * sizeof(int32_t), st));
    hipLaunchKernelGGL(mask_count_wide_kernel, dim3(nseg * splits, static_cast<unsigned>(n)),
                       dim3(kBlock), 0, st, a, nseg, splits);
  } else {
    hipLaunchKernelGGL(mask_count_kernel, dim3(static_cast<unsigned>(n)), dim3(kBlock),
                       0, static_cast<hipStream_t>(d->stream), a);
  }
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

size_t sfm_peaks_workspace_bytes(const SfmPeaksDesc* d) {
  if (!d || d->batch < 1) return 0;
  long long sn = 1;
  for (int i = 0; i < 3; ++i) sn *= d->shape[i];
  sfm::Carver c(nullptr);
  return carve_peaks(c, d->batch, sn).bytes;
}

int sfm_peaks(const SfmPeaksDesc* d, float* peaks) {
  if (!d || !peaks || !d->surface)
    return sfm::fail(SFM_ERR_INVALID, "desc / surface / peaks is NULL");
  if (d->ndim != 2 && d->ndim != 3)
    return sfm::fail(SFM_ERR_INVALID, "ndim must be 2 or 3");
  if (d->batch < 1) return sfm::fail(SFM_ERR_INVALID, "batch must be >= 1");
  long long sn = 1;
  for (int i = 0; i < 3; ++i) {
    if (d->shape[i] < 1) return sfm::fail(SFM_ERR_INVALID, "bad surface shape");
    sn *= d->shape[i];
  }
  if (sn > 0x7fffffffLL)
    return sfm::fail(SFM_ERR_INVALID, "surface too large for int32 indices");
  if (d->min_distance < 0)
    return sfm::fail(SFM_ERR_INVALID, "min_distance must be >= 0, got %d", d->min_distance);
  for (int i = 3 - d->ndim; i < 3; ++i)
    if (d->peak_radius[i] < 0)
      return sfm::fail(SFM_ERR_INVALID, "peak_radius must be >= 0, got %d", d->peak_radius[i]);
  sfm::Carver c(d->workspace);
  const PeakWs w = carve_peaks(c, d->batch, sn);
  if (int rc = check_workspace("peaks", d->workspace, d->workspace_bytes, w.bytes)) return rc;
  const PeakArgs p = make_peak_args(
      w, {d->surface, d->ndim, d->shape, sn, d->shape[2], sn, d->batch}, *d,
      d->center_offset, peaks);
  // caller-supplied surfaces may hold NaN: the only entry that asks for the
  // NaN-propagating surface maximum
  PeakDone done = {};
  done.nans = true;
  return run_peaks(p, done, w, static_cast<hipStream_t>(d->stream));
}

}  // extern "C"
