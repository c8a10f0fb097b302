// Matrix-core correlation path (overview and list of units: sfm_mfma.h).
// This header holds the correlation kernel xcorr_mfma_kernel<NCA, NCE, MODE> and its launch
// templates.  It is included by the geometry units sfm_mfma_g<NCA>x<NCE>.hip, each of which
// instantiates launch_variant for one entry of SFM_MFMA_GEOMETRIES; sfm_mfma.h lists the
// other units of the path.
#ifndef SFM_MFMA_KERNEL_H_
#define SFM_MFMA_KERNEL_H_

#include "sfm_mfma.h"

#include <algorithm>
#include <type_traits>

namespace sfm {
namespace mfma {
namespace {

__device__ __forceinline__ unsigned load_u32_guarded(const unsigned* base,
                                                     long long idx,
                                                     long long n_words) {
  return (idx >= 0 && idx < n_words) ? base[idx] : 0u;
}

// ---------------------------------------------------------------------------
// main kernel
// ---------------------------------------------------------------------------
// Loads the pre and the post patch into LDS as int8 (pixel - centre), 16 bytes
// per work item, from arbitrarily aligned global rows.  The aligned dword
// loads of BOTH patches are issued before anything is consumed (kStageBatch
// items per thread and plane cover a 160 x 160 patch in one round), so a
// patch costs one global-memory round trip.
struct StagePlane {
  const unsigned char* img;
  long long img_bytes;
  int W, y0, x0, py, px, centre;
  unsigned char* dst;
  int pitch, row_off, col_off, n_chunks;
};

constexpr int kStageBatch = 7;

template <int NT = kThreads>
__device__ __forceinline__ void stage_patches(const StagePlane& p0, const StagePlane& p1,
                                              const int tid) {
  const StagePlane* pl[2] = {&p0, &p1};
  const int n_items0 = p0.py * p0.n_chunks, n_items1 = p1.py * p1.n_chunks;
  const int n_max = max(n_items0, n_items1);
  for (int item0 = tid; item0 < n_max; item0 += NT * kStageBatch) {
    v4i w[2][kStageBatch];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const StagePlane& p = *pl[s];
      const int n_items = p.py * p.n_chunks;
#pragma unroll
      for (int u = 0; u < kStageBatch; ++u) {
        const int item = min(item0 + u * NT, n_items - 1);  // extra items: ignored
        const int y = item / p.n_chunks, ch = item - y * p.n_chunks;
        const long long off = (long long)(p.y0 + y) * p.W + p.x0 + ch * 16;
        w[s][u] = load_16_bytes(p.img, off, p.img_bytes);
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const StagePlane& p = *pl[s];
      const unsigned cc = static_cast<unsigned>(p.centre) * 0x01010101u;
      const int n_items = p.py * p.n_chunks;
#pragma unroll
      for (int u = 0; u < kStageBatch; ++u) {
        const int item = item0 + u * NT;
        if (item >= n_items) break;
        const int y = item / p.n_chunks, ch = item - y * p.n_chunks;
        v4i out;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          unsigned v = static_cast<unsigned>(w[s][u][k]);
          // bytewise v - centre (mod 256) == int8 value of pixel - centre
          const unsigned H = 0x80808080u;
          v = ((v | H) - (cc & ~H)) ^ ((v ^ ~cc) & H);
          // zero bytes beyond the patch width
          const int xb = ch * 16 + k * 4;
          if (xb + 4 > p.px) {
            const int keep = p.px - xb;  // < 4
            v = keep <= 0 ? 0u : (v & (0xffffffffu >> (8 * (4 - keep))));
          }
          out[k] = static_cast<int>(v);
        }
        *reinterpret_cast<v4i*>(p.dst + (p.row_off + y) * p.pitch + p.col_off + ch * 16) =
            out;
      }
    }
  }
}

// Masked path: stages one operand plane of a patch, 16 pixels per work item,
// from arbitrarily aligned image / mask rows (aligned dword loads + funnel
// shift, several items in flight).
__device__ void stage_plane(const unsigned char* __restrict__ img, long long img_bytes,
                            int W, int y0, int x0,
                            const unsigned char* __restrict__ mask,
                            long long mask_bytes, int MW, int my0, int mx0, int py,
                            int px, int centre, int plane,
                            unsigned char* __restrict__ dst, int pitch, int row_off,
                            int col_off, int n_chunks) {
  const unsigned* iw = reinterpret_cast<const unsigned*>(img);
  const long long n_iw = (img_bytes + 3) >> 2;
  // the mask base pointer may be byte aligned: split into aligned base + shift
  const unsigned long long mbase = reinterpret_cast<unsigned long long>(mask);
  const unsigned* mw = reinterpret_cast<const unsigned*>(mbase & ~3ull);
  const long long m_lead = static_cast<long long>(mbase & 3ull);
  const long long n_mw = (mask_bytes + m_lead + 3) >> 2;
  constexpr int kBatch = 2;
  const int n_items = py * n_chunks;
  for (int item0 = threadIdx.x; item0 < n_items; item0 += kThreads * kBatch) {
    unsigned wi[kBatch][5], wm[kBatch][5], shi[kBatch], shm[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int item = item0 + u * kThreads;
      const int y = item / n_chunks, ch = item - y * n_chunks;
      const long long off = (long long)(y0 + y) * W + x0 + ch * 16;
      const long long moff = (long long)(my0 + y) * MW + mx0 + ch * 16 + m_lead;
      shi[u] = static_cast<unsigned>(off & 3);
      shm[u] = static_cast<unsigned>(moff & 3);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        wi[u][k] = item < n_items ? load_u32_guarded(iw, (off >> 2) + k, n_iw) : 0u;
        wm[u][k] = (mask && item < n_items) ? load_u32_guarded(mw, (moff >> 2) + k, n_mw)
                                            : 0u;
      }
    }
#pragma unroll
    for (int u = 0; u < kBatch; ++u) {
      const int item = item0 + u * kThreads;
      if (item >= n_items) break;
      const int y = item / n_chunks, ch = item - y * n_chunks;
      v4i out;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned pv = __builtin_amdgcn_alignbyte(wi[u][k + 1], wi[u][k], shi[u]);
        const unsigned mv = __builtin_amdgcn_alignbyte(wm[u][k + 1], wm[u][k], shm[u]);
        unsigned o = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int x = ch * 16 + k * 4 + t;
          const int ap = static_cast<int>((pv >> (8 * t)) & 0xffu) - centre;
          const bool valid = ((mv >> (8 * t)) & 0xffu) == 0 && x < px;
          const int sq = ap * ap;
          int val = plane == kPlaneVal ? ap
                    : plane == kPlaneValid ? 1
                    : plane == kPlaneSqHi ? (sq >> 7) - 64
                                          : (sq & 127);
          if (!valid) val = 0;
          o |= static_cast<unsigned>(val & 0xff) << (8 * t);
        }
        out[k] = static_cast<int>(o);
      }
      *reinterpret_cast<v4i*>(dst + (row_off + y) * pitch + col_off + ch * 16) = out;
    }
  }
}

// Inclusive add scan over the 16 lanes of a DPP row (the 16 columns of a tile).
__device__ __forceinline__ int row16_scan_incl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
  return v;
}
// Lane 15 of every 16-lane row to the whole row (ds_swizzle, bit mode: lane' =
// (lane & 0x10) | 0x0f inside each half wave; no LDS memory is touched).
__device__ __forceinline__ int row16_last(int v) {
  return __builtin_amdgcn_ds_swizzle(v, (0x0f << 5) | 0x10);
}
// Lane n <- lane 15 - n of the same row.
__device__ __forceinline__ int row16_mirror(int v) {
  return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);   // row_mirror
}

// Wave-wide maximum of non-negative values on the DPP network (no LDS round
// trips): row shifts inside each 16-lane row, then row broadcasts; the result
// is read from lane 63 into a scalar.
#define SFM_DPP_MAXF(x, ctrl, rmask, bc)                                            \
  fmaxf(x, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl,   \
                                                      rmask, 0xf, bc)))
__device__ __forceinline__ float wave_max_nonneg(float v) {
  v = SFM_DPP_MAXF(v, 0x111, 0xf, true);   // row_shr:1
  v = SFM_DPP_MAXF(v, 0x112, 0xf, true);   // row_shr:2
  v = SFM_DPP_MAXF(v, 0x114, 0xf, true);   // row_shr:4
  v = SFM_DPP_MAXF(v, 0x118, 0xf, true);   // row_shr:8
  v = SFM_DPP_MAXF(v, 0x142, 0xa, false);  // row_bcast:15
  v = SFM_DPP_MAXF(v, 0x143, 0xc, false);  // row_bcast:31
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// The same for non-negative integers (six DPP steps on the VALU; the shuffle
// form of the reduction is six dependent LDS round trips, next to the matrix
// loops' fragment reads).
#define SFM_DPP_MAXI(x, ctrl, rmask, bc) \
  max(x, __builtin_amdgcn_update_dpp(0, x, ctrl, rmask, 0xf, bc))
__device__ __forceinline__ int wave_max_nonneg_i(int v) {
  v = SFM_DPP_MAXI(v, 0x111, 0xf, true);   // row_shr:1
  v = SFM_DPP_MAXI(v, 0x112, 0xf, true);   // row_shr:2
  v = SFM_DPP_MAXI(v, 0x114, 0xf, true);   // row_shr:4
  v = SFM_DPP_MAXI(v, 0x118, 0xf, true);   // row_shr:8
  v = SFM_DPP_MAXI(v, 0x142, 0xa, false);  // row_bcast:15
  v = SFM_DPP_MAXI(v, 0x143, 0xc, false);  // row_bcast:31
  return __builtin_amdgcn_readlane(v, 63);
}

// Bitwise OR over the wave, the same way.
#define SFM_DPP_OR(x, ctrl, rmask, bc) \
  ((x) | __builtin_amdgcn_update_dpp(0, x, ctrl, rmask, 0xf, bc))
__device__ __forceinline__ int wave_or(int v) {
  v = SFM_DPP_OR(v, 0x111, 0xf, true);   // row_shr:1
  v = SFM_DPP_OR(v, 0x112, 0xf, true);   // row_shr:2
  v = SFM_DPP_OR(v, 0x114, 0xf, true);   // row_shr:4
  v = SFM_DPP_OR(v, 0x118, 0xf, true);   // row_shr:8
  v = SFM_DPP_OR(v, 0x142, 0xa, false);  // row_bcast:15
  v = SFM_DPP_OR(v, 0x143, 0xc, false);  // row_bcast:31
  return __builtin_amdgcn_readlane(v, 63);
}

// base[byte_off]: a 32-bit byte offset on a wave-uniform base selects the
// scalar-base + VGPR-offset addressing mode (no 64-bit VALU address math).
__device__ __forceinline__ float at_byte(const float* base, unsigned byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}

// First patch of queue ticket t (see MfmaArgs::run).
__device__ __forceinline__ int ticket_patch(const MfmaArgs& a, int t) {
  return t < a.n_runs ? t * a.run : a.run_end + (t - a.n_runs);
}

// Next patch of this workgroup; called by all threads at the end of a patch.  `left`:
// patches of the workgroup's run after b (wave-uniform).  Inside a run the next patch is
// the next index: no barrier, no atomic.
__device__ __forceinline__ int next_patch(const MfmaArgs& a, int b, int* next_lds, int& left) {
  if (!a.work_counter) return b + gridDim.x;
  if (left > 0) {
    --left;
    return b + 1;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    *next_lds = ticket_patch(a, gridDim.x + atomicAdd(a.work_counter, 1));
  __syncthreads();
  // wave-uniform: keeps every per-patch base address in scalar registers
  const int item = __builtin_amdgcn_readfirstlane(*next_lds);
  left = item < a.run_end ? a.run - 1 : 0;
  return item;
}

template <int NCA, int NCE, int MODE>
__global__ void __launch_bounds__(NCA > 10 ? kWideThreads : kThreads,
                                  NCA > 10 ? 1 : 2) xcorr_mfma_kernel(MfmaArgs a) {
  // NCA <= 10: two workgroups of four waves per CU, each on its own patch; the waves of a
  // workgroup draw the row tiles of that patch.
  // Search-window geometry (NCA > 10: pre patches 161 .. 320 wide against a post patch of up
  // to 160, processor/flow.py:577,792-803; kModeGeneral semantics, no pruning).  The pre patch
  // alone is up to 119 KB of LDS, so a CU holds ONE workgroup, see WIDE8 below.
  constexpr bool LAZYG = MODE == kModeSameExactLazyG;
  constexpr bool SAME = MODE == kModeSame || MODE == kModeSameExact || MODE == kModeSameLazy ||
                        MODE == kModeSameExactLazy || LAZYG;
  constexpr bool EXACT = MODE == kModeSameExact || MODE == kModeSameExactLazy || LAZYG;
  constexpr bool LAZY = MODE == kModeSameLazy || MODE == kModeSameExactLazy || LAZYG;
  constexpr bool RAW = MODE == kModeRaw;
  constexpr int NQ = NCA + NCE - 1;
  // Search-window variants: the CU's one workgroup
  // has EIGHT waves (two per SIMD: a partner covers a wave's fragment round trips and runs
  // its matrix loop under the other's epilogue) and a tile job is one column HALF of a row
  // tile -- NQH accumulator tiles in plain VGPRs, the 12 .. 15 A chunks that reach them.
  constexpr bool WIDE8 = NCA > 10 && MODE == kModeGeneral;
  constexpr int NQH = (NQ + 1) / 2;
  constexpr int kCq0 = NCE - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float touch_junk[kThreads];  // sink of the LDS-direct G touches
  __shared__ int probe_lds[kThreads];     // K-split sums of the seed probe (a.prune)
  unsigned char* A_lds = smem;
  unsigned char* B_lds = smem + a.a_bytes;
  float* R_lds = reinterpret_cast<float*>(smem + a.a_bytes + a.b_bytes);
  // Behind the aux arrays: the workgroup's state words (LdsTail; the raw mode has the head only).
  LdsTail* tail = reinterpret_cast<LdsTail*>(smem + a.a_bytes + a.b_bytes + a.r_bytes);
  int* pmax_lds = tail->head;   // running maximum of the current surface
  int* hot_lds = pmax_lds + 1;  // hot-list fill count of the current patch
  float* tb_lds = tail->tb;     // pruning bounds (a.prune)
  int* best_lds = tail->best;
  int* lz = tail->lz;
  float* lz_tmax = tail->lz_tmax;
  int* lz_prev = &tail->lz_prev;
  int* lz_cq = tail->lz_cq;
  int* lz_ks = tail->lz_ks;
  int* lz_rows = tail->lz_rows;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;
  const int Py = a.P[0], Px = a.P[1], Qy = a.Q[0], Qx = a.Q[1];
  const int Sy = a.S[0], Sx = a.S[1];

  const long long probe_c0 = clock64(), probe_w0 = wall_clock64();
  // Zero the whole LDS image once: pad rows / margins stay zero afterwards.
  for (int i = threadIdx.x * 16; i < a.a_bytes + a.b_bytes;
       i += (WIDE8 ? kWideThreads : kThreads) * 16)
    *reinterpret_cast<v4i*>(smem + i) = v4i{0, 0, 0, 0};

  if (SAME && (a.prune || LAZY) && threadIdx.x == 0) {
    *best_lds = (((a.Q[0] - 1) / 16) << 8) | ((a.Q[1] - 1) / 16);  // the zero shift
    best_lds[2] = 1;  // pruning events of the previous patch (optimistic start)
    best_lds[3] = 0;  // patches of this workgroup so far
    if (LAZY) {
      *lz_prev = 0;
      lz_cq[0] = NQ;
      lz_cq[1] = -1;
      lz_cq[2] = lz_cq[3] = (a.Q[1] - 1) / 16;   // the zero shift
    }
  }
  const long long bytes0 = (long long)a.ishape[0][0] * a.ishape[0][1];
  const long long bytes1 = (long long)a.ishape[1][0] * a.ishape[1][1];
  const int cq0 = NCE - 1;
  // Per-lane start of the B windows inside a padded post-patch row.
  const int pos0 = a.ml + Qx - 1 - n - 16 * cq0;
  const int sh = pos0 & 3;

#ifdef SFM_MFMA_TIMING
  const long long wstart = wall_clock64();
  const long long cstart = clock64();
  long long tph[18] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0}; long long tc = clock64(); int npat = 0;
  int run_pat[2] = {0, 0}, run_redo[2] = {0, 0}, run_seed[2] = {0, 0};  // see kRunStatWords
#define TICK(i) { long long tn = clock64(); tph[i] += tn - tc; tc = tn; }
#else
#define TICK(i)
#endif
  // Patches are handed out dynamically: the two workgroups of a CU do not run
  // at the same speed (see the priority note below) and finish whole patches
  // at different times.
  int* next_lds = hot_lds + 1;
  int tiles_drawn = 0, tiles_skipped = 0, cols_skipped = 0, tiles_early = 0;  // (wave-uniform; reported through a.clk)
  long long mfma_issued = 0;  // matrix instructions this wave issued in the row loops
  if (a.prio_mode == 3) {
    // HW_REG_LDS_ALLOC[7:0] = LDS_BASE: 0 for the first workgroup of the CU.
    const unsigned lds_base = __builtin_amdgcn_s_getreg((7 << 11) | 6) & 0xff;
    if (lds_base != 0)
      __builtin_amdgcn_s_setprio(3);
    else
      __builtin_amdgcn_s_setprio(0);
  }
  // Work items: patches, or the extra (patch, operand-plane pair) passes of
  // the masked path (see masked_classify_kernel).
  const int n_items = (RAW && a.list) ? *a.n_list : a.batch;
  // (g0, gs: first row group and stride of the calling wave; the four waves of a
  // workgroup, sums through LDS atomics, barrier, seed)
  auto seed_probe = [&](const int g0, const int gs) {
      // Seed of the running maximum.  The first tiles are drawn before any tile
      // has finished, i.e. with nothing to prune against.  So the 16 x 16 block of
      // shifts that held the previous patch's maximum is evaluated first, its
      // patch rows split over the four waves (exact integer sums S, the same
      // fragments the row loop would use), summed through LDS atomics, and
      //   max(surface) >= max(S over the block) - |correction|max =: m_lo
      // (tbound[kBoundCorr], prep kernel) goes into the running maximum.  m_lo is
      // strictly below a real element, so the final maximum is unaffected.
      const int pq = __builtin_amdgcn_readfirstlane(*best_lds);
      const int ps = pq >> 8, qs = pq & 255;
      const int pdy0 = 16 * ps - (Qy - 1);
      const int pylo = max(0, -pdy0 - 15), pyhi = min(Qy, Py - pdy0);
      const unsigned char* pap = A_lds + (kPadTop + pylo + g + pdy0 + n) * a.pa;
      const unsigned char* pbp = B_lds + (pylo + g) * a.pb + (pos0 & ~3);
      // two row groups per trip: their loads are in flight together and they
      // accumulate into separate registers (no dependent MFMA chain of 2 NCA)
      v4i pacc = v4i{0, 0, 0, 0}, pacc2 = v4i{0, 0, 0, 0};
      const int n_grp = (pyhi - pylo + 3) >> 2;
      // The pairs (ca, c) on the diagonal of column tile qs are ca = ca_lo + i,
      // c = c_lo + i, i < n_on: contiguous A chunks against a contiguous run of B
      // dwords (4 n_on + 1, shared between neighbouring fragments like in the row
      // loop).  Pairs past n_on, and groups past the tile, read A from a zero
      // padding row instead (branch-free).
      const int ca_lo = max(0, qs - cq0), c_lo = ca_lo - qs + cq0;
      const int n_on = min(NCA - ca_lo, NCE - c_lo);
      const unsigned char* zero_row = A_lds + n * a.pa;  // inside the top padding
      constexpr int kPD = 4 * NCA + 1;
      auto load_group = [&](int grp, v4i* paf, unsigned* pd) {
        const bool live = grp < n_grp;
        const int gc = min(grp, n_grp - 1);
        const unsigned char* ag = pap + 4 * gc * a.pa + 16 * ca_lo;
        const unsigned char* bg = pbp + 4 * gc * a.pb + 16 * c_lo;
#pragma unroll
        for (int i = 0; i < NCA; ++i)
          paf[i] = *reinterpret_cast<const v4i*>((live && i < n_on) ? ag + 16 * i : zero_row);
#pragma unroll
        for (int j = 0; j < kPD; ++j) pd[j] = *reinterpret_cast<const unsigned*>(bg + 4 * j);
      };
      auto mma_group = [&](const v4i* paf, const unsigned* pd, v4i& acc_out) {
#pragma unroll
        for (int i = 0; i < NCA; ++i) {
          v4i bf;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            bf[k] = static_cast<int>(
                __builtin_amdgcn_alignbyte(pd[4 * i + k + 1], pd[4 * i + k], sh));
          acc_out = __builtin_amdgcn_mfma_i32_16x16x64_i8(paf[i], bf, acc_out, 0, 0, 0);
        }
      };
      for (int grp = g0; grp < n_grp; grp += 2 * gs) {
        v4i paf[NCA], paf2[NCA];
        unsigned pd[kPD], pd2[kPD];
        load_group(grp, paf, pd);
        load_group(grp + gs, paf2, pd2);
        mma_group(paf, pd, pacc);
        mma_group(paf2, pd2, pacc2);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) pacc[r] += pacc2[r];
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(&probe_lds[r * 64 + lane], pacc[r]);
      __syncthreads();
      int sm = max(max(probe_lds[lane], probe_lds[64 + lane]),
                   max(probe_lds[128 + lane], probe_lds[192 + lane]));
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) sm = max(sm, __shfl_xor(sm, d, 64));
      const float m_lo = __int2float_rd(sm) - tb_lds[kBoundCorr];
      if (lane == 0 && m_lo > 0.f) atomicMax(pmax_lds, __float_as_int(m_lo));
  };
  // The first assignment is ticket blockIdx.x.
  const int item0 = ticket_patch(a, blockIdx.x);
  int run_left = item0 < a.run_end ? a.run - 1 : 0;
  for (int item = item0; item < n_items; item = next_patch(a, item, next_lds, run_left)) {
    int b = item;
    int plane0 = a.plane[0], plane1 = a.plane[1];
    if (RAW && a.list) {
      const int code = a.list[item], pass = code & 7;  // kMaskedPasses[pass]
      b = code >> 3;
      plane0 = pass == 1 ? kPlaneVal : pass == 4 ? kPlaneSqHi : pass == 5 ? kPlaneSqLo
                                                                          : kPlaneValid;
      plane1 = pass == 2 ? kPlaneVal : pass == 6 ? kPlaneSqHi : pass == 7 ? kPlaneSqLo
                                                                          : kPlaneValid;
    }
#ifdef SFM_MFMA_TIMING
    ++npat;
    // (runs start at multiples of a.run below a.run_end; later patches are runs of one)
    const int in_run = (item < a.run_end && item % a.run != 0) ? 1 : 0;
    const int seed_pq = SAME && (a.prune || LAZY) ? *best_lds : -1;
    ++run_pat[in_run];
#endif
    TICK(7)
    float const_a = 0.f, const_b = 0.f;
    __syncthreads();  // previous patch fully consumed / zero fill done
    TICK(0)
    const PatchParams pp = a.pp[b];
    // covers aux_n <= 192 and Py Px <= 32768 in registers; taller patches
    // take the remainder loops below
    constexpr int kAuxRegs = 3;
    float auxv[kAuxRegs];
    float tbv = 0.f;
    if (RAW) {
      stage_plane(a.img[0], bytes0, a.ishape[0][1], pp.y0[0], pp.x0[0], a.mask[0],
                  (long long)a.mshape[0][0] * a.mshape[0][1], a.mshape[0][1],
                  pp.my0[0], pp.mx0[0], Py, Px, pp.c[0], plane0, A_lds, a.pa,
                  kPadTop, 0, NCA);
      stage_plane(a.img[1], bytes1, a.ishape[1][1], pp.y0[1], pp.x0[1], a.mask[1],
                  (long long)a.mshape[1][0] * a.mshape[1][1], a.mshape[1][1],
                  pp.my0[1], pp.mx0[1], Qy, Qx, pp.c[1], plane1, B_lds, a.pb, 0,
                  a.ml, (Qx + 15) / 16);
    } else {
      // Everything staging needs from global memory is requested before the
      // first wait (the four 1-D correction arrays and the pixels of both
      // patches): loads return in order, so staging costs one round trip.
      if (SAME) {
        const float* aux = a.aux + (long long)b * (4 * a.aux_n + 4);
#pragma unroll
        for (int k = 0; k < kAuxRegs; ++k) {
          const int i = threadIdx.x + k * kThreads;
          auxv[k] = i < 4 * a.aux_n ? aux[i] : 0.f;
        }
        const_a = aux[4 * a.aux_n + 0];
        const_b = aux[4 * a.aux_n + 1];
        // (unconditional: a load under a condition would be waited for on its own)
        tbv = a.tbound[(long long)b * kBoundStride + (threadIdx.x & (kBoundStride - 1))];
      }
      const StagePlane sa = {a.img[0], bytes0, a.ishape[0][1], pp.y0[0], pp.x0[0], Py, Px,
                             pp.c[0], A_lds, a.pa, kPadTop, 0, NCA};
      const StagePlane sb = {a.img[1], bytes1, a.ishape[1][1], pp.y0[1], pp.x0[1], Qy, Qx,
                             pp.c[1], B_lds, a.pb, 0, a.ml, (Qx + 15) / 16};
      stage_patches<WIDE8 ? kWideThreads : kThreads>(sa, sb, threadIdx.x);
      TICK(8)
    }
    if (threadIdx.x == 0) {
      *pmax_lds = 0;  // float bits of max(surface, 0)
      *hot_lds = 0;
      pmax_lds[3] = 0;  // tile counter of this patch
      if (LAZY) {
        // requested from the start: what the previous patch of this workgroup
        // turned out to need, and the tiles around the row tile that held its
        // maximum (flow fields are coherent; the tiles next to the peak tile are
        // drawn together with it and would otherwise finish un-stored and be
        // recomputed: measured 2.4 redone tiles per patch without any request,
        // 0.75 with the peak tile's band alone -- the peak's blob often straddles
        // two tiles, whose bands are four tiles)
        // (a prediction: the band of a tile away from the surface border, in tiles)
        const int pt = *best_lds >> 8, gt = (max(a.guard_md, a.win >> 1) + 15) >> 4;
        const int lo_t = max(pt - gt, 0), hi_t = min(pt + gt, a.n_order - 1);
        const int pv = *lz_prev;
        // (the band of the peak tile only while there is no previous need mask: the
        // mask counts the guard band in rows and is usually a tile narrower)
        lz[0] = (pv ? 0 : static_cast<int>(((2u << hi_t) - 1u) & ~((1u << lo_t) - 1u))) | pv;
        lz[1] = lz[2] = lz[3] = 0;
        if (lz_cq[1] >= lz_cq[0]) {   // (the previous patch had hot elements)
          lz_cq[2] = lz_cq[0];
          lz_cq[3] = lz_cq[1];
        }
        lz_cq[0] = NQ;
        lz_cq[1] = -1;
      }
      if (SAME && a.prune) {
        best_lds[1] = 0;  // row tiles pruned in this patch
        // The seed probe pays only where something gets pruned: it runs if the
        // previous patch of this workgroup pruned anything, and every eighth
        // patch regardless (to notice when the data improve).
        const int n_done = best_lds[3];
        best_lds[3] = n_done + 1;
        best_lds[4] = (best_lds[2] > 0 || (n_done & 7) == 0) ? 1 : 0;
        best_lds[2] = 0;
      }
    }
    if (SAME) {
#pragma unroll
      for (int k = 0; k < kAuxRegs; ++k) {
        const int i = threadIdx.x + k * kThreads;
        if (i < 4 * a.aux_n) R_lds[i] = auxv[k];
      }
      if (a.prune && threadIdx.x < kBoundStride) tb_lds[threadIdx.x] = tbv;
      if (a.prune) probe_lds[threadIdx.x] = 0;
      if (LAZY && threadIdx.x < 32) lz_ks[threadIdx.x] = 0;
      const float* aux = a.aux + (long long)b * (4 * a.aux_n + 4);
      for (int i = threadIdx.x + kAuxRegs * kThreads; i < 4 * a.aux_n; i += kThreads)
        R_lds[i] = aux[i];
    }
    TICK(9)
    __syncthreads();

    if (SAME && a.prune && a.probe && __builtin_amdgcn_readfirstlane(best_lds[4]))
      seed_probe(wave, kWaves);

    TICK(1)
    const float mua = pp.mu[0], mub = pp.mu[1];
    float muab = mua * mub;
    asm volatile("" : "+v"(muab));  // every global load so far has been consumed
    if (SAME) {
      // Pull this patch's correction table G (written by the prep kernel, by now
      // in HBM / Infinity Cache) into this XCD's L2, one touch per 64-byte line.
      // It is first needed by the epilogue of the first tile, a whole matrix
      // loop away, so the touches use the LDS-direct load path into a junk
      // area: no VGPR result, and nothing waits for them before that epilogue.
      // (The lane offset is made opaque so that the per-touch addresses are
      // scalar base + one VGPR instead of loop-invariant VGPRs that spill.)
      // (Written as inline assembly: the compiler's global_load_lds builtin does
      // not initialise M0, the LDS destination base, on this toolchain.  The
      // asm loads are invisible to the compiler's vmcnt bookkeeping, which is
      // safe because every counted wait that follows is for YOUNGER loads and
      // the counter retires in order.)
      const char* gt = LAZYG ? reinterpret_cast<const char*>(a.c16 + b * a.c16_stride)
                             : reinterpret_cast<const char*>(a.gtab + (long long)b * Py * Px);
      const unsigned junk_off = static_cast<unsigned>(reinterpret_cast<unsigned long long>(
          (__attribute__((address_space(3))) float*)touch_junk));
      constexpr int kTouches = (32768 / 16 + kThreads - 1) / kThreads;
      // opaque per patch: otherwise the eight lane addresses are hoisted out of
      // the patch loop as 16 VGPRs and spilled
      unsigned lane_off;
      asm volatile("v_lshlrev_b32 %0, 6, %1" : "=v"(lane_off) : "v"(threadIdx.x));
      // Lazy modes: the epilogue runs on the few tiles that may be hot or are asked
      // for, so only the table rows of the tiles requested at this point are pulled
      // (row yv serves the shifts dy = yv and dy = yv - Py: two row tiles); a tile
      // that turns out hot without having been predicted takes its L2 misses.
      const int req_now = LAZY ? *const_cast<volatile int*>(&lz[0]) : -1;
#pragma unroll
      for (int k = 0; k < kTouches; ++k) {
        const int i = (threadIdx.x + k * kThreads) * 16;
        bool wanted = i < Py * Px;
        // (the column-sum tables the table rows are built from: all of them)
        if (LAZYG) wanted = i < 2 * ((Py >> 4) + 1) * Px + Py + 1;
        if (!LAZYG && LAZY && a.prune && !a.touch_all) {
          const int yv = min(i / Px, Py - 1), yv2 = min((i + 15) / Px, Py - 1);   // (a line may straddle two rows)
          const unsigned t_mask = (1u << ((yv + Py - 1) >> 4)) | (1u << (max(yv - 1, 0) >> 4)) |
                                  (1u << ((yv2 + Py - 1) >> 4)) | (1u << (max(yv2 - 1, 0) >> 4));
          wanted = wanted && (t_mask & static_cast<unsigned>(req_now)) != 0;
        }
        if (wanted) {
          const char* src = gt + (size_t)k * kThreads * 64 + lane_off;
          unsigned saved_m0;  // M0 is the LDS base of the load; put it back
          asm volatile(
              "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
              "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
              : "=&s"(saved_m0)
              : "v"(src), "s"(junk_off)
              : "memory");
        }
      }
    }
    const int* IA = (SAME || RAW) ? nullptr : a.integ[0] + b * a.integ_stride[0];
    const int* IB = (SAME || RAW) ? nullptr : a.integ[1] + b * a.integ_stride[1];
    const float* G = SAME ? a.gtab + (long long)b * Py * Px : nullptr;
    float* surf = a.surface + b * a.s_stride;

    bool redo_phase = false;   // LAZY: the patch's tiles are finished, recompute what was missed
    for (;;) {
      int ti = 0, p = 0;
      bool forced = false;
      if (!redo_phase) {
        if (lane == 0) ti = atomicAdd(pmax_lds + 3, 1);
        ti = __builtin_amdgcn_readfirstlane(ti);
        if (ti >= a.n_order) {
          if (!LAZY) break;
          __syncthreads();   // (once per wave and patch) every tile is finished: the redo set is final
          redo_phase = true;
        } else {
          p = __builtin_amdgcn_readfirstlane(a.order[ti]);
        }
      }
      int half = 0;   // WIDE8: which column half of row tile p this job is
      if constexpr (WIDE8) {
        half = p >> 8;
        p &= 255;
      }
      if (LAZY && redo_phase) {
        // What has to be in memory, now that the maximum is final: the tiles that
        // hold an element above threshold_rel x the maximum and their guard bands.
        // The former stored themselves (the running maximum they were judged by
        // was not larger); of the latter, those that finished before anybody asked
        // are recomputed -- every wave forms the same set and claims its share.
        const float thr_f = a.threshold_rel * __int_as_float(*const_cast<volatile int*>(pmax_lds));
        const int done = *const_cast<volatile int*>(&lz[1]);
        // (one tile per lane: as loops over the tiles these were forty dependent LDS
        // round trips per wave and patch, under the fragment traffic of the other
        // workgroup's matrix loops)
        const int t_l = min(lane, 30);
        const bool mine = lane < a.n_order && ((done >> lane) & 1);
        const float tm_l = lz_tmax[t_l];
        const int rr_l = lz_rows[t_l], ks_l = lz_ks[t_l];
        const int hq_lo = *const_cast<volatile int*>(&lz_cq[0]);
        const int hq_hi = *const_cast<volatile int*>(&lz_cq[1]);
        int mask_l = 0;
        if (mine && tm_l > thr_f) {
          // (the band is counted in rows from the tile's hot rows, and is what the
          // peak kernels can read on their account: need_tiles)
          int lo_t, hi_t;
          need_tiles(a, 16 * t_l + (rr_l & 255), 16 * t_l + (rr_l >> 8), &lo_t, &hi_t);
          mask_l = static_cast<int>(((2u << hi_t) - 1u) & ~((1u << lo_t) - 1u));
        }
        const int need = wave_or(mask_l);
        if (lane == 0) *lz_prev = need;   // (every wave writes the same value)
        // stored tiles that dropped column tiles in flight and turn out to have a
        // possibly hot column (of any row tile) within a tile of what they dropped:
        // recomputed in full like the band tiles that finished un-stored
        const int bad = static_cast<int>(__ballot(mine && hq_hi >= hq_lo && ks_l > 0 &&
                                                  (hq_lo < ks_l + 1 || hq_hi > NQ - 2 - ks_l)));
        int todo = need & done & (~*const_cast<volatile int*>(&lz[2]) | bad) &
                   ~*const_cast<volatile int*>(&lz[3]);
        todo = __builtin_amdgcn_readfirstlane(todo);
        if (todo == 0) break;
        p = __builtin_ctz(todo);
        int old = 0;
        if (lane == 0) old = atomicOr(&lz[3], 1 << p);
        old = __builtin_amdgcn_readfirstlane(old);
        if ((old >> p) & 1) continue;   // another wave took it
        forced = true;
#ifdef SFM_MFMA_TIMING
        ++run_redo[in_run];
#endif
      }
      // (the tile's body is a block of its own: a `continue` inside it ends the tile; the
      // same code without the block gets another block layout and register allocation)
      do {
      // The two workgroups of a CU share each SIMD's MFMA pipe, and the issue
      // arbiter always favours the older wave: the younger workgroup would
      // run ~25 % slower and finish long after its partner.  Alternating the
      // priority per tile (opposite phase for the second dispatch wave of
      // workgroups) evens the two out.
      if (a.prio_mode == 1) {
        if ((ti & 1) ^ (blockIdx.x >= (gridDim.x >> 1) ? 1 : 0))
          __builtin_amdgcn_s_setprio(1);
        else
          __builtin_amdgcn_s_setprio(0);
      } else if (a.prio_mode == 2) {
        if (blockIdx.x >= (gridDim.x >> 1))
          __builtin_amdgcn_s_setprio(1);
        else
          __builtin_amdgcn_s_setprio(0);
      }
      int raw_col_skip = 0;
      if (RAW && a.ov_lb) {
        // largest ny = overlap rows of a shift in this tile (ny rises to min(Py, Qy)
        // at dy in [0, Py - Qy] and falls): at the tile's row nearest that range
        const int ky0 = 16 * p, ky1 = min(16 * p + 15, Sy - 1);
        const int dyc = min(max(min(max(0, ky0 - (Qy - 1)), Py - Qy), ky0 - (Qy - 1)), ky1 - (Qy - 1));
        const int ny_max = min(Py, Qy + dyc) - max(0, dyc);
        const int lb = __builtin_amdgcn_readfirstlane(a.ov_lb[b / a.ov_group]);
        const float ov_thr = 0.3f * static_cast<float>(lb);
        if (static_cast<float>(ny_max * Qx) < ov_thr) continue;
        // the same along x: outer column tiles whose widest overlap nx, times
        // ny_max, stays below the threshold are zeroed as well (row-loop variants)
        auto cols_dead = [&](int ks) {
          if (ks <= 0) return false;
          auto nx_at = [&](int kx) {
            const int dx = kx - (Qx - 1);
            return kx < Sx ? min(Px, Qx + dx) - max(0, dx) : 0;
          };
          const int nx_max = max(nx_at(16 * ks - 1), nx_at(16 * (NQ - ks)));
          return static_cast<float>(ny_max * nx_max) < ov_thr;
        };
        raw_col_skip = cols_dead(col_skip_3(NQ))   ? col_skip_3(NQ)
                       : cols_dead(col_skip_2(NQ)) ? col_skip_2(NQ)
                       : cols_dead(col_skip_hi(NQ)) ? col_skip_hi(NQ)
                       : cols_dead(col_skip_lo(NQ)) ? col_skip_lo(NQ)
                                                    : 0;
      }
      int col_skip = raw_col_skip;  // outer column tiles (each side) this tile leaves out
      // (lazy modes) read with the pruning bounds, used by the test in front of the row loop
      unsigned hd_ea = 0, hd_eb = 0;
      float hd_corr = 0.f, hd_thr = 0.f;
      int hd_req = 0, hd_cq = 0;
      if (SAME && a.prune && !forced) {
        // Exact pruning.  Every element of this tile and of the tile_guard(p) rows
        // around it is bounded by tb (prep kernel).  If tb < threshold_rel x (the
        // running maximum, which never exceeds the final one), none of them is
        // the maximum or a peak candidate, so no row of the tile is inside a
        // candidate's max-filter window (min_distance <= tile_guard) or inside the
        // first peak's sharpness window (a window centred on its peak reaches
        // peak_radius <= tile_guard rows; one pushed back inside the surface covers
        // only the tiles that keep the full 2 peak_radius): the tile is never read
        // for its values.  It is not stored at all; the overflow fall-backs of the
        // peak kernels, which sweep whole surfaces, get the set of pruned tiles
        // (a.skipmask) and skip / zero them.
        // (everything the decisions of this tile read from LDS is requested here, in
        // one round: under the fragment traffic of eight waves a dependent LDS read
        // costs several hundred cycles, and the tests below were six of them in a row)
        const int mrun_bits = *const_cast<volatile int*>(pmax_lds);
        const float tb_p = tb_lds[p], tb_c0 = tb_lds[kBoundTiles + 0], tb_c1 = tb_lds[kBoundTiles + 1];
        const float tb_2a = tb_lds[32 + 3 * p + 0], tb_2b = tb_lds[32 + 3 * p + 1];
        const float tb_2c = tb_lds[32 + 3 * p + 2];
        if (LAZY) {
          const int dy0h = 16 * p - (Qy - 1);
          const int yloh = max(0, -dy0h - 15), yhih = min(Qy, Py - dy0h);
          const unsigned* rp = reinterpret_cast<const unsigned*>(tb_lds + kRowPre);
          const int a_lo = max(0, yloh + dy0h), a_hi = min(Py, yhih + dy0h + 15);
          hd_ea = rp[(a_hi + 3) >> 2] - rp[a_lo >> 2];
          hd_eb = rp[64 + ((yhih + 3) >> 2)] - rp[64 + (yloh >> 2)];
          hd_corr = tb_lds[kBoundCorr];
          hd_req = *const_cast<volatile int*>(&lz[0]);
          hd_cq = min(lz_cq[2], NQ - 1 - lz_cq[3]);
        }
        const float mrun = __int_as_float(__builtin_amdgcn_readfirstlane(mrun_bits));
        hd_thr = a.threshold_rel * mrun;
        ++tiles_drawn;
        if (tb_p < a.threshold_rel * mrun) {
          ++tiles_skipped;
          if (lane == 0) {
            atomicOr(&best_lds[1], 1 << p);
            best_lds[2] = 1;  // (benign race: any non-zero value)
          }
          continue;
        }
        // Along x the same argument holds for the outer column tiles (bounds of
        // the outermost kKs1 / kKs2 tiles on either side, widened by the
        // guard): the row loop below has variants that leave them out.
        const float t = a.threshold_rel * mrun;
        if (tb_c0 < t) col_skip = col_skip_lo(NQ);
        if (tb_c1 < t) col_skip = col_skip_hi(NQ);
        // this row tile with fewer columns still (2-D block bounds; each already
        // capped by the 1-D column bound of its variant)
        if (tb_2a < t) col_skip = max(col_skip, col_skip_hi(NQ));
        if (tb_2b < t) col_skip = max(col_skip, col_skip_2(NQ));
        if (tb_2c < t) col_skip = max(col_skip, col_skip_3(NQ));
        cols_skipped += 2 * col_skip;
        if (col_skip > 0 && lane == 0) best_lds[2] = 1;
      }
      const int dy0 = 16 * p - (Qy - 1);
      const int ylo = max(0, -dy0 - 15);
      const int yhi = min(Qy, Py - dy0);
      if constexpr (NCA > 10 && MODE == kModeGeneral) {
        // Search-window variants: the rows of the two integral images this tile's epilogue
        // will gather from (written by the prep launch: in HBM by now) are pulled towards
        // this XCD's L2 while the matrix loop runs -- LDS-direct loads into a junk area,
        // no register result, nothing waits for them.  For the 16 shifts dy of the tile
        // the epilogue reads the rows ya0 = max(0, dy) and ya1 = min(Py, Qy + dy) of IA and
        // the rows ya0 - dy, ya1 - dy of IB: four runs of at most 16 consecutive rows.
        const int dlo = dy0, dhi = min(dy0 + 15, Sy - 1 - (Qy - 1));
        const unsigned junk_off = static_cast<unsigned>(reinterpret_cast<unsigned long long>(
            (__attribute__((address_space(3))) float*)touch_junk));
        auto touch_rows = [&](const int* tab, int ipitch, int row_lo, int row_hi) {
          const char* base = reinterpret_cast<const char*>(tab + (long long)row_lo * ipitch);
          const int n_lines = ((row_hi - row_lo + 1) * ipitch * 4 + 63) >> 6;
          for (int k = lane; k < n_lines; k += 64) {
            const char* src = base + (size_t)k * 64;
            unsigned saved_m0;
            asm volatile(
                "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                "global_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                : "=&s"(saved_m0)
                : "v"(src), "s"(junk_off)
                : "memory");
          }
        };
        const int* IAt = a.integ[0] + b * a.integ_stride[0];
        const int* IBt = a.integ[1] + b * a.integ_stride[1];
        const int a0lo = max(0, dlo), a0hi = max(0, dhi);
        const int a1lo = min(Py, Qy + dlo), a1hi = min(Py, Qy + dhi);
        if (a0hi > 0) touch_rows(IAt, Px + 1, a0lo, a0hi);        // (row 0 is all zero: one line)
        touch_rows(IAt, Px + 1, a1lo, a1hi);
        const int b0lo = min(a0lo - dlo, a0hi - dhi), b0hi = max(a0lo - dlo, a0hi - dhi);
        const int b1lo = min(a1lo - dlo, a1hi - dhi), b1hi = max(a1lo - dlo, a1hi - dhi);
        if (b0hi > 0) touch_rows(IBt, Qx + 1, b0lo, b0hi);
        touch_rows(IBt, Qx + 1, b1lo, b1hi);
      }
      v4i acc[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[q] = v4i{0, 0, 0, 0};
      const bool chk_early = LAZY && a.early > 0 && a.prune && !forced;
      bool abandoned = false;   // (lazy modes) given up inside the row loop: see check_after
      bool narrowed = false;    // (lazy modes) column tiles dropped inside the row loop
      int yb0 = ylo, y_checked = -1;   // row-loop position (shared by the loop variants)
      int y_next = ylo;                // row of the next in-loop test (see check_after)
      // widest narrowing the previous patch's hot column tiles allow (one tile of margin)
      int kmax_pred = 0;
      if (LAZY && chk_early && a.narrow && a.guard_x <= 16)
        kmax_pred = min(__builtin_amdgcn_readfirstlane(hd_cq) - 1, a.narrow);

      const unsigned char* ap =
          A_lds + (kPadTop + ylo + g + dy0 + n) * a.pa;
      const unsigned char* bp = B_lds + (ylo + g) * a.pb + (pos0 & ~3);
      // One row group of the general mode with up to ten A chunks: the B dwords are
      // read, funnel-shifted into NCE fragments and each used against every A chunk.
      auto row_group = [&](const v4i* af, const unsigned char* bp_cur) {
        unsigned d[4 * NCE + 1];
#pragma unroll
        for (int j = 0; j < 4 * NCE + 1; ++j)
          d[j] = *reinterpret_cast<const unsigned*>(bp_cur + 4 * j);
        // (one read of the caller's array per chunk)
        v4i afl[NCA];
#pragma unroll
        for (int ca = 0; ca < NCA; ++ca) afl[ca] = af[ca];
#pragma unroll
        for (int c = 0; c < NCE; ++c) {
          v4i bf;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            bf[k] = static_cast<int>(
                __builtin_amdgcn_alignbyte(d[4 * c + k + 1], d[4 * c + k], sh));
#pragma unroll
          for (int ca = 0; ca < NCA; ++ca) {
            const int q = ca - c + cq0;
            acc[q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(afl[ca], bf, acc[q], 0,
                                                           0, 0);
          }
        }
      };
      // (the general P != Q epilogue needs the registers: old order there)
      if constexpr (MODE != kModeGeneral) {
        // Software-pipelined order: A chunk outer, B fragment inner.  All NCE B
        // fragments of the row group stay in registers (4 NCE VGPRs) and every A
        // fragment is reloaded IN PLACE for the next row group right after its
        // last MFMA has been issued; the B dwords of the next group arrive in
        // small batches between the A chunks and are funnel-shifted into the
        // fragment registers behind the last chunk's MFMAs.  Nothing is waited
        // for at the loop head: the matrix pipe never drains between row
        // groups, even when the wave is alone on its SIMD.  (The prefetches of
        // the last group read up to 4 rows past the tile: inside the
        // workgroup's LDS, never used.)
        constexpr int kND = 4 * NCE + 1;
        constexpr int kPerCa = (kND + NCA - 2) / (NCA - 1);  // dwords fetched per chunk
        // A fragments live in a rotating window of kW register sets: chunk ca
        // uses set ca % kW and, once its MFMAs are issued, the set is reloaded
        // with the chunk kW positions ahead (of this row group or the next).
        constexpr int kW = (NCA > 6 && NCA % 2 == 0) ? NCA / 2 : NCA;
        static_assert(NCA % kW == 0, "window must divide the chunk count");
        // The row loop exists in up to three variants: KS outer column tiles on
        // either side are left out (exact pruning along x, see col_skip below).
        // Cold before it is finished (lazy modes).  After the patch rows yb < y the
        // accumulators hold exact partial sums; what the rows y .. yhi - 1 can still
        // add to any element of the tile is at most
        //   sqrt(E_A(rows y + dy0 .. yhi + dy0 + 14) E_B(rows y .. yhi - 1))
        // (Cauchy-Schwarz over the remaining operand bytes, whole rows: shifts and
        // the column window only shrink the sums; rows outside a patch are zero
        // padding) -- integer row energies about the operand centres from the prep
        // kernel (tb_lds[kRowPre ...], every fourth row, rounded outwards).  With the
        // bound of the mean correction added, a tile whose every element stays below
        // threshold_rel x the running maximum is exactly what the test behind the
        // loop calls cold: not hot, not a maximum, and -- unless requested -- never
        // read.  It is abandoned here, with the rest of its row loop unissued (before
        // the first row group this is the tile's own bound, without the guard band
        // the a-priori test has to include); requested later, it is recomputed like
        // any tile that finished un-stored.
        // (returns -1: abandoned; otherwise the number of outer column tiles the rest
        // of the row loop may leave out, >= ks_now)
        // Narrower in flight.  The same bound column by column: if every shift of the
        // outer K + 1 column tiles on either side (one tile of margin: guard_x <= 16)
        // already satisfies partial sum + rest + |correction|max < threshold_rel x the
        // running maximum, the K outer tiles are cold whatever the remaining rows hold,
        // and the loop continues in the variant without them; the epilogue zeroes them
        // like tiles left out a priori.  Zeros stand in for cold values wherever a cold
        // value may be read (a max-filter window); the windows that need true values
        // belong to hot elements, which this tile does not have within a tile of the
        // columns it dropped -- but another row tile of the band might.  So every tile
        // that may be hot records its hot column tiles (lz_cq), a stored tile records
        // how far it was narrowed (lz_ks), and the end-of-patch pass recomputes in full
        // what turns out to lie within a tile of a hot column (rare: the loop only
        // narrows to what the previous patch's hot columns leave, kmax_pred).
        // The tests are not free (80 integer maxima, wave reductions, a square root:
        // measured 2 300 cycles each next to the other workgroup's matrix loop, 23 %
        // of a wave's time in the tile loop when run every four row groups), so each
        // one schedules the next: the rest bound falls about linearly with the rows
        // that are left, which puts the earliest row at which the tile (or its outer
        // column tiles) can pass at  yhi - (rows left) x gap / rest  for the current
        // gap = threshold - partial maximum - |correction|max.
        auto check_after = [&](int y, int ks_now) {
          int run = 0, m_k[5] = {0, 0, 0, 0, 0};
          constexpr int kCand[5] = {col_skip_lo(NQ), col_skip_hi(NQ), col_skip_2(NQ),
                                    col_skip_3(NQ), col_skip_c(NQ)};
          if (y > ylo) {   // (before the first row group every sum is zero)
#pragma unroll
            for (int j = 0; j < (NQ + 1) / 2; ++j) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                run = max(run, acc[j][r]);
                run = max(run, acc[NQ - 1 - j][r]);
              }
#pragma unroll
              for (int i = 0; i < 5; ++i)
                if (kCand[i] == j) m_k[i] = run;   // tiles q <= K and q >= NQ - 1 - K
            }
          }
          const int ms = wave_max_nonneg_i(run);
          const unsigned* rp = reinterpret_cast<const unsigned*>(tb_lds + kRowPre);
          const int a_lo = max(0, y + dy0), a_hi = min(Py, yhi + dy0 + 15);
          const unsigned ea = rp[(a_hi + 3) >> 2] - rp[a_lo >> 2];
          const unsigned eb = rp[64 + ((yhi + 3) >> 2)] - rp[64 + (y >> 2)];
          // (margins: a few ulp of the product, the root and the two sums)
          const float rest = sqrtf(__uint2float_ru(ea) * __uint2float_ru(eb)) * 1.000002f + 2.f;
          const float corr = tb_lds[kBoundCorr];
          const float ub = (__int2float_ru(ms) + rest + corr) * 1.000002f + 2.f;
          const float thr_now = a.threshold_rel * __int_as_float(__builtin_amdgcn_readfirstlane(
                                                      *const_cast<volatile int*>(pmax_lds)));
          const int req = __builtin_amdgcn_readfirstlane(*const_cast<volatile int*>(&lz[0]));
          const bool requested = (req >> p) & 1;
          if (ub < thr_now && !requested) {
            if (lane == 0) {
              lz_tmax[p] = ub;
              atomicOr(&lz[1], 1 << p);
            }
            return -1;
          }
          // earliest row at which a set of columns with partial maximum m can pass
          const float left = static_cast<float>(yhi - y);
          auto passes_at = [&](int m) {
            const float gap = thr_now - (__int2float_ru(m) + corr);
            return gap > 0.f ? yhi - static_cast<int>(left * (gap / rest)) : yhi;
          };
          int y_at = requested ? yhi : passes_at(ms);
          // (before the first row group nothing is known about the columns: the first
          // row at which anything can pass -- requested tiles are tested for narrowing only)
          if (y == ylo && kmax_pred > ks_now) y_at = min(y_at, passes_at(0));
          int ks_new = ks_now;
          if (y > ylo && kmax_pred > ks_now) {
            bool open = true;   // widest first: the sets are nested
#pragma unroll
            for (int i = 4; i >= 0; --i) {
              if (i < 4 && kCand[i] == kCand[i + 1]) continue;
              if (kCand[i] <= 0 || 2 * kCand[i] + 2 > NQ) continue;
              if (!open || kCand[i] <= ks_now || kCand[i] > kmax_pred) continue;   // (wave-uniform)
              const int mo = wave_max_nonneg_i(m_k[i]);
              const float ubk = (__int2float_ru(mo) + rest + corr) * 1.000002f + 2.f;
              if (ubk < thr_now) {
                ks_new = kCand[i];
                open = false;
              } else {
                y_at = min(y_at, passes_at(mo));
              }
            }
          }
          y_next = max(y + 4 * a.early, ylo + ((y_at - ylo + 3) & ~3));
          return ks_new;
        };
        auto rows = [&](auto ks_const) {
        constexpr int KS = decltype(ks_const)::value;
        v4i af[kW], bf[NCE];
        unsigned dn[kND];
#pragma unroll
        for (int j = 0; j < kND; ++j) dn[j] = *reinterpret_cast<const unsigned*>(bp + 4 * j);
#pragma unroll
        for (int w = 0; w < kW; ++w)
          af[w] = *reinterpret_cast<const v4i*>(ap + 16 * w);
#pragma unroll
        for (int c = 0; c < NCE; ++c)
#pragma unroll
          for (int k = 0; k < 4; ++k)
            bf[c][k] = static_cast<int>(
                __builtin_amdgcn_alignbyte(dn[4 * c + k + 1], dn[4 * c + k], sh));
        // Lazy modes: every a.early row groups (and before the first) the tile is
        // tested for being provably cold already, as a whole or in its outer column
        // tiles -- see check_after above.
        const int y_enter = yb0;
        for (;;) {
        int yseg = yhi;
        if (LAZY && chk_early) {
          if (yhi - yb0 > 8 && yb0 >= y_next && yb0 != y_checked) {
            y_checked = yb0;
            TICK(12)   // (timing build) row groups (and the loop prologue)
            const int ks_new = check_after(yb0, KS);
            TICK(11)   // (timing build) the in-loop tests
            if (ks_new < 0) {
              abandoned = true;
              break;
            }
            if (ks_new > KS) {   // the rest of the tile runs in a narrower variant
              col_skip = ks_new;
              narrowed = true;
              break;
            }
          }
          yseg = min(yhi, max(y_next, yb0 + 4));
        }
        for (; yb0 < yseg; yb0 += 4) {
          bp += 4 * a.pb;
#pragma unroll
          for (int ca = 0; ca < NCA; ++ca) {
            // the register set of the PREVIOUS chunk is free now: its reload and
            // this chunk's share of the next B dwords can sit in the MFMA gaps
            // (one LDS instruction per gap) instead of in a burst behind them
            if (ca > 0) {
              const int cp = ca - 1;
              if (cp + kW < NCA)
                af[cp % kW] = *reinterpret_cast<const v4i*>(ap + 16 * (cp + kW));
              else
                af[cp % kW] =
                    *reinterpret_cast<const v4i*>(ap + 4 * a.pa + 16 * (cp + kW - NCA));
            }
            if (ca < NCA - 1) {
#pragma unroll
              for (int j = ca * kPerCa; j < (ca + 1) * kPerCa && j < kND; ++j)
                dn[j] = *reinterpret_cast<const unsigned*>(bp + 4 * j);
            }
#pragma unroll
            for (int c = 0; c < NCE; ++c) {
              const int q = ca - c + cq0;
              if (q >= KS && q < NQ - KS)
                acc[q] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[ca % kW], bf[c], acc[q], 0,
                                                               0, 0);
              if (ca == NCA - 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                  bf[c][k] = static_cast<int>(
                      __builtin_amdgcn_alignbyte(dn[4 * c + k + 1], dn[4 * c + k], sh));
              }
            }
            if (ca == NCA - 1)  // the last chunk's set: nothing follows in this group
              af[ca % kW] =
                  *reinterpret_cast<const v4i*>(ap + 4 * a.pa + 16 * (ca + kW - NCA));
            if (ca < NCA - 1) {
              // MFMAs of this chunk: columns q = ca - c + cq0 inside [KS, NQ - KS)
              const int c_lo = ca + cq0 - (NQ - KS - 1) > 0 ? ca + cq0 - (NQ - KS - 1) : 0;
              const int c_hi = ca + cq0 - KS < NCE - 1 ? ca + cq0 - KS : NCE - 1;
              const int n_mfma = c_hi - c_lo + 1;
              // (the builtin wants literal counts; ca is a constant after unrolling)
#define SFM_PAIR(i)                                                             \
  if (n_mfma > i) {                                                             \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); /* one MFMA */           \
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); /* one LDS read */       \
  }
              SFM_PAIR(0) SFM_PAIR(1) SFM_PAIR(2) SFM_PAIR(3)
#undef SFM_PAIR
              switch (n_mfma - 4) {
                case 1: __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); break;
                case 2: __builtin_amdgcn_sched_group_barrier(0x008, 2, 0); break;
                case 3: __builtin_amdgcn_sched_group_barrier(0x008, 3, 0); break;
                case 4: __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); break;
                case 5: __builtin_amdgcn_sched_group_barrier(0x008, 5, 0); break;
                case 6: __builtin_amdgcn_sched_group_barrier(0x008, 6, 0); break;
                case 7: __builtin_amdgcn_sched_group_barrier(0x008, 7, 0); break;
                case 8: __builtin_amdgcn_sched_group_barrier(0x008, 8, 0); break;
                default: break;
              }
              static_assert(NCE - 4 <= 8, "extend the switch");
            }
            // keep the chunk order: the machine scheduler would otherwise sink
            // every prefetch to the end of the body (= no prefetch distance)
            __builtin_amdgcn_sched_barrier(0);
          }
          ap += 4 * a.pa;
        }
        if (yb0 >= yhi) break;
        }
        {
          // instructions of one row group of this variant: (ca, c) pairs whose
          // column tile q = ca - c + cq0 is kept
          int per_group = 0;
#pragma unroll
          for (int ca = 0; ca < NCA; ++ca)
#pragma unroll
            for (int c = 0; c < NCE; ++c)
              per_group += (ca - c + NCE - 1 >= KS && ca - c + NCE - 1 < NQ - KS) ? 1 : 0;
          mfma_issued += (long long)((yb0 - y_enter) / 4) * per_group;  // (groups issued)
        }
        };
        constexpr int kKs1 = col_skip_lo(NQ), kKs2 = col_skip_hi(NQ);
        constexpr int kKs3 = col_skip_2(NQ), kKs4 = col_skip_3(NQ);
        constexpr int kKs5 = (LAZY && 2 * col_skip_c(NQ) + 2 <= NQ) ? col_skip_c(NQ) : 0;
        static_assert(kKs1 <= kKs2 && kKs2 <= kKs3 && kKs3 <= kKs4, "ascending");
        // (a variant returns when the tile is finished, abandoned or to be continued
        // in a narrower variant)
        TICK(10)   // (timing build) tile draw, pruning tests, setup
        // ascending and straight-line: a tile only ever moves to a narrower variant
        // (a loop around one dispatch made the register allocator spill 255 VGPRs)
        // (the test before the first row group runs here: a tile it abandons never
        // loads the loop's first fragments)
        if (LAZY && chk_early && yhi - ylo > 8) {
          // check_after(ylo) on the values read with the pruning bounds: every partial
          // sum is zero, the bound is the tile's own a-priori bound
          y_checked = ylo;
          const float rest = sqrtf(__uint2float_ru(hd_ea) * __uint2float_ru(hd_eb)) * 1.000002f + 2.f;
          const float ub = (rest + hd_corr) * 1.000002f + 2.f;
          const bool requested = (__builtin_amdgcn_readfirstlane(hd_req) >> p) & 1;
          if (ub < hd_thr && !requested) {
            if (lane == 0) {
              lz_tmax[p] = ub;
              atomicOr(&lz[1], 1 << p);
            }
            abandoned = true;
          } else {
            const float gap = hd_thr - hd_corr;
            const int y0_at = gap > 0.f ? yhi - static_cast<int>(static_cast<float>(yhi - ylo) * (gap / rest)) : yhi;
            const int y_at = (requested && kmax_pred <= col_skip) ? yhi : y0_at;
            y_next = max(ylo + 4 * a.early, ylo + ((y_at - ylo + 3) & ~3));
          }
        }
        if (!abandoned && (col_skip == 0 || (kKs1 == 0 && col_skip == kKs1)))
          rows(std::integral_constant<int, 0>{});
        if (kKs1 > 0 && col_skip == kKs1 && !abandoned && yb0 < yhi)
          rows(std::integral_constant<int, kKs1>{});
        if (kKs2 > kKs1 && col_skip == kKs2 && !abandoned && yb0 < yhi)
          rows(std::integral_constant<int, kKs2>{});
        if (kKs3 > kKs2 && col_skip == kKs3 && !abandoned && yb0 < yhi)
          rows(std::integral_constant<int, kKs3>{});
        if (kKs4 > kKs3 && col_skip == kKs4 && !abandoned && yb0 < yhi)
          rows(std::integral_constant<int, kKs4>{});
        if (kKs5 > kKs4 && col_skip == kKs5 && !abandoned && yb0 < yhi)
          rows(std::integral_constant<int, kKs5>{});
      } else if constexpr (WIDE8) {
        auto half_rows = [&](auto h_const) {
          constexpr int H = decltype(h_const)::value;
          constexpr int Q0 = H ? NQH : 0, Q1 = H ? NQ : NQH;
          // A chunks with a pair (ca, c) whose column tile ca - c + kCq0 lies in [Q0, Q1)
          constexpr int CA0 = Q0 - kCq0 > 0 ? Q0 - kCq0 : 0;
          constexpr int CA1 = Q1 - 1 < NCA - 1 ? Q1 - 1 : NCA - 1;
          constexpr int NC = CA1 - CA0 + 1;
          constexpr int kNDW = 4 * NCE + 1;   // B dwords of a row group
          int n_pairs = 0;
          // (the A chunks of the next row group are requested behind this group's B dwords:
          // two register sets, swapped by unrolling two groups per trip)
          auto group = [&](const v4i* af, v4i* af_next) {
            unsigned d[kNDW];
#pragma unroll
            for (int j = 0; j < kNDW; ++j) d[j] = *reinterpret_cast<const unsigned*>(bp + 4 * j);
            if (af_next) {
#pragma unroll
              for (int i = 0; i < NC; ++i)
                af_next[i] = *reinterpret_cast<const v4i*>(ap + 4 * a.pa + 16 * (CA0 + i));
            }
            v4i afl[NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) afl[i] = af[i];
#pragma unroll
            for (int c = 0; c < NCE; ++c) {
              v4i bf;
#pragma unroll
              for (int k = 0; k < 4; ++k)
                bf[k] = static_cast<int>(
                    __builtin_amdgcn_alignbyte(d[4 * c + k + 1], d[4 * c + k], sh));
#pragma unroll
              for (int i = 0; i < NC; ++i) {
                const int q = CA0 + i - c + kCq0;
                if (q >= Q0 && q < Q1)
                  acc[q - Q0] =
                      __builtin_amdgcn_mfma_i32_16x16x64_i8(afl[i], bf, acc[q - Q0], 0, 0, 0);
              }
            }
            ap += 4 * a.pa;
            bp += 4 * a.pb;
          };
          v4i afA[NC], afB[NC];
#pragma unroll
          for (int i = 0; i < NC; ++i)
            afA[i] = *reinterpret_cast<const v4i*>(ap + 16 * (CA0 + i));
          int yy = ylo;
          for (; yy + 4 < yhi; yy += 8) {
            group(afA, afB);
            group(afB, afA);
          }
          if (yy < yhi) group(afA, nullptr);
#pragma unroll
          for (int c = 0; c < NCE; ++c)
#pragma unroll
            for (int i = 0; i < NC; ++i)
              n_pairs += (CA0 + i - c + kCq0 >= Q0 && CA0 + i - c + kCq0 < Q1) ? 1 : 0;
          mfma_issued += (long long)((yhi - ylo + 3) / 4) * n_pairs;
        };
        if (half)
          half_rows(std::integral_constant<int, 1>{});
        else
          half_rows(std::integral_constant<int, 0>{});
      } else {
        for (int yb0 = ylo; yb0 < yhi; yb0 += 4) {
          v4i af[NCA];
#pragma unroll
          for (int ca = 0; ca < NCA; ++ca)
            af[ca] = *reinterpret_cast<const v4i*>(ap + 16 * ca);
          row_group(af, bp);
          ap += 4 * a.pa;
          bp += 4 * a.pb;
        }
        mfma_issued += (long long)((yhi - ylo + 3) / 4) * (NCA * NCE);
      }

      TICK(2)
      if (LAZY && abandoned) {
        ++tiles_early;
        continue;
      }
      if constexpr (LAZY) {
        // Cold tile, known before its epilogue: every output is S + correction, the
        // integer sums S are in the accumulators and |correction| has the patch-wide
        // bound of the seed probe (tbound[kBoundCorr]).  If max S + that bound stays
        // below threshold_rel x the running maximum, no element of the tile is hot,
        // none raises the maximum, and -- unless a hot tile asked for it -- nothing
        // of it is stored: the epilogue (40 table gathers and ~400 VALU operations
        // per lane) has nothing to deliver.  Asked for later after all, it is
        // recomputed like any band tile that finished un-stored.
        if (a.prune && !forced) {
          int ms = 0;   // (max(S, 0): a bound of max S all the same)
#pragma unroll
          for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) ms = max(ms, acc[q][r]);
          ms = wave_max_nonneg_i(ms);
          const float ub = __int2float_ru(ms) + tb_lds[kBoundCorr];
          const float mrun = __int_as_float(__builtin_amdgcn_readfirstlane(
              *const_cast<volatile int*>(pmax_lds)));
          const int req = __builtin_amdgcn_readfirstlane(*const_cast<volatile int*>(&lz[0]));
          if (ub < a.threshold_rel * mrun && !((req >> p) & 1)) {
            if (lane == 0) {
              lz_tmax[p] = ub;
              atomicOr(&lz[1], 1 << p);
            }
            continue;
          }
        }
      }
      if constexpr (LAZYG) {
        // The 16 rows of the correction table this tile's epilogue reads, built here
        // (the prep kernel of this mode leaves no table): rows yv = 16 Ib + j + 1, j < 16,
        // Ib = p mod (Py / 16), of
        //   G[yv][xv] = g_entry( IA'[yv][xv], IB'[Py - yv][Px - xv] ),
        //   IA'[yv][xv]           = sum_{x < xv} colA[x],  colA = c16[0][Ib] + rows 16 Ib .. yv - 1 of a'
        //   IB'[Py - yv][Px - xv] = T - sum_{x >= Px - xv} colB[x],
        //                           colB = c16[1][NB - Ib] - rows Py - yv .. 16 (NB - Ib) - 1 of b'
        // (a', b': the int8 operand copies in LDS; c16: centred column sums above every
        // 16th row, prep kernel; T = sum of colB over all columns).  This is the prep
        // kernel's sweep over 16 rows, run by the wave that needs them: lane l owns the
        // four columns 4 l .. 4 l + 3 of the pre patch and the MIRRORED columns of the post
        // patch (one aligned LDS dword per row and side), keeps their running column sums,
        // and a wave scan over the lane totals gives the exclusive prefixes, so the lane
        // leaves G[yv][4 l .. 4 l + 3] as one 16-byte store.  The same integers as the
        // table of the other modes, the same expression (g_entry): the same bits.  The rows
        // go to this patch's G area, now a scratch that stays in L2: every entry the
        // epilogue below gathers is stored here by this wave first.
        int oz;
        asm volatile("v_mov_b32 %0, 0" : "=v"(oz) : : "memory");
        const int NB = Py >> 4;
        const int Ib = p < NB ? p : p - NB;
        const int* c16 = a.c16 + b * a.c16_stride;
        const int l4 = 4 * lane + oz;
        const bool act = l4 < Px;
        const int xa = act ? l4 : 0;              // (idle lanes read column 0 and store nothing)
        const int xb = Px - 4 - xa;               // first of the four mirrored columns
        v4i ca = *reinterpret_cast<const v4i*>(c16 + Ib * Px + xa);
        const v4i cbn = *reinterpret_cast<const v4i*>(c16 + (NB + 1 + NB - Ib) * Px + xb);
        // tile NB - 1: its last row is dy = 0, i.e. yv = 0: IA' = 0 and IB' over ALL rows
        v4i call = v4i{0, 0, 0, 0};
        if (p == NB - 1) call = *reinterpret_cast<const v4i*>(c16 + (NB + 1 + NB) * Px + xb);
        int cb[4] = {cbn[3], cbn[2], cbn[1], cbn[0]};     // mirrored order
        if (!act) {
          ca = v4i{0, 0, 0, 0};
          call = v4i{0, 0, 0, 0};
#pragma unroll
          for (int k = 0; k < 4; ++k) cb[k] = 0;
        }
        const unsigned char* ap = A_lds + (kPadTop + 16 * Ib) * a.pa + xa;
        const unsigned char* bp = B_lds + (16 * (NB - Ib) - 1) * a.pb + a.ml + xb;
        float* Gw = a.gtab + (long long)b * Py * Px + xa;
#pragma unroll 4
        for (int j = 0; j < 16; ++j) {
          const unsigned da = *reinterpret_cast<const unsigned*>(ap + j * a.pa);
          const unsigned db = *reinterpret_cast<const unsigned*>(bp - j * a.pb);
          if (act) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              ca[k] += static_cast<int>(static_cast<signed char>(da >> (8 * k)));
              cb[k] -= static_cast<int>(static_cast<signed char>(db >> (8 * (3 - k))));
            }
          }
          const bool zero_row = p == NB - 1 && j == 15;      // yv = 0 (wave-uniform)
          int va[4], vb[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            va[k] = zero_row ? 0 : ca[k];
            vb[k] = zero_row ? call[3 - k] : cb[k];
          }
          const int sa = va[0] + va[1] + va[2] + va[3], sb = vb[0] + vb[1] + vb[2] + vb[3];
          const int inc_a = wave_scan_incl(sa), inc_b = wave_scan_incl(sb);
          const int tb = __builtin_amdgcn_readlane(inc_b, 63);   // T = IB'[Py - yv][Px]
          int ia = inc_a - sa, ib = tb - (inc_b - sb);
          v4i out;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            out[k] = __float_as_int(g_entry(mua, mub, static_cast<float>(ia), static_cast<float>(ib)));
            ia += va[k];
            ib -= vb[k];
          }
          const int yv = zero_row ? 0 : 16 * Ib + j + 1;
          // (row 15 of the last tile is padding: there is no row yv = Py)
          if (act && yv < Py) *reinterpret_cast<v4i*>(Gw + yv * Px) = out;
        }
        // The epilogue below gathers these rows back (other lanes' stores included) through
        // loads the compiler cannot relate to the stores above: every store of this wave has
        // to have reached the L2 (vector memory is write-through) before the first gather
        // is issued.  (Tiles p and p + NB of a patch write the SAME values into the same
        // rows, possibly from two waves at once: duplicate writers of identical bits.)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      // The epilogue's table addresses do not depend on the MFMA loop; without
      // this opaque zero the compiler hoists its ~100 gathers above the loop
      // and spills the accumulators.  After the loop there are >140 free VGPRs,
      // so all gathers of a tile can be in flight together.
      int opaque_zero;
      asm volatile("v_mov_b32 %0, 0" : "=v"(opaque_zero) : : "memory");
      // Epilogue: lane holds rows ky = 16 p + 4 g + r, columns kx = 16 q + n.
      // Branch-free: indices are clamped so every table load is in bounds;
      // only the store is predicated.
      // The surface buffer is padded to whole tiles (pitch 16 NQ, 16 NP rows),
      // so every lane stores unconditionally.
      int srow[4];
      bool rowok[4];
      float tmax = 0.f;  // max(tile, 0): only positive maxima matter
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        srow[r] = (16 * p + 4 * g + r) * a.sx_pitch + n;
        rowok[r] = 16 * p + 4 * g + r < Sy;
      }
#ifdef SFM_ABLATE_EPILOGUE
      // timing experiment only (results are garbage): how fast is the kernel
      // when a tile costs nothing after its matrix loop?
      {
        int sink = 0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) sink ^= acc[q][0] ^ acc[q][1] ^ acc[q][2] ^ acc[q][3];
        if (sink == 0x7fffffff) a.surface[0] = 1.f;
        continue;
      }
#endif
      // One column tile's share of the hot list (see the tile's peak pass below).
      int hq_lo = NQ, hq_hi = -1;   // column tiles with elements that may be hot
      auto hot_insert = [&](const int q, const float v0, const float v1, const float v2,
                            const float v3, const float thr_t) {
        float* hv = a.hot_val + (long long)b * a.hot_cap;
        int* hi = a.hot_idx + (long long)b * a.hot_cap;
        const float vv[4] = {v0, v1, v2, v3};
        const float vm = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
        if (__any(vm > thr_t)) {  // wave-uniform, rarely taken
          hq_lo = min(hq_lo, q);
          hq_hi = q;
          // one list reservation per column tile (ballots + one LDS atomic): an
          // atomic per lane and row was four dependent LDS round trips here
          unsigned long long bal[4];
          int total = 0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            bal[r] = __ballot(vv[r] > thr_t);
            total += __builtin_popcountll(bal[r]);
          }
          int base = 0;
          if (lane == 0) base = atomicAdd(hot_lds, total);
          base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = vv[r];
            if (v > thr_t) {
              const int slot = base + static_cast<int>(__builtin_amdgcn_mbcnt_hi(
                                          static_cast<unsigned>(bal[r] >> 32),
                                          __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(bal[r]), 0u)));
              if (slot < a.hot_cap) {
                hv[slot] = v;
                hi[slot] = (16 * p + 4 * g + r) * Sx + 16 * q + n;
              }
            }
            base += __builtin_popcountll(bal[r]);
          }
        }
      };
      // kModeGeneral, search-window variants (NCA > 10): the epilogue (pass 0) and the
      // hot-list pass (pass 1) over the column tiles of this row tile.
      // Search-window variants: a lone wave per SIMD pays every round trip of its table
      // look-ups in full, and eight of them per output (two box sums from two integral
      // images) made the epilogue as long as the matrix loop.  With Px >= Qx a shift dx
      // is in one of three regimes, and in each of them half of the eight corner terms
      // are a row constant or zero:
      //   L  dx <= 0:            xa0 = 0 (IA[.][0] = 0),  xb1 = Qx (row total of B)
      //   M  0 < dx < Px - Qx:   xb0 = 0,  xb1 = Qx: the post patch lies inside -- SB is
      //                          the row total, SA the only box with four corners
      //   R  dx >= Px - Qx:      xa1 = Px (row total of A),  xb0 = 0
      // so FOUR gathers per output are enough, selected per lane without a branch:
      //   v0, v1 = IA[oa1 | oa0][L, M: xa1;  R: xa0]
      //   v2, v3 = L: IB[ob1 | ob0][xb0]   M: IA[oa1 | oa0][xa0]   R: IB[ob1 | ob0][xb1]
      //   SA = L: v0 - v1   M: (v0 - v1) - (v2 - v3)   R: total_A - (v0 - v1)
      //   SB = L: total_B - (v2 - v3)   M: total_B   R: v2 - v3
      // -- the same integers as the eight-corner form, so the same bits.  The gathers of
      // a group of column tiles are all in flight before the previous group is consumed.
      auto wide_general = [&](const int pass, const float thr) {
        if constexpr (NCA > 10 && MODE == kModeGeneral) {
          const int ipa = Px + 1, ipb = Qx + 1;
          int oa0[4], oa1[4], ob0[4], ob1[4], ny[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ky = min(16 * p + 4 * g + r, Sy - 1);
            const int dy = ky - (Qy - 1);
            const int ya0 = max(0, dy), ya1 = min(Py, Qy + dy);
            oa0[r] = ya0 * ipa + opaque_zero;
            oa1[r] = ya1 * ipa;
            ob0[r] = (ya0 - dy) * ipb + opaque_zero;
            ob1[r] = (ya1 - dy) * ipb;
            ny[r] = ya1 - ya0;
          }
          int ta[4], tb[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            ta[r] = IA[oa1[r] + Px] - IA[oa0[r] + Px];
            tb[r] = IB[ob1[r] + Qx] - IB[ob0[r] + Qx];
          }
          // (regimes as all-ones / zero lane masks: nested selects came out as divergent
          // branches, one basic block per output)
          const long long ib_delta = IB - IA;   // IB's entries addressed from IA
          // The column tiles are walked by a RUN-TIME loop, two tiles per trip: unrolled over
          // 25 .. 30 tiles the scheduler hoisted every gather of a tile's 100 .. 120 outputs
          // per lane to the front and spilled a thousand registers.  The accumulator tile of
          // a run-time q is reached through a switch over its compile-time names (a compare
          // tree on a scalar: the accumulators must never be indexed dynamically) and is
          // only ever READ here -- a loop that also wrote the finished values back through
          // such a switch left every register array of the kernel in scratch memory.  The
          // hot-list pass (pass 1, only for a tile that may hold a hot element: a few per
          // patch) therefore recomputes its values from the integer sums instead.
          auto acc_get = [&](int q, int* dst) {
            switch (q) {
#define SFM_ACC_CASE(k)                                                   \
  case k:                                                                 \
    if constexpr (k < NQ) {                                               \
      dst[0] = acc[k][0]; dst[1] = acc[k][1]; dst[2] = acc[k][2]; dst[3] = acc[k][3]; \
    }                                                                     \
    break;
              SFM_ACC_CASE(0) SFM_ACC_CASE(1) SFM_ACC_CASE(2) SFM_ACC_CASE(3) SFM_ACC_CASE(4)
              SFM_ACC_CASE(5) SFM_ACC_CASE(6) SFM_ACC_CASE(7) SFM_ACC_CASE(8) SFM_ACC_CASE(9)
              SFM_ACC_CASE(10) SFM_ACC_CASE(11) SFM_ACC_CASE(12) SFM_ACC_CASE(13) SFM_ACC_CASE(14)
              SFM_ACC_CASE(15) SFM_ACC_CASE(16) SFM_ACC_CASE(17) SFM_ACC_CASE(18) SFM_ACC_CASE(19)
              SFM_ACC_CASE(20) SFM_ACC_CASE(21) SFM_ACC_CASE(22) SFM_ACC_CASE(23) SFM_ACC_CASE(24)
              SFM_ACC_CASE(25) SFM_ACC_CASE(26) SFM_ACC_CASE(27) SFM_ACC_CASE(28) SFM_ACC_CASE(29)
#undef SFM_ACC_CASE
              default: break;
            }
          };
          static_assert(NQ <= 30, "extend the accumulator switch");
          const int qb_half = WIDE8 ? half * NQH : 0;
          const int qe_half = WIDE8 ? min(NQ, qb_half + NQH) : NQ;
          // One trip: the column tiles q0 .. q0 + kT - 1 of the run that ends at hi.  REG:
          // the regime every lane of both tiles is in (0 L, 1 M, 2 R: scalar table bases,
          // 32-bit byte offsets, no selects) or 3 (the one or two tiles a regime boundary
          // runs through: per-lane masks).
          constexpr int kT = 2;   // column tiles per trip (16 kT gathers in flight)
          // (REG 0 .. 2: consecutive tiles are 16 columns = 64 bytes apart in every table row
          // and in the surface, so a trip forms its addresses once, for its first tile, and
          // reaches the others through the instructions' immediate offsets)
          auto trip = [&](auto reg_const, auto t_const, const int q0) {
            constexpr int REG = decltype(reg_const)::value;
            constexpr int T = decltype(t_const)::value;
            int sv[T][4], gv[T][4][4], mLs[T], mRs[T], xw[T];
#pragma unroll
            for (int u = 0; u < T; ++u) acc_get(q0 + u - qb_half, sv[u]);
            if constexpr (REG == 3) {
#pragma unroll
              for (int u = 0; u < T; ++u) {
                const int q = q0 + u;
                const int kx = 16 * q + n;
                const int dx = min(kx, Sx - 1) - (Qx - 1);
                const int xa0 = max(0, dx), xa1 = min(Px, Qx + dx);
                xw[u] = xa1 - xa0;
                const int mL = -static_cast<int>(dx <= 0);
                const int mR = ~mL & -static_cast<int>(dx >= Px - Qx);
                const int mM = ~(mL | mR);
                const int xb0 = xa0 - dx, xb1 = xa1 - dx;
                const int c01 = (xa0 & mR) | (xa1 & ~mR);
                const int c23 = (xb0 & mL) | (xa0 & mM) | (xb1 & mR);
                const long long d23 = ib_delta & ~static_cast<long long>(mM);
                mLs[u] = mL;
                mRs[u] = mR;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  gv[u][r][0] = IA[oa1[r] + c01];
                  gv[u][r][1] = IA[oa0[r] + c01];
                  gv[u][r][2] = IA[d23 + (((oa1[r] & mM) | (ob1[r] & ~mM)) + c23)];
                  gv[u][r][3] = IA[d23 + (((oa0[r] & mM) | (ob0[r] & ~mM)) + c23)];
                }
              }
            } else {
              const int dx0 = 16 * q0 + n - (Qx - 1);     // (no clamped column in these runs)
              // L: IA[.][xa1 = Qx + dx], IB[.][xb0 = -dx]   M: IA[.][Qx + dx], IA[.][xa0 = dx]
              // R: IA[.][xa0 = dx], IB[.][xb1 = Px - dx]   -- step per tile: +16, except the
              // two IB columns, which step -16
              const int c01 = REG == 2 ? dx0 : Qx + dx0;
              const int c23 = REG == 0 ? -dx0 : (REG == 1 ? dx0 : Px - dx0);
              constexpr int kStep23 = REG == 1 ? 16 : -16;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int* p0 = IA + (oa1[r] + c01);
                const int* p1 = IA + (oa0[r] + c01);
                const int* p2 = REG == 1 ? IA + (oa1[r] + c23) : IB + (ob1[r] + c23);
                const int* p3 = REG == 1 ? IA + (oa0[r] + c23) : IB + (ob0[r] + c23);
#pragma unroll
                for (int u = 0; u < T; ++u) {
                  gv[u][r][0] = p0[16 * u];
                  gv[u][r][1] = p1[16 * u];
                  gv[u][r][2] = p2[kStep23 * u];
                  gv[u][r][3] = p3[kStep23 * u];
                }
              }
#pragma unroll
              for (int u = 0; u < T; ++u) {
                const int dx = dx0 + 16 * u;
                xw[u] = REG == 0 ? Qx + dx : (REG == 1 ? Qx : Px - dx);
              }
            }
            float* srow_p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) srow_p[r] = surf + (srow[r] + 16 * q0);
#pragma unroll
            for (int u = 0; u < T; ++u) {
              const int q = q0 + u;
              const int kx = 16 * q + n;
              const float fnx = static_cast<float>(xw[u]);
              float outv[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int d01 = gv[u][r][0] - gv[u][r][1], d23 = gv[u][r][2] - gv[u][r][3];
                int sa, sb;
                if constexpr (REG == 3) {
                  const int mL = mLs[u], mR = mRs[u], mM = ~(mL | mR);
                  sa = (d01 & ~mR) + ((ta[r] - d01) & mR) - (d23 & mM);
                  sb = ((tb[r] - d23) & mL) + (tb[r] & mM) + (d23 & mR);
                } else {
                  sa = REG == 0 ? d01 : (REG == 1 ? d01 - d23 : ta[r] - d01);
                  sb = REG == 0 ? tb[r] - d23 : (REG == 1 ? tb[r] : d23);
                }
                // (explicit fused operations: the passes and regimes are copies of this code,
                // and the hot list must hold the very bits pass 0 stored -- the first-peak
                // kernel compares a hot value with the stored surface around it)
                float v = static_cast<float>(sv[u][r]);
                v = __builtin_fmaf(-mua, static_cast<float>(sb), v);
                v = __builtin_fmaf(-mub, static_cast<float>(sa), v);
                v = __builtin_fmaf(muab, __fmul_rn(static_cast<float>(ny[r]), fnx), v);
                // (a variant wider than the patch has whole column tiles past the surface:
                // their clamped shifts carry the mean correction of the last column without
                // its product sum, which outgrows the true maximum once |mean - centre| is
                // large -- they must reach neither the running maximum nor the hot list)
                const bool ok = REG == 3 ? rowok[r] && kx < Sx : rowok[r];
                if (pass == 0) {
                  __builtin_nontemporal_store(v, srow_p[r] + 16 * u);
                  tmax = fmaxf(tmax, ok ? v : 0.f);
                }
                outv[r] = ok ? v : -INFINITY;
              }
              if (pass == 1) hot_insert(q, outv[0], outv[1], outv[2], outv[3], thr);
            }
          };
          auto run = [&](auto reg_const, int lo, int hi) {   // tiles [lo, hi)
            int q0 = lo;
#pragma unroll 1
            for (; q0 + kT <= hi; q0 += kT) trip(reg_const, std::integral_constant<int, kT>{}, q0);
#pragma unroll 1
            for (; q0 < hi; ++q0) trip(reg_const, std::integral_constant<int, 1>{}, q0);
          };
          // Column tiles by regime (dx = 16 q + n - (Qx - 1), n = 0 .. 15; the clamped
          // columns past the surface count as R):
          //   L  every lane dx <= 0:            q < qL
          //   M  every lane 0 < dx < Px - Qx:   qM0 <= q < qM1
          //   R  every lane dx >= Px - Qx:      q >= qR
          const int qL = Qx >= 16 ? min((Qx - 16) / 16 + 1, NQ) : 0;
          const int qM0 = min((Qx + 15) / 16, NQ);
          const int qM1 = min(max(Px >= 17 ? (Px - 17) / 16 + 1 : 0, qM0), NQ);
          // (tiles with columns past the surface -- from column Sx on; several tiles when the
          // variant is wider than the patch -- take the per-lane code: their shifts are clamped)
          const int qc = min(Sx / 16, NQ);
          const int qR = min(max((Px + 14) / 16, qM1), qc);
          // (WIDE8: this job's column half only)
          auto run_c = [&](auto reg_const, int lo, int hi) {
            run(reg_const, max(lo, qb_half), min(hi, qe_half));
          };
          run_c(std::integral_constant<int, 0>{}, 0, min(qL, qc));
          run_c(std::integral_constant<int, 3>{}, min(qL, qc), min(qM0, qc));
          run_c(std::integral_constant<int, 1>{}, min(qM0, qc), min(qM1, qc));
          run_c(std::integral_constant<int, 3>{}, min(qM1, qc), qR);
          run_c(std::integral_constant<int, 2>{}, qR, qc);
          run_c(std::integral_constant<int, 3>{}, qc, NQ);
        }
      };
      if (RAW) {
        // exact integer products; the Padfield assembly happens afterwards
        int* raw = a.raw_out + (a.list ? item : b) * a.raw_stride;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) raw[srow[r] + 16 * q] = acc[q][r];
        continue;
      }
      if (SAME) {
        // corr = ey ex G[yv][xv] + ey Rrow[sx][yv] + ex Rcol[sy][xv] + const
        //        + mua mub ny nx        (header comment, item 3)
        // arranged as  (ey ex) g + A[r][sx] + B[q][sy] + fny[r] fnx[q]  with the
        // constants folded into A.  Rows / columns of the tile padding get
        // NaN through fny / fnx: NaN never wins fmaxf and never passes "> thr".
        const float* rrowA = R_lds;
        const float* rrowB = R_lds + a.aux_n;
        const float* rcolA = R_lds + 2 * a.aux_n;
        const float* rcolB = R_lds + 3 * a.aux_n;
        const int nn = n + opaque_zero;
        int grow[4];
        float ey[4], a_neg[4], a_pos[4], fny[4];
        bool sy[4];
        unsigned rowp[4];  // byte offsets into `surf` (scalar base + 32-bit offset)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ky_raw = 16 * p + 4 * g + r;
          const int ky = min(ky_raw, Sy - 1);
          const int dy = ky - (Py - 1);
          sy[r] = dy >= 0;
          const int yv = sy[r] ? dy : dy + Py;
          ey[r] = sy[r] ? -1.f : 1.f;
          grow[r] = yv * Px + opaque_zero;
          // A[r][sx]: sx = 0 (dx < 0) and sx = 1 (dx >= 0)
          a_neg[r] = ey[r] * rrowB[yv] + (sy[r] ? 0.f : const_b);
          a_pos[r] = ey[r] * rrowA[yv] + (sy[r] ? const_a : 0.f);
          fny[r] = ky_raw < Sy ? muab * static_cast<float>(Py - abs(dy)) : NAN;
          rowp[r] = 4u * static_cast<unsigned>(ky_raw * a.sx_pitch + nn);
        }
        if constexpr (EXACT) {
          // Px == 16 NCA: column tile q < NCA holds kx = 16 q + n < Px - 1 (dx < 0,
          // xv = kx + 1, ex = +1, fnx = kx + 1); tile q + NCA holds the shifts
          // dx = kx + 1 > 0 with the SAME xv (ex = -1, fnx = Px - xv).  The only
          // lanes that deviate are n = 15 of tile NCA - 1 (dx = 0: xv = 0) and of
          // tile 2 NCA - 1 (kx = Sx: padding).  Table addresses are one VGPR per
          // row plus an immediate, signs are folded into the instruction.
          const int xvb = nn + 1;                         // xv of tile 0
          const bool last = nn == 15;                     // the deviating lane
          const float fxb = static_cast<float>(xvb);
          const float* rcolA = R_lds + 2 * a.aux_n;
          const float* rcolB = R_lds + 3 * a.aux_n;
          unsigned gofs[4];                               // byte offsets of G[yv][xvb]
#pragma unroll
          for (int r = 0; r < 4; ++r) gofs[r] = 4u * static_cast<unsigned>(grow[r] + xvb);
          constexpr int kQG = 2;   // output columns per gather group
          constexpr int kGroupsE = (NCA + kQG - 1) / kQG;
          float gb[2][kQG][4];
          float rca_e[NCA], rcb_e[NCA];
#pragma unroll
          for (int qq = 0; qq < NCA; ++qq) {
            // the deviating lane of the last tile reads xv = 0 (first half); its
            // second-half value is padding
            const int xv = (qq == NCA - 1 && last) ? 0 : xvb + 16 * qq;
            rca_e[qq] = rcolA[xv];
            rcb_e[qq] = rcolB[xv];
          }
          auto fetch_e = [&](int grp, int slot) {
#pragma unroll
            for (int u = 0; u < kQG; ++u) {
              const int qq = grp * kQG + u;
              if (qq >= NCA) break;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                unsigned off = gofs[r] + 64u * qq;
                if (qq == NCA - 1)  // xv = 0 for the deviating lane (also keeps the
                  off = last ? 4u * static_cast<unsigned>(grow[r]) : off;  // read in bounds)
                gb[slot][u][r] = at_byte(G, off);
              }
            }
          };
          auto store4 = [&](int q, int r, float v) {
            if (q < col_skip || q >= NQ - col_skip) v = 0.f;  // column tile left out
            if constexpr (!LAZY)
              __builtin_nontemporal_store(
                  v, reinterpret_cast<float*>(reinterpret_cast<char*>(surf) +
                                              (static_cast<size_t>(rowp[r]) + 64u * q)));
            tmax = fmaxf(tmax, v);
            acc[q][r] = __float_as_int(v);
          };
          auto emit_e = [&](int qq, const float* gv) {
            // first half: dx < 0 (except the deviating lane of tile NCA - 1: dx = 0)
            {
              const int q = qq;
              const bool dev = qq == NCA - 1 && last;
              const float fnx = dev ? static_cast<float>(Px) : fxb + static_cast<float>(16 * qq);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float bsel = sy[r] ? rca_e[qq] : rcb_e[qq];
                float corr = dev ? fmaf(-ey[r], gv[r], a_pos[r]) - bsel
                                 : fmaf(ey[r], gv[r], a_neg[r]) + bsel;
                corr = fmaf(fny[r], fnx, corr);
                store4(q, r, static_cast<float>(acc[q][r]) + corr);
              }
            }
            // second half: dx = 16 qq + n + 1 > 0, same xv; the deviating lane of
            // the last tile is the padding column kx = Sx
            if (qq + NCA < NQ) {
              const int q = qq + NCA;
              const bool dev = qq == NCA - 1 && last;
              const float fnx =
                  dev ? NAN : static_cast<float>(Px) - (fxb + static_cast<float>(16 * qq));
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float bsel = sy[r] ? rca_e[qq] : rcb_e[qq];
                float corr = fmaf(-ey[r], gv[r], a_pos[r]) - bsel;
                corr = fmaf(fny[r], fnx, corr);
                store4(q, r, static_cast<float>(acc[q][r]) + corr);
              }
            }
          };
          fetch_e(0, 0);
#pragma unroll
          for (int grp = 0; grp < kGroupsE; ++grp) {
            __builtin_amdgcn_sched_barrier(0);
            if (grp + 1 < kGroupsE) fetch_e(grp + 1, (grp + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < kQG; ++u) {
              const int qq = grp * kQG + u;
              if (qq >= NCA) break;
              emit_e(qq, gb[grp & 1][u]);
            }
          }
        } else {
        const bool paired = Px == 16 * NCA;
        constexpr int kQG = 2;     // output columns per gather group
        constexpr int kDepth = 1;  // groups in flight ahead of the stores
        constexpr int kSlots = kDepth + 1;
        constexpr int kGroups = (NCA + kQG - 1) / kQG;
        auto xv_of = [&](int q) {
          const int dx = min(16 * q + nn, Sx - 1) - (Px - 1);
          return dx >= 0 ? dx : dx + Px;
        };
        // Column terms of all NQ output columns, read from LDS in one batch
        // (one round trip instead of one per column while the other waves
        // keep the LDS pipeline busy with matrix fragments).
        float rca[NQ], rcb[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int xv = xv_of(q);
          rca[q] = rcolA[xv];
          rcb[q] = rcolB[xv];
        }
        auto emit = [&](int q, const float* gv) {
          const int kx = 16 * q + nn;
          const int dx = min(kx, Sx - 1) - (Px - 1);
          const bool sx = dx >= 0;
          const int xv = sx ? dx : dx + Px;
          const float ex = sx ? -1.f : 1.f;
          const float b_pos = ex * rca[q];  // sy = 1
          const float b_neg = ex * rcb[q];  // sy = 0
          // (every column past the surface, not only those of the last tile: a variant
          // wider than the patch has whole tiles of them)
          const float fnx = kx < Sx ? static_cast<float>(Px - abs(dx)) : NAN;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float corr = fmaf(ey[r] * ex, gv[r], sx ? a_pos[r] : a_neg[r]);
            corr += sy[r] ? b_pos : b_neg;
            corr = fmaf(fny[r], fnx, corr);
            float v = static_cast<float>(acc[q][r]) + corr;
            if (q < col_skip || q >= NQ - col_skip) v = 0.f;  // column tile left out
            if constexpr (!LAZY)
              __builtin_nontemporal_store(
                  v, reinterpret_cast<float*>(reinterpret_cast<char*>(surf) +
                                              (static_cast<size_t>(rowp[r]) + 64u * q)));
            tmax = fmaxf(tmax, v);
            acc[q][r] = __float_as_int(v);
          }
        };
        // gbuf[slot][u][0] = G for column q, [1] = G for column q + NCA
        float gbuf[kSlots][kQG][2][4];
        auto fetch = [&](int grp, int slot) {
#pragma unroll
          for (int u = 0; u < kQG; ++u) {
            const int q = grp * kQG + u;
            if (q >= NCA) break;
            const int x0 = xv_of(q);
#pragma unroll
            for (int r = 0; r < 4; ++r) gbuf[slot][u][0][r] = at_byte(G, 4u * static_cast<unsigned>(grow[r] + x0));
            // Px == 16 NCA: column q + NCA reads the same table entries (the
            // copy is taken at use time; copying here would wait for the loads)
            if (q + NCA < NQ && !paired) {
              const int x1 = xv_of(q + NCA);
#pragma unroll
              for (int r = 0; r < 4; ++r) gbuf[slot][u][1][r] = at_byte(G, 4u * static_cast<unsigned>(grow[r] + x1));
            }
          }
        };
#pragma unroll
        for (int grp = 0; grp < kDepth; ++grp)
          if (grp < kGroups) fetch(grp, grp % kSlots);
#pragma unroll
        for (int grp = 0; grp < kGroups; ++grp) {
          __builtin_amdgcn_sched_barrier(0);
          if (grp + kDepth < kGroups) fetch(grp + kDepth, (grp + kDepth) % kSlots);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int u = 0; u < kQG; ++u) {
            const int q = grp * kQG + u;
            if (q >= NCA) break;
            emit(q, gbuf[grp % kSlots][u][0]);
            if (q + NCA < NQ) {
              float g1[4];
#pragma unroll
              for (int r = 0; r < 4; ++r)
                g1[r] = paired ? gbuf[grp % kSlots][u][0][r] : gbuf[grp % kSlots][u][1][r];
              emit(q + NCA, g1);
            }
          }
        }
        }  // generic (not EXACT) column handling
      } else {
        const int ipa = Px + 1, ipb = Qx + 1;
        int oa0[4], oa1[4], ob0[4], ob1[4], ny[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ky = min(16 * p + 4 * g + r, Sy - 1);
          const int dy = ky - (Qy - 1);
          const int ya0 = max(0, dy), ya1 = min(Py, Qy + dy);
          oa0[r] = ya0 * ipa + opaque_zero;
          oa1[r] = ya1 * ipa;
          ob0[r] = (ya0 - dy) * ipb + opaque_zero;
          ob1[r] = (ya1 - dy) * ipb;
          ny[r] = ya1 - ya0;
        }
        if constexpr (NCA > 10) {
          wide_general(0, 0.f);
        } else {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int kx = 16 * q + n;
          const int dx = min(kx, Sx - 1) - (Qx - 1);
          const int xa0 = max(0, dx), xa1 = min(Px, Qx + dx);
          const int xb0 = xa0 - dx, xb1 = xa1 - dx;
          const float fnx = static_cast<float>(xa1 - xa0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int sa = IA[oa1[r] + xa1] - IA[oa0[r] + xa1] -
                           IA[oa1[r] + xa0] + IA[oa0[r] + xa0];
            const int sb = IB[ob1[r] + xb1] - IB[ob0[r] + xb1] -
                           IB[ob1[r] + xb0] + IB[ob0[r] + xb0];
            float v = static_cast<float>(acc[q][r]);
            v = v - mua * static_cast<float>(sb);
            v = v - mub * static_cast<float>(sa);
            v = v + muab * (static_cast<float>(ny[r]) * fnx);
            surf[srow[r] + 16 * q] = v;
            const bool ok = rowok[r] && kx < Sx;   // (also in the tiles before the last)
            tmax = fmaxf(tmax, ok ? v : 0.f);
            acc[q][r] = __float_as_int(ok ? v : -INFINITY);
          }
        }
        }
      }
      TICK(3)
      if (a.do_peaks && forced) {
        // LAZY, recomputed tile: it is cold (nothing for the running maximum or
        // the hot list), it only has to reach memory
        if constexpr (LAZY) {
#pragma unroll
          for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              __builtin_nontemporal_store(
                  __int_as_float(acc[q][r]),
                  reinterpret_cast<float*>(reinterpret_cast<char*>(surf) +
                                           (4 * static_cast<size_t>(srow[r]) + 64u * q)));
          if (lane == 0) atomicOr(&lz[2], 1 << p);
        }
      } else if (a.do_peaks) {
        tmax = wave_max_nonneg(tmax);
        // non-negative floats order like their bit patterns; the atomic hands
        // back the running maximum of the tiles finished so far
        int prev_bits = 0;
        if (lane == 0) prev_bits = atomicMax(pmax_lds, __float_as_int(tmax));
        prev_bits = __builtin_amdgcn_readfirstlane(prev_bits);
        // Hot list: every element above threshold_rel * (running maximum) can
        // still turn out to be a peak; the final filter runs when the surface
        // is complete.  The running maximum never exceeds the final one, so
        // nothing that matters is dropped.
        const float mrun = fmaxf(tmax, __int_as_float(prev_bits));
        const float thr_t = a.threshold_rel * mrun;
        if (SAME && (a.prune || LAZY) && tmax > __int_as_float(prev_bits)) {
          // new running maximum (rare): remember its column tile for the seed
          // probe of the next patch
          int qbest = 0;
#pragma unroll
          for (int q = NQ - 1; q >= 0; --q) {
            const float vm = fmaxf(fmaxf(__int_as_float(acc[q][0]), __int_as_float(acc[q][1])),
                                   fmaxf(__int_as_float(acc[q][2]), __int_as_float(acc[q][3])));
            if (__any(vm == tmax)) qbest = q;
          }
          if (lane == 0) *best_lds = (p << 8) | qbest;
        }
        if constexpr (LAZY) {
          // Store this tile?  `hot`: it may hold an element above threshold_rel x
          // the final maximum (the running maximum only grows, so this errs on the
          // side of storing).  A hot tile asks for the tiles of its band; a
          // tile of the band that had finished before is dealt with at the end of
          // the patch, against the FINAL maximum (redo phase above).
          const bool hot = tmax > thr_t;
          int nbmask = 0;
          if (hot) {
            // rows of the tile that hold a possibly hot element -> the tiles the peak
            // kernels can read because of them (need_tiles)
            unsigned rowmask = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float vm = __int_as_float(acc[0][r]);
#pragma unroll
              for (int q = 1; q < NQ; ++q) vm = fmaxf(vm, __int_as_float(acc[q][r]));
              const unsigned long long bal = __ballot(vm > thr_t);
#pragma unroll
              for (int gg = 0; gg < 4; ++gg)
                if ((bal >> (16 * gg)) & 0xffffull) rowmask |= 1u << (4 * gg + r);
            }
            const int r_lo = __builtin_ctz(rowmask | 0x10000u);
            const int r_hi = 31 - __builtin_clz(rowmask | 1u);
            int lo_t, hi_t;
            need_tiles(a, 16 * p + r_lo, 16 * p + r_hi, &lo_t, &hi_t);
            nbmask = static_cast<int>(((2u << hi_t) - 1u) & ~((1u << lo_t) - 1u)) | (1 << p);
            if (lane == 0) lz_rows[p] = r_lo | (r_hi << 8);
          }
          int req = 0;
          if (lane == 0) {
            if (hot) atomicOr(&lz[0], nbmask);   // later tiles of the band store right away
            req = *const_cast<volatile int*>(&lz[0]);
          }
          req = __builtin_amdgcn_readfirstlane(req);
          const bool need = hot || ((req >> p) & 1);
          if (need) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                __builtin_nontemporal_store(
                    __int_as_float(acc[q][r]),
                    reinterpret_cast<float*>(reinterpret_cast<char*>(surf) +
                                             (4 * static_cast<size_t>(srow[r]) + 64u * q)));
          }
          if (lane == 0) {
            lz_tmax[p] = tmax;
            lz_ks[p] = narrowed ? col_skip : 0;
            if (need) atomicOr(&lz[2], 1 << p);
            atomicOr(&lz[1], 1 << p);
          }
        }
        // tmax is the wave-wide tile maximum: nothing to do unless it clears
        // the running threshold (the common case away from the peak).
        if (tmax > thr_t) {
        if constexpr (NCA > 10) wide_general(1, thr_t);
#pragma unroll
        for (int q = 0; q < (NCA > 10 ? 0 : NQ); ++q) {
          const float v0 = __int_as_float(acc[q][0]), v1 = __int_as_float(acc[q][1]);
          const float v2 = __int_as_float(acc[q][2]), v3 = __int_as_float(acc[q][3]);
          hot_insert(q, v0, v1, v2, v3, thr_t);
        }
        if (LAZY && lane == 0 && hq_hi >= 0) {
          atomicMin(&lz_cq[0], hq_lo);
          atomicMax(&lz_cq[1], hq_hi);
        }
        }
      }
      TICK(4)
      } while (0);
    }
    TICK(5)
    if (a.do_peaks) {
      // Publish the running maximum and the hot-list fill; the first-peak
      // search over them is mfma_first_peak_kernel (every patch in parallel,
      // off the matrix pipeline's critical path).
      __syncthreads();
      if (threadIdx.x == 0) {
        a.v1[b] = __int_as_float(*pmax_lds);
        a.hot_count[b] = *hot_lds;
        if (SAME && a.prune) a.skipmask[b] = best_lds[1];
        // un-stored tiles (pruned ones included) are what the sweeps must leave out
        if (LAZY) a.skipmask[b] = ~lz[2] & static_cast<int>((2u << (a.n_order - 1)) - 1u);
      }
    }
    TICK(6)
#ifdef SFM_MFMA_TIMING
    if (seed_pq >= 0 && *best_lds == seed_pq) ++run_seed[in_run];
#endif
  }
  if (a.clk && blockIdx.x == 0 && threadIdx.x == 0) {
    a.clk[0] = clock64() - probe_c0;
    a.clk[1] = wall_clock64() - probe_w0;
  }
  // (only while the timing hooks are on: same-address atomics are serialised in the
  // L2 -- three per wave cost a launch of one patch per workgroup 100 us at its end)
  if (SAME && a.prune && a.count_tiles && a.clk && lane == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(a.clk + 2),
              (static_cast<unsigned long long>(tiles_drawn) << 32) |
                  static_cast<unsigned long long>(tiles_skipped));
    atomicAdd(reinterpret_cast<unsigned long long*>(a.clk + 3),
              (static_cast<unsigned long long>(tiles_early) << 32) |
                  static_cast<unsigned long long>(cols_skipped));
  }
  if (a.count_tiles && a.clk && lane == 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(a.clk + 4),
              static_cast<unsigned long long>(mfma_issued));
#ifdef SFM_MFMA_TIMING
  if (a.work_counter && lane == 0) {
    // Run statistics of the launch; the wave that finishes last prints them.
    int* rs = a.work_counter;
    for (int k = 0; k < 2; ++k) {
      if (wave == 0) atomicAdd(rs + 2 + k, run_pat[k]);
      atomicAdd(rs + 4 + k, run_redo[k]);
      if (wave == 0) atomicAdd(rs + 6 + k, run_seed[k]);
    }
    __threadfence();
    if (atomicAdd(rs + 1, 1) == static_cast<int>(gridDim.x * (blockDim.x >> 6)) - 1) {
      int v[6];
      for (int k = 0; k < 6; ++k) v[k] = atomicAdd(rs + 2 + k, 0);
      printf("RUNS run %d grid %d batch %d: patches head %d inside %d redone head %d inside %d "
             "seed==peak head %d inside %d\n",
             a.run, gridDim.x, a.batch, v[0], v[1], v[2], v[3], v[4], v[5]);
    }
  }
  if (lane == 0 && wave == 0) {
    // HW_REG_HW_ID (4): [11:8] CU, [12] SH, [15:13] SE; HW_REG_XCC_ID (20): [3:0]
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
    const long long wall = wall_clock64() - wstart, cyc = clock64() - cstart;
    printf("WG %d xcc %u se %u cu %u patches %d wall %lld cycles %lld MHz %lld mfma %lld epi %lld\n",
           blockIdx.x, xcc & 15, (hw >> 13) & 7, (hw >> 8) & 15, npat, wall, cyc,
           wall ? cyc * 100 / wall : 0, tph[2] / (npat ? npat : 1),
           tph[3] / (npat ? npat : 1));
  }
  if (blockIdx.x == 7 && lane == 0)
    printf("wave %d patches %d: next %lld sync %lld pix %lld aux+touch %lld stagesync %lld mfma %lld (+ setup %lld tests %lld groups %lld) epi %lld hot %lld tail %lld peaks %lld\n",
           wave, npat, tph[7] / npat, tph[0] / npat, tph[8] / npat, tph[9] / npat, tph[1] / npat, tph[2] / npat,
           tph[10] / npat, tph[11] / npat, tph[12] / npat, tph[3] / npat,
           tph[4] / npat, tph[5] / npat, tph[6] / npat);
#endif
}

// How the patch queue hands out the batch to `grid` workgroups (MfmaArgs::run).  RUNS: the
// same-size launches, whose workgroups carry predictions from patch to patch; the raw and
// search-window launches keep one patch per ticket.
//
// A workgroup predicts the seed block, the need mask and the hot columns of a patch from its
// previous one, so consecutive patches of a workgroup should be neighbours in the field: a
// ticket is a run of kRun consecutive patches (SFM_MFMA_RUN=n; 1: one patch per ticket, the
// order before runs existed).  The last kRunTail x grid patches go out one at a time, so that
// the launch ends balanced (a run is kRun x ~120 us of a workgroup; SFM_MFMA_RUN_TAIL=n, a
// measurement switch).  A batch below grid x run shrinks the run: nobody starts without work
// while others hold runs.  8 / 8: measured, DESIGN_LOG.md "Runs".
constexpr int kRun = 8;
constexpr int kRunTail = 8;
template <bool RUNS>
void set_runs(int grid, MfmaArgs* ap) {
  MfmaArgs& a = *ap;
  a.run = 1;
  a.n_runs = a.run_end = 0;
  if (!RUNS || !a.work_counter || grid < 1) return;
  const int want = std::min(std::max(sfm::option_int("SFM_MFMA_RUN", kRun), 1), 64);
  a.run = std::max(std::min(want, a.batch / grid), 1);
  if (a.run == 1) return;
  const int tail_mult = std::max(sfm::measure_option_int("SFM_MFMA_RUN_TAIL", kRunTail), 0);
  // (the first assignment of every workgroup stays a run)
  const long long tail = std::min<long long>((long long)tail_mult * grid,
                                             a.batch - (long long)grid * a.run);
  a.n_runs = static_cast<int>((a.batch - tail) / a.run);
  a.run_end = a.n_runs * a.run;
}

template <int NCA, int NCE, int MODE>
int launch_one(const MfmaArgs& a, int grid, size_t lds, hipStream_t st) {
  // (search-window variants: eight waves per workgroup, see WIDE8 in the kernel)
  constexpr int kThreadsV = NCA > 10 ? kWideThreads : kThreads;
  if (int rc = sfm::set_lds(&xcorr_mfma_kernel<NCA, NCE, MODE>, lds)) return rc;
  // Persistent grid: as many workgroups as the CUs hold at once (registers and
  // LDS decide: 2 per CU for 160-wide patches, 3-4 for the small variants).
  int wg_per_cu = sfm::blocks_per_cu(
      reinterpret_cast<const void*>(&xcorr_mfma_kernel<NCA, NCE, MODE>), kThreadsV, lds);
  if (wg_per_cu < 1) wg_per_cu = lds * 2 <= kLdsPerCu ? 2 : 1;
  {
    // (a measurement switch; read per call so that a test can flip it)
    const int cap = sfm::measure_option_int("SFM_MFMA_MAX_WG_PER_CU", 0);
    if (cap > 0) wg_per_cu = std::min(wg_per_cu, cap);
  }
  grid = std::min(grid, sfm::device_cus() * wg_per_cu);
  {
    // SFM_MFMA_GRID=n (tests): at most n workgroups, so that a small batch runs
    // MANY patches through one workgroup -- the state a workgroup carries from
    // patch to patch (previous need mask / hot columns / seed block, the probe's
    // self-switch-off) is otherwise only exercised by full-size fields.
    const int g = sfm::option_int("SFM_MFMA_GRID", 0);
    if (g > 0) grid = std::min(grid, g);
  }
  MfmaArgs ar = a;
  set_runs<NCA <= 10 && MODE != kModeGeneral && MODE != kModeRaw>(grid, &ar);
  sfm::prof_begin(sfm::kProfXcorr, st);
  hipLaunchKernelGGL((xcorr_mfma_kernel<NCA, NCE, MODE>), dim3(grid),
                     dim3(kThreadsV), lds, st, ar);
  sfm::prof_end(sfm::kProfXcorr, st);
  sfm::prof_clock(sfm::kProfXcorr, a.clk, st, 5);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace

template <int NCA, int NCE>
int launch_variant(const MfmaArgs& a, int mode, int grid, size_t lds,
                   hipStream_t st) {
#ifdef SFM_DEV_ONLY_WIDE   // (development: compile the search-window variants alone)
  if constexpr (NCA <= 10) return sfm::fail(SFM_ERR_INVALID, "no MFMA variant");
  else
#endif
  if constexpr (NCA > 10) {   // search-window variants: un-masked general mode only
    if (mode != kModeGeneral) return sfm::fail(SFM_ERR_INVALID, "wide MFMA variant: general mode only");
    return launch_one<NCA, NCE, kModeGeneral>(a, grid, lds, st);
  } else
  switch (mode) {
    case kModeSame: return launch_one<NCA, NCE, kModeSame>(a, grid, lds, st);
    case kModeSameExact: return launch_one<NCA, NCE, kModeSameExact>(a, grid, lds, st);
    case kModeSameLazy: return launch_one<NCA, NCE, kModeSameLazy>(a, grid, lds, st);
    case kModeSameExactLazy: return launch_one<NCA, NCE, kModeSameExactLazy>(a, grid, lds, st);
    case kModeSameExactLazyG: return launch_one<NCA, NCE, kModeSameExactLazyG>(a, grid, lds, st);
    case kModeRaw: return launch_one<NCA, NCE, kModeRaw>(a, grid, lds, st);
    default: return launch_one<NCA, NCE, kModeGeneral>(a, grid, lds, st);
  }
}

}  // namespace mfma
}  // namespace sfm

// The whole of a geometry unit.
#define SFM_MFMA_GEOMETRY_UNIT(NCA, NCE)                                                \
  namespace sfm {                                                                      \
  namespace mfma {                                                                     \
  static_assert(listed_geometry(NCA, NCE), "not in SFM_MFMA_GEOMETRIES");              \
  template int launch_variant<NCA, NCE>(const MfmaArgs&, int, int, size_t, hipStream_t); \
  }                                                                                    \
  }

#endif  // SFM_MFMA_KERNEL_H_
