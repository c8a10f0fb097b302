// Matrix-core correlation path: the kernels around the correlation kernel -- prep (patch
// statistics, centres, integral images / correction tables), the masked (Padfield)
// assembly, the first-peak search -- and their launches.  sfm_mfma.h lists the units of
// the path; the overview of the algorithm is there too.
#include "sfm_mfma.h"

namespace sfm {
namespace mfma {
namespace {

// The correlation kernel's patch queue starts at ticket 0 (every prep kernel, one thread).
__device__ __forceinline__ void reset_patch_queue(const MfmaArgs& a) {
  *a.work_counter = 0;
#ifdef SFM_MFMA_TIMING
  for (int k = 1; k <= kRunStatWords; ++k) a.work_counter[k] = 0;  // run statistics
#endif
}

// ---------------------------------------------------------------------------
// prep: patch statistics, integer centre, integral image
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) mfma_prep_kernel(MfmaArgs a) {
  if (a.work_counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    reset_patch_queue(a);
  if (a.clk && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    a.clk[2] = a.clk[3] = a.clk[4] = 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int red[3][kThreads];
  const int b = blockIdx.x, s = blockIdx.y;
  const int py = s == 0 ? a.P[0] : a.Q[0];
  const int px = s == 0 ? a.P[1] : a.Q[1];
  const int H = a.ishape[s][0], W = a.ishape[s][1];
  // lax.dynamic_slice start clamping (flow_field.py:320-325).
  const int y0 = min(max(a.starts[s][b * 2 + 0], 0), H - py);
  const int x0 = min(max(a.starts[s][b * 2 + 1], 0), W - px);
  const unsigned char* img = a.img[s];
  int mn = 255, mx = 0, sum = 0;
  for (int i = threadIdx.x; i < py * px; i += kThreads) {
    const int y = i / px, x = i - y * px;
    const int v = img[(long long)(y0 + y) * W + x0 + x];
    smem[i] = static_cast<unsigned char>(v);
    mn = min(mn, v);
    mx = max(mx, v);
    sum += v;
  }
  red[0][threadIdx.x] = mn;
  red[1][threadIdx.x] = mx;
  red[2][threadIdx.x] = sum;
  __syncthreads();
  for (int k = kThreads / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      red[0][threadIdx.x] = min(red[0][threadIdx.x], red[0][threadIdx.x + k]);
      red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + k]);
      red[2][threadIdx.x] += red[2][threadIdx.x + k];
    }
    __syncthreads();
  }
  mn = red[0][0];
  mx = red[1][0];
  sum = red[2][0];
  const float n_f = static_cast<float>(py * px);
  const float mean = a.use_mean ? a.mean : static_cast<float>(sum) / n_f;
  // Centre: nearest integer to the mean that keeps every pixel in int8.
  int c = static_cast<int>(rintf(fminf(fmaxf(mean, 0.f), 255.f)));
  c = min(max(c, mx - 127), mn + 128);
  if (threadIdx.x == 0) {
    PatchParams* p = &a.pp[b];
    p->y0[s] = y0;
    p->x0[s] = x0;
    p->c[s] = c;
    p->mu[s] = a.use_mean
                   ? a.mean - static_cast<float>(c)
                   : static_cast<float>(
                         (static_cast<double>(sum) - static_cast<double>(c) * py * px) /
                         (static_cast<double>(py) * px));
  }
  int* I = a.integ[s] + b * a.integ_stride[s];
  const int ip = px + 1;
  // Column running sums -> I[y + 1][x + 1]; zero first row / column.
  for (int x = threadIdx.x; x <= px; x += kThreads) I[x] = 0;
  for (int y = threadIdx.x; y <= py; y += kThreads) I[y * ip] = 0;
  for (int x = threadIdx.x; x < px; x += kThreads) {
    int run = 0;
    for (int y = 0; y < py; ++y) {
      run += static_cast<int>(smem[y * px + x]) - c;
      I[(y + 1) * ip + x + 1] = run;
    }
  }
  __syncthreads();
  // Row-wise inclusive scan (wave scan with carry).
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int y = 1 + wave; y <= py; y += kWaves) {
    int carry = 0;
    for (int x0c = 0; x0c < px; x0c += 64) {
      const int x = x0c + lane;
      int v = x < px ? I[y * ip + x + 1] : 0;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
      }
      v += carry;
      if (x < px) I[y * ip + x + 1] = v;
      carry = __shfl(v, 63, 64);
    }
  }
}

// ---------------------------------------------------------------------------
// prep of the search-window variants (pre patches up to 320 x 320): the same outputs as
// mfma_prep_kernel -- clamped origin, integer centre, mean - centre, the integral image
// I[y + 1][x + 1] = sum_{y' <= y, x' <= x} (pixel - centre) of one patch side -- for patches
// where that kernel's thread-per-column sweep (a byte load per pixel, Py dependent LDS round
// trips per column, a second pass over the table in global memory) took a third of the
// correlation launch's time.  One workgroup of eight waves per (patch, side):
//   1. the patch goes to LDS with 16-byte loads (minimum, maximum and sum on the way);
//   2. wave w owns the rows [w R, (w + 1) R); lane l the columns 8 l .. 8 l + 7 (one aligned
//      8-byte LDS read per row).  A first sweep leaves the column sums of every stripe, so
//      that each wave knows the column sums ABOVE its stripe;
//   3. a second sweep carries the running column sums down the stripe; per row the lane's
//      eight prefix sums plus a wave scan of the lane totals are the integral-image row,
//      stored as two 16-byte pieces per lane (contiguous across the wave).
// ---------------------------------------------------------------------------
constexpr int kWidePrepWaves = 8;
constexpr int kWidePrepColsPerLane = 8, kWidePrepMaxCols = 64 * kWidePrepColsPerLane;
// static LDS of the kernel: per-wave reduction words and the column sums of every stripe
constexpr size_t kWidePrepStaticLds =
    sizeof(int) * (3 * kWidePrepWaves + kWidePrepWaves * kWidePrepMaxCols);
typedef int v4i_a4 __attribute__((ext_vector_type(4), aligned(4)));

__global__ void __launch_bounds__(64 * kWidePrepWaves) mfma_prep_wide_kernel(MfmaArgs a) {
  if (a.work_counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    reset_patch_queue(a);
  if (a.clk && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    a.clk[2] = a.clk[3] = a.clk[4] = 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int red[3][kWidePrepWaves];
  constexpr int kColsPerLane = kWidePrepColsPerLane, kMaxCols = kWidePrepMaxCols;
  __shared__ int stripe[kWidePrepWaves][kMaxCols];
  static_assert(sizeof(red) + sizeof(stripe) == kWidePrepStaticLds, "the host sizes the launch by it");
  const int b = blockIdx.x, s = blockIdx.y;
  const int py = s == 0 ? a.P[0] : a.Q[0];
  const int px = s == 0 ? a.P[1] : a.Q[1];
  const int H = a.ishape[s][0], W = a.ishape[s][1];
  // lax.dynamic_slice start clamping (flow_field.py:320-325).
  const int y0 = min(max(a.starts[s][b * 2 + 0], 0), H - py);
  const int x0 = min(max(a.starts[s][b * 2 + 1], 0), W - px);
  const unsigned char* img = a.img[s];
  const long long img_bytes = (long long)H * W;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_chunks = (px + 15) >> 4, pitch = 16 * n_chunks + 16;   // (+16: rows on different banks)
  int mn = 255, mx = 0, sum = 0;
  for (int item = threadIdx.x; item < py * n_chunks; item += 64 * kWidePrepWaves) {
    const int y = item / n_chunks, ch = item - y * n_chunks;
    v4i w = load_16_bytes(img, (long long)(y0 + y) * W + x0 + ch * 16, img_bytes);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned v = static_cast<unsigned>(w[k]);
      const int keep = min(px - (ch * 16 + 4 * k), 4);   // bytes of this dword inside the patch
      if (keep < 4) v = keep <= 0 ? 0u : (v & (0xffffffffu >> (8 * (4 - keep))));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int pv = static_cast<int>((v >> (8 * j)) & 255u);
        if (j < keep) {
          mn = min(mn, pv);
          mx = max(mx, pv);
        }
        sum += pv;   // (bytes outside the patch are zero)
      }
      w[k] = static_cast<int>(v);
    }
    *reinterpret_cast<v4i*>(smem + y * pitch + ch * 16) = w;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    mn = min(mn, __shfl_xor(mn, d, 64));
    mx = max(mx, __shfl_xor(mx, d, 64));
    sum += __shfl_xor(sum, d, 64);
  }
  if (lane == 0) {
    red[0][wave] = mn;
    red[1][wave] = mx;
    red[2][wave] = sum;
  }
  __syncthreads();
  mn = red[0][0];
  mx = red[1][0];
  sum = red[2][0];
#pragma unroll
  for (int w = 1; w < kWidePrepWaves; ++w) {
    mn = min(mn, red[0][w]);
    mx = max(mx, red[1][w]);
    sum += red[2][w];
  }
  const float n_f = static_cast<float>(py * px);
  const float mean = a.use_mean ? a.mean : static_cast<float>(sum) / n_f;
  // Centre: nearest integer to the mean that keeps every pixel in int8.
  int c = static_cast<int>(rintf(fminf(fmaxf(mean, 0.f), 255.f)));
  c = min(max(c, mx - 127), mn + 128);
  if (threadIdx.x == 0) {
    PatchParams* p = &a.pp[b];
    p->y0[s] = y0;
    p->x0[s] = x0;
    p->c[s] = c;
    p->mu[s] = a.use_mean
                   ? a.mean - static_cast<float>(c)
                   : static_cast<float>(
                         (static_cast<double>(sum) - static_cast<double>(c) * py * px) /
                         (static_cast<double>(py) * px));
  }
  int* I = a.integ[s] + b * a.integ_stride[s];
  const int ip = px + 1;
  const int R = (py + kWidePrepWaves - 1) / kWidePrepWaves;
  const int r0 = wave * R, r1 = min(py, r0 + R);
  const int xl = kColsPerLane * lane;
  const bool act = xl < px;
  // (columns past the patch hold zero bytes: they must not pick up -c)
  int cm[kColsPerLane];
#pragma unroll
  for (int k = 0; k < kColsPerLane; ++k) cm[k] = xl + k < px ? c : 0;
  auto row_pixels = [&](int y, int* pv) {
    const uint2 d = *reinterpret_cast<const uint2*>(smem + y * pitch + (act ? xl : 0));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pv[k] = static_cast<int>((d.x >> (8 * k)) & 255u) - cm[k];
      pv[4 + k] = static_cast<int>((d.y >> (8 * k)) & 255u) - cm[4 + k];
    }
  };
  int col[kColsPerLane];
#pragma unroll
  for (int k = 0; k < kColsPerLane; ++k) col[k] = 0;
  for (int y = r0; y < r1; ++y) {
    int pv[kColsPerLane];
    row_pixels(y, pv);
#pragma unroll
    for (int k = 0; k < kColsPerLane; ++k) col[k] += pv[k];
  }
#pragma unroll
  for (int k = 0; k < kColsPerLane; ++k) stripe[wave][xl + k] = act ? col[k] : 0;
  // zero first row / column of the table
  for (int x = threadIdx.x; x <= px; x += 64 * kWidePrepWaves) I[x] = 0;
  for (int y = threadIdx.x; y <= py; y += 64 * kWidePrepWaves) I[y * ip] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kColsPerLane; ++k) col[k] = 0;
  for (int w = 0; w < wave; ++w)
#pragma unroll
    for (int k = 0; k < kColsPerLane; ++k) col[k] += stripe[w][xl + k];
  for (int y = r0; y < r1; ++y) {
    int pv[kColsPerLane];
    row_pixels(y, pv);
    int run = 0, pre[kColsPerLane];
#pragma unroll
    for (int k = 0; k < kColsPerLane; ++k) {
      col[k] += pv[k];
      run += act ? col[k] : 0;
      pre[k] = run;
    }
    const int before = wave_scan_incl(run) - run;   // columns left of this lane
    if (act) {
      int* dst = I + (y + 1) * ip + xl + 1;
      const v4i_a4 lo = {pre[0] + before, pre[1] + before, pre[2] + before, pre[3] + before};
      const v4i_a4 hi = {pre[4] + before, pre[5] + before, pre[6] + before, pre[7] + before};
      if (xl + 8 <= px) {
        *reinterpret_cast<v4i_a4*>(dst) = lo;
        *reinterpret_cast<v4i_a4*>(dst + 4) = hi;
      } else {
#pragma unroll
        for (int k = 0; k < kColsPerLane; ++k)
          if (xl + k < px) dst[k] = (k < 4 ? lo[k] : hi[k - 4]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// prep for P == Q: centres, means, combined correction table G and the 1-D
// row / column arrays.  One 256-thread block per patch; LDS holds the two raw
// uint8 patches (2 Py Px bytes), so several blocks share a CU.
//
// Wave w sweeps the rows yv = [w R, (w + 1) R) of the table (R = ceil(Py / 4))
// keeping, per lane, the running column sums of the pre patch above row yv and
// of the post patch above row Py - yv; a wave scan over x turns them into the
// integral-image rows IA[yv][.] and IB[Py - yv][.]; raw pixel sums are used and
// the centre is folded in afterwards (I'[y][x] = Iraw[y][x] - c y x).
// ---------------------------------------------------------------------------

// v_pk_min_u16 / v_pk_max_u16 on two 16-bit fields of a dword
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) {
  us2 x, y;
  __builtin_memcpy(&x, &a, 4);
  __builtin_memcpy(&y, &b, 4);
  const us2 z = __builtin_elementwise_min(x, y);
  unsigned r;
  __builtin_memcpy(&r, &z, 4);
  return r;
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  us2 x, y;
  __builtin_memcpy(&x, &a, 4);
  __builtin_memcpy(&y, &b, 4);
  const us2 z = __builtin_elementwise_max(x, y);
  unsigned r;
  __builtin_memcpy(&r, &z, 4);
  return r;
}

// LDS tables of the prep pass (behind the two raw uint8 patches).
// (LAZY: the band sums live in the dynamic area, behind the packed words they come from)
template <int WAVES, int ROWS, bool LAZY>
struct PrepTables {
  int s_c[2];
  float s_mu[2];
  alignas(16) int band_tot[2][LAZY ? 1 : WAVES + 1][LAZY ? 4 : 64 * kPrepCols];
  // pruning bounds: per-row sum and sum of squares of the raw pixels, later the
  // prefix sums of the row energies (doubles)
  // (sum in the low, sum of squares in the high word: one 64-bit LDS atomic per item)
  unsigned long long row_acc[2][ROWS];
  double row_pre[2][ROWS + 1];
  int col_sq[2][64 * kPrepCols];  // column sums of squares (post: mirrored)
  int wred[2][3][WAVES];          // min / max / sum per wave (LAZY)
  // sums / sums of squares per 16 x 16 block, later their 2-D prefix sums (in place)
  unsigned long long blk_acc[2][kBlkRows][kBlkCols];  // packed like row_acc
};

// The prep pass of patch `b` by a workgroup of WAVES waves: `smem` holds the two
// raw patches (2 Py Px bytes, 16-byte aligned halves), `tp` the tables.  Used by
// the stand-alone kernel (8 waves, one block per patch).  Round 3 also ran it with
// 4 waves at the head of every patch INSIDE the correlation kernel (its LDS patch
// area as scratch, outputs written to global memory and read back): bit-identical,
// but the correlation kernel grew from 15.6 to 18.7 ms per pair while the 2.6 ms
// launch went away -- 19.25 vs 18.9 ms per pair.  The two workgroups of a CU do
// not stay in anti-phase, so the extra VALU / LDS phase of a patch is not hidden
// behind the other workgroup's matrix loop; it simply adds.  Removed again.
// LAZY (kModeSameExactLazyG, its own instantiation): the pass never needs a pixel
// twice, so nothing is staged in LDS -- see the fused loop below.
template <int WAVES, int ROWS, bool LAZY>
__device__ __forceinline__ void prep_same_body(const MfmaArgs& a, const int b,
                                               unsigned char* smem,
                                               PrepTables<WAVES, ROWS, LAZY>* tp) {
  constexpr int kPrepWaves = WAVES;
  constexpr int kPrepThreads = 64 * WAVES;
  int (&s_c)[2] = tp->s_c;
  float (&s_mu)[2] = tp->s_mu;
  auto& band_tot = tp->band_tot;
  // reduction scratch of phase 2, aliased onto band_tot (separated by a barrier)
  static_assert(LAZY || sizeof(tp->band_tot) >= sizeof(int) * 2 * 3 * kPrepThreads, "alias");
  // LAZY: band sums [2][Py / 16][Px] over the row words of the fused loop (same size),
  // written once those are folded into the row table
  int* const lazy_bsum = reinterpret_cast<int*>(smem);
  // (LAZY: band_tot holds the band sums by then; the scratch is its own small array)
  constexpr int kRedPitch = LAZY ? WAVES : kPrepThreads;
  int* const redp = LAZY ? &tp->wred[0][0][0] : &band_tot[0][0][0];
#define SFM_RED(s, i, w) redp[((s) * 3 + (i)) * kRedPitch + (w)]
  unsigned long long (&row_acc)[2][ROWS] = tp->row_acc;
  double (&row_pre)[2][ROWS + 1] = tp->row_pre;
  int (&col_sq)[2][64 * kPrepCols] = tp->col_sq;
  unsigned long long (&blk_acc)[2][kBlkRows][kBlkCols] = tp->blk_acc;
  const int py = a.P[0], px = a.P[1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned char* pix[2] = {smem, smem + ((py * px + 15) & ~15)};
  if (a.prune) {
    for (int i = threadIdx.x; i < 2 * ROWS; i += kPrepThreads) {
      (&row_acc[0][0])[i] = 0;
    }
    for (int i = threadIdx.x; i < 2 * 64 * kPrepCols; i += kPrepThreads) (&col_sq[0][0])[i] = 0;
    for (int i = threadIdx.x; i < 2 * kBlkRows * kBlkCols; i += kPrepThreads) {
      (&blk_acc[0][0][0])[i] = 0;
    }
    __syncthreads();
  }
#ifdef SFM_MFMA_TIMING
  long long pt[6]; pt[0] = clock64();
#define PTICK(i) pt[i] = clock64();
#else
#define PTICK(i)
#endif

  // Phase 1 + 2: copy both patches into LDS (unaligned 16-byte loads, all of a
  // round in flight together) and take min / max / sum of the pixels on the
  // way, from the registers.
  int y0[2], x0[2];
  int mn[2] = {255, 255}, mx[2] = {0, 0}, sum[2] = {0, 0};
  const int n_chunks = (px + 15) / 16;
  const int n_items = py * n_chunks;
  long long img_bytes[2];
  for (int s = 0; s < 2; ++s) {
    const int H = a.ishape[s][0], W = a.ishape[s][1];
    y0[s] = min(max(a.starts[s][b * 2 + 0], 0), H - py);
    x0[s] = min(max(a.starts[s][b * 2 + 1], 0), W - px);
    img_bytes[s] = (long long)H * W;
  }
  constexpr int kItems = 4;  // items per thread and plane whose loads are in flight
  if constexpr (LAZY) {
    // LAZY: everything this pass needs of a pixel is a sum -- per row, per column
    // and band of 16 rows, per 16 x 16 block, minimum / maximum -- so the patches
    // are never staged in LDS.  A thread takes one half block (8 rows x 16 columns
    // of one side: eight 16-byte loads in flight, one global round trip per patch)
    // and leaves its eight row sums and sixteen column sums, each packed with its
    // sum of squares into one word, in two LDS arrays (plain 16-byte stores: the
    // first version added them to the shared tables with 41 LDS atomics per thread,
    // 6- to 10-way address conflicts each, and spent 25 k cycles per patch here);
    // a second pass (a thread per row / per column) folds them into the tables
    // the staged form fills.  2 x Py / 8 x Px / 16 items (400 for 160 x 160).  The
    // same exact integers in the same tables: everything below is shared.  Py, Px
    // multiples of 16 (host: choose_mode).
    const int NB = py >> 4, NC = px >> 4;
    const int per_side = 2 * NB * NC;
    // rowpart[s][y][chunk] = row sum (12 bits) | sum of squares << 12;
    // halfcol[s][half band][x] = column sum over 8 rows (11 bits) | sum of squares << 11
    unsigned* rowpart = reinterpret_cast<unsigned*>(smem);
    unsigned* halfcol = rowpart + 2 * py * NC;
    unsigned mnp[2] = {0x00ff00ffu, 0x00ff00ffu}, mxp[2] = {0u, 0u};
    for (int item = threadIdx.x; item < 2 * per_side; item += kPrepThreads) {
      const int s = item >= per_side ? 1 : 0;
      const int rem = item - s * per_side;
      const int bh = rem / NC, ch = rem - bh * NC;   // half band (8 rows), chunk (16 columns)
      const int yb = 8 * bh;
      const int W = s ? a.ishape[1][1] : a.ishape[0][1];
      const unsigned char* img = s ? a.img[1] : a.img[0];
      const int yy0 = s ? y0[1] : y0[0], xx0 = s ? x0[1] : x0[0];
      const long long ib = s ? img_bytes[1] : img_bytes[0];
      v4i w[8];
#pragma unroll
      for (int r = 0; r < 8; ++r)
        w[r] = load_16_bytes(img, (long long)(yy0 + yb + r) * W + xx0 + ch * 16, ib);
      unsigned lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};   // bytes 0 | 2, 1 | 3 as 16-bit fields
      unsigned q[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) q[j] = 0;
      unsigned mn2 = 0x00ff00ffu, mx2 = 0u;
      int tsum = 0;
      unsigned tsq = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        int isum = 0, isq = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned v = static_cast<unsigned>(w[r][k]);
          const unsigned e = v & 0x00ff00ffu, o = (v >> 8) & 0x00ff00ffu;
          lo[k] += e;
          hi[k] += o;
          mn2 = pk_min_u16(pk_min_u16(mn2, e), o);
          mx2 = pk_max_u16(pk_max_u16(mx2, e), o);
          isum = static_cast<int>(__builtin_amdgcn_sad_u8(v, 0u, isum));
          isq = static_cast<int>(__builtin_amdgcn_udot4(v, v, isq, false));
          const unsigned b0 = v & 0xffu, b1 = (v >> 8) & 0xffu, b2 = (v >> 16) & 0xffu, b3 = v >> 24;
          q[4 * k + 0] = __umul24(b0, b0) + q[4 * k + 0];
          q[4 * k + 1] = __umul24(b1, b1) + q[4 * k + 1];
          q[4 * k + 2] = __umul24(b2, b2) + q[4 * k + 2];
          q[4 * k + 3] = __umul24(b3, b3) + q[4 * k + 3];
        }
        rowpart[(s * py + yb + r) * NC + ch] =
            static_cast<unsigned>(isum) | (static_cast<unsigned>(isq) << 12);
        tsum += isum;
        tsq += static_cast<unsigned>(isq);
      }
      atomicAdd(&blk_acc[s][bh >> 1][ch],
                (static_cast<unsigned long long>(tsq) << 32) | static_cast<unsigned>(tsum));
      v4i* hd = reinterpret_cast<v4i*>(halfcol + (s * 2 * NB + bh) * px + 16 * ch);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        hd[k] = v4i{static_cast<int>((lo[k] & 0xffffu) | (q[4 * k + 0] << 11)),
                    static_cast<int>((hi[k] & 0xffffu) | (q[4 * k + 1] << 11)),
                    static_cast<int>((lo[k] >> 16) | (q[4 * k + 2] << 11)),
                    static_cast<int>((hi[k] >> 16) | (q[4 * k + 3] << 11))};
      if (s) {
        mnp[1] = pk_min_u16(mnp[1], mn2);
        mxp[1] = pk_max_u16(mxp[1], mx2);
        sum[1] += tsum;
      } else {
        mnp[0] = pk_min_u16(mnp[0], mn2);
        mxp[0] = pk_max_u16(mxp[0], mx2);
        sum[0] += tsum;
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      mn[s] = static_cast<int>(min(mnp[s] & 0xffffu, mnp[s] >> 16));
      mx[s] = static_cast<int>(max(mxp[s] & 0xffffu, mxp[s] >> 16));
    }
  } else
  for (int item0 = threadIdx.x; item0 < n_items; item0 += kPrepThreads * kItems) {
    v4i w[2][kItems];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int u = 0; u < kItems; ++u) {
        const int item = min(item0 + u * kPrepThreads, n_items - 1);  // extra items: ignored
        const int y = item / n_chunks, ch = item - y * n_chunks;
        const long long off = (long long)(y0[s] + y) * a.ishape[s][1] + x0[s] + ch * 16;
        w[s][u] = load_16_bytes(a.img[s], off, img_bytes[s]);
      }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int u = 0; u < kItems; ++u) {
        const int item = item0 + u * kPrepThreads;
        if (item >= n_items) break;
        const int y = item / n_chunks, ch = item - y * n_chunks;
        int isum = 0, isq = 0;  // this item's share of its row's sums
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned v = static_cast<unsigned>(w[s][u][k]);
          const int xb = ch * 16 + k * 4;
          const int keep = min(4, px - xb);  // valid bytes of this dword
          if (keep <= 0) continue;
          unsigned char* dst = pix[s] + y * px + xb;
          if (keep == 4 && ((y * px + xb) & 3) == 0) {
            *reinterpret_cast<unsigned*>(dst) = v;
          } else {
            for (int t = 0; t < keep; ++t) dst[t] = static_cast<unsigned char>(v >> (8 * t));
          }
          const unsigned live = keep == 4 ? 0xffffffffu : (0xffffffffu >> (8 * (4 - keep)));
          isum = static_cast<int>(__builtin_amdgcn_sad_u8(v & live, 0u, isum));
          isq = static_cast<int>(__builtin_amdgcn_udot4(v & live, v & live, isq, false));
          const unsigned lo = v | ~live, hi = v & live;  // dead bytes: 255 for min, 0 for max
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            mn[s] = min(mn[s], static_cast<int>((lo >> (8 * t)) & 0xffu));
            mx[s] = max(mx[s], static_cast<int>((hi >> (8 * t)) & 0xffu));
          }
        }
        sum[s] += isum;
        if (a.prune) {
          const unsigned long long both =
              (static_cast<unsigned long long>(static_cast<unsigned>(isq)) << 32) |
              static_cast<unsigned>(isum);
          atomicAdd(&row_acc[s][y], both);
          atomicAdd(&blk_acc[s][y >> 4][ch], both);
        }
      }
  }
  // wave reduction on the shuffle network, then one LDS exchange across waves
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      mn[s] = min(mn[s], __shfl_xor(mn[s], d, 64));
      mx[s] = max(mx[s], __shfl_xor(mx[s], d, 64));
      sum[s] += __shfl_xor(sum[s], d, 64);
    }
    if (lane == 0) {
      SFM_RED(s, 0, wave) = mn[s];
      SFM_RED(s, 1, wave) = mx[s];
      SFM_RED(s, 2, wave) = sum[s];
    }
  }
  __syncthreads();
  PTICK(1)
  if constexpr (LAZY) {
    // second pass of the fused loop: a thread per column folds the half-band words
    // into the band sums and the column's sum of squares, a thread per row the
    // chunk words into the row's sums (the barrier behind the centres orders them)
    const int NB = py >> 4, NC = px >> 4;
    const unsigned* rowpart = reinterpret_cast<const unsigned*>(smem);
    const unsigned* halfcol = rowpart + 2 * py * NC;
    int* bsum = lazy_bsum;
    for (int t = threadIdx.x; t < 2 * py; t += kPrepThreads) {
      const int u = 2 * py - 1 - t;   // (rows from the other end of the workgroup than the columns)
      const unsigned* rp = rowpart + u * NC;
      unsigned wv[12];
#pragma unroll
      for (int c = 0; c < 12; ++c) wv[c] = c < NC ? rp[c] : 0u;
      unsigned sm = 0, sq = 0;
#pragma unroll
      for (int c = 0; c < 12; ++c) {
        sm += wv[c] & 0xfffu;
        sq += wv[c] >> 12;
      }
      (&row_acc[0][0])[(u >= py ? ROWS : 0) + (u >= py ? u - py : u)] =
          (static_cast<unsigned long long>(sq) << 32) | sm;
    }
    __syncthreads();   // the row words are consumed: the band sums take their place
    for (int t = threadIdx.x; t < 2 * px; t += kPrepThreads) {
      const int s = t >= px ? 1 : 0, x = t - s * px;
      const unsigned* hc = halfcol + s * 2 * NB * px + x;
      unsigned wv[24];
#pragma unroll
      for (int h = 0; h < 24; ++h) wv[h] = h < 2 * NB ? hc[h * px] : 0u;   // (all in flight together)
      unsigned sq = 0;
#pragma unroll
      for (int I = 0; I < 12; ++I)
        if (I < NB) {
          bsum[(s * NB + I) * px + x] = static_cast<int>((wv[2 * I] & 0x7ffu) + (wv[2 * I + 1] & 0x7ffu));
          sq += (wv[2 * I] >> 11) + (wv[2 * I + 1] >> 11);
        }
      // (post patch: mirrored index, like the sweep's column energies)
      col_sq[s][s ? px - 1 - x : x] = static_cast<int>(sq);
    }
  }
  // (LAZY: by two lanes of the last wave, which has no share of the second pass)
  const int ctr_lane = static_cast<int>(threadIdx.x) - (LAZY ? kPrepThreads - 64 : 0);
  if (ctr_lane >= 0 && ctr_lane < 2) {
    const int s = ctr_lane;
    int r_mn = 255, r_mx = 0, r_sum = 0;
    for (int w2 = 0; w2 < kPrepWaves; ++w2) {
      r_mn = min(r_mn, SFM_RED(s, 0, w2));
      r_mx = max(r_mx, SFM_RED(s, 1, w2));
      r_sum += SFM_RED(s, 2, w2);
    }
    SFM_RED(s, 0, 0) = r_mn;
    SFM_RED(s, 1, 0) = r_mx;
    SFM_RED(s, 2, 0) = r_sum;
  }
  if (ctr_lane >= 0 && ctr_lane < 2) {
    const int s = ctr_lane;
    const int mn = SFM_RED(s, 0, 0), mx = SFM_RED(s, 1, 0), sum = SFM_RED(s, 2, 0);
    const float mean =
        a.use_mean ? a.mean : static_cast<float>(sum) / static_cast<float>(py * px);
    int c = static_cast<int>(rintf(fminf(fmaxf(mean, 0.f), 255.f)));
    c = min(max(c, mx - 127), mn + 128);
    s_c[s] = c;
    s_mu[s] = a.use_mean
                  ? a.mean - static_cast<float>(c)
                  : static_cast<float>((static_cast<double>(sum) -
                                        static_cast<double>(c) * py * px) /
                                       (static_cast<double>(py) * px));
    PatchParams* p = &a.pp[b];
    p->y0[s] = y0[s];
    p->x0[s] = x0[s];
    p->c[s] = c;
    p->mu[s] = s_mu[s];
  }
#undef SFM_RED
  __syncthreads();  // `red` (aliased with band_tot) fully consumed
  PTICK(2)
  if (a.prune && wave < 2) {
    // Row energies e[y] = sum_x (pixel - mean)^2 of side `wave` (exact integers
    // in, doubles out) and their prefix sums: lane l owns rows 4 l .. 4 l + 3.
    const int s = wave;
    const double mu = static_cast<double>(s_c[s]) + static_cast<double>(s_mu[s]);
    double e[4], tot = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = 4 * lane + k;
      e[k] = 0.0;
      if (y < py)
        e[k] = fmax(static_cast<double>(row_acc[s][y] >> 32) -
                        2.0 * mu * static_cast<double>(row_acc[s][y] & 0xffffffffull) + mu * mu * px,
                    0.0);
      tot += e[k];
      e[k] = tot;  // inclusive within the lane
    }
    double inc = tot;  // inclusive scan of the lane totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const double o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    const double excl = inc - tot;
    if (lane == 0) row_pre[s][0] = 0.0;
    {
      // the same about the integer centre c (what the matrix operands hold), every
      // fourth row: the correlation kernel bounds the rows a tile has not visited yet
      const long long c = s_c[s];
      unsigned tot_c = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int y = 4 * lane + k;
        if (y < py) {
          const long long sq = static_cast<long long>(row_acc[s][y] >> 32);
          const long long sm = static_cast<long long>(row_acc[s][y] & 0xffffffffull);
          tot_c += static_cast<unsigned>(sq - 2 * c * sm + c * c * px);
        }
      }
      unsigned inc_c = tot_c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc_c, d, 64);
        if (lane >= d) inc_c += o;
      }
      a.tbound[(long long)b * kBoundStride + kRowPre + 64 * s + lane] =
          __uint_as_float(inc_c - tot_c);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = 4 * lane + k;
      if (y < py) row_pre[s][y + 1] = excl + e[k];
    }
  }
  if (a.prune && wave == 2) {
    // inclusive 2-D prefix sums of the four block tables, in place (exact
    // integers; one wave: rows first, then columns)
    // (both fields at once: neither prefix overflows its 32 bits)
    if (lane < 2 * kBlkRows) {  // a lane reads its whole row (loads in flight together)
      const int s = lane >> 4, r = lane & 15;
      unsigned long long v[kBlkCols];
#pragma unroll
      for (int c = 0; c < kBlkCols; ++c) v[c] = blk_acc[s][r][c];
#pragma unroll
      for (int c = 1; c < kBlkCols; ++c) v[c] += v[c - 1];
#pragma unroll
      for (int c = 0; c < kBlkCols; ++c) blk_acc[s][r][c] = v[c];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 32 && (lane & 15) < kBlkCols) {
      const int s = lane >> 4, c = lane & 15;
      unsigned long long v[kBlkRows];
#pragma unroll
      for (int r = 0; r < kBlkRows; ++r) v[r] = blk_acc[s][r][c];
#pragma unroll
      for (int r = 1; r < kBlkRows; ++r) v[r] += v[r - 1];
#pragma unroll
      for (int r = 0; r < kBlkRows; ++r) blk_acc[s][r][c] = v[r];
    }
  }

  const int xl = kPrepCols * lane;
  if (LAZY) {
    // The correction table is built where it is read (kModeSameExactLazyG): of the
    // 20 row tiles of a patch 2.8 ever reach an epilogue, so instead of sweeping
    // Py rows of G (102 KB per patch, 60 % of this kernel's time) the pass leaves
    // the centred column sums above every 16th row, c16[side][I][x] (14 KB), and
    // the four 1-D arrays, which need one wave scan each.  Py, Px multiples of 16,
    // both <= 192 (host).
    const int NB = py >> 4;
    int* bsum = lazy_bsum;   // [2][NB][px]: raw column sums per band of 16 rows
    // (the band sums, the column energies and the block sums were accumulated by
    // the fused loop above; the barriers since then order them)
    int* c16 = a.c16 + b * a.c16_stride;   // [2][NB + 1][px], then T[py + 1]
    if (threadIdx.x < 2 * px) {
      const int s = threadIdx.x >= px ? 1 : 0, x = threadIdx.x - s * px;
      const int c = s_c[s];
      int band_sum[12];
#pragma unroll
      for (int I = 0; I < 12; ++I) band_sum[I] = I < NB ? bsum[(s * NB + I) * px + x] : 0;
      int run = 0;
      int* out = c16 + s * (NB + 1) * px + x;
#pragma unroll
      for (int I = 0; I < 12; ++I) {
        if (I < NB) out[I * px] = run - c * 16 * I;
        run += band_sum[I];
      }
      out[NB * px] = run - c * py;
      bsum[s * NB * px + x] = run;   // the column's raw total (its own entries are consumed)
    }
    __syncthreads();
    PTICK(3)
    const int ca = s_c[0], cb = s_c[1];
    const float mua = s_mu[0], mub = s_mu[1];
    float* aux = a.aux + (long long)b * (4 * a.aux_n + 4);
    float* rrowA = aux;
    float* rrowB = aux + a.aux_n;
    float* rcolA = aux + 2 * a.aux_n;
    float* rcolB = aux + 3 * a.aux_n;
    if (wave == 2 || wave == 3) {
      // wave 2: exclusive prefixes over the centred ROW sums: IA'[y][Px], IB'[y][Px];
      // wave 3: over the centred COLUMN sums: IA'[Py][x], IB'[Py][x]  (lane l owns the
      // entries 3 l .. 3 l + 2, one wave scan per side)
      const bool rows = wave == 2;
      const int len = rows ? py : px, other = rows ? px : py;
      int va[kPrepCols], vb[kPrepCols], sa = 0, sb = 0;
#pragma unroll
      for (int k = 0; k < kPrepCols; ++k) {
        const int i = xl + k;
        int raw_a = 0, raw_b = 0;
        if (i < len) {
          raw_a = rows ? static_cast<int>(row_acc[0][i] & 0xffffffffull) : bsum[i];
          raw_b = rows ? static_cast<int>(row_acc[1][i] & 0xffffffffull) : bsum[NB * px + i];
        }
        va[k] = sa;   // exclusive within the lane
        vb[k] = sb;
        sa += i < len ? raw_a - ca * other : 0;
        sb += i < len ? raw_b - cb * other : 0;
      }
      const int ea = wave_scan_incl(sa) - sa, eb = wave_scan_incl(sb) - sb;
      float* oa = rows ? rrowA : rcolA;
      float* ob = rows ? rrowB : rcolB;
#pragma unroll
      for (int k = 0; k < kPrepCols; ++k) {
        const int i = xl + k;
        const float fa = static_cast<float>(ea + va[k]), fb = static_cast<float>(eb + vb[k]);
        // T = IB'[y][Px], y <= Py, as integers behind the two column-sum tables
        if (rows && i <= len) c16[2 * (NB + 1) * px + i] = eb + vb[k];
        if (i < len) oa[i] = -mub * fa;             // rrowA[yv] / rcolA[xv]
        if (i >= 1 && i <= len) ob[len - i] = mua * fb;   // rrowB[Py - y] / rcolB[Px - x]
        if (rows && i == len) {
          aux[4 * a.aux_n + 0] = -mub * fa;         // -mB' IA'[Py][Px]
          aux[4 * a.aux_n + 1] = -mua * fb;         // -mA' IB'[Py][Px]
        }
      }
    }
  } else {
    // Phase 3a: per-band column totals (band w = rows [w R, (w + 1) R)).
    // Lane l owns the kPrepCols consecutive columns kPrepCols * l + k, so one
    // wave scan over the per-lane totals gives the prefix along x.
    const int R = (py + kPrepWaves - 1) / kPrepWaves;
    const int ra0 = min(wave * R, py), ra1 = min(ra0 + R, py);
  #pragma unroll
    for (int k = 0; k < kPrepCols; ++k) {
      const int x = xl + k;
      int ta = 0, tb = 0, qa = 0, qb = 0;
      if (x < px) {
        // several rows per trip: the byte loads of a trip are in flight together
  #pragma unroll 5
        for (int y = ra0; y < ra1; ++y) {
          const int va = pix[0][y * px + x];
          const int vb = pix[1][y * px + (px - 1 - x)];  // post patch: mirrored columns
          ta += va;
          tb += vb;
          qa += va * va;
          qb += vb * vb;
        }
      }
      band_tot[0][wave][xl + k] = ta;
      band_tot[1][wave][xl + k] = tb;
      if (a.prune && x < px) {
        atomicAdd(&col_sq[0][x], qa);
        atomicAdd(&col_sq[1][x], qb);
      }
    }
    __syncthreads();
    const int ca = s_c[0], cb = s_c[1];
    const float mua = s_mu[0], mub = s_mu[1];
    float* G = a.gtab + (long long)b * py * px;
    float* aux = a.aux + (long long)b * (4 * a.aux_n + 4);
    float* rrowA = aux;
    float* rrowB = aux + a.aux_n;
    float* rcolA = aux + 2 * a.aux_n;
    float* rcolB = aux + 3 * a.aux_n;

    // Phase 3b: running column sums at the first row of the band.
    //   colA = sum of pre rows  [0, yv)      at yv = ra0
    //   colB = sum of post rows [0, py - yv) at yv = ra0
    int colA[kPrepCols], colB[kPrepCols];
  #pragma unroll
    for (int k = 0; k < kPrepCols; ++k) {
      colA[k] = 0;
      colB[k] = 0;
      for (int w2 = 0; w2 < kPrepWaves; ++w2) {
        const int lo = min(w2 * R, py), hi = min(lo + R, py);
        if (hi <= ra0) colA[k] += band_tot[0][w2][xl + k];
        if (hi <= py - ra0) {
          colB[k] += band_tot[1][w2][xl + k];
        } else if (lo < py - ra0) {
          const int x = xl + k;  // partial band: rows [lo, py - ra0)
          if (x < px)
            for (int y = lo; y < py - ra0; ++y) colB[k] += pix[1][y * px + (px - 1 - x)];
        }
      }
    }
    PTICK(3)
    // Sweep.  The last wave also emits the yv == py row (pre-patch totals).
    // The post patch is scanned in MIRRORED column order (lane l owns columns
    // px - 1 - (3 l + k)): the table needs IB[py - yv][px - xv], and
    //     sum_{x < px - xv} b[.][x]  =  TB - (mirrored prefix up to xv),
    // so the lane that holds IA[yv][xv] also holds the matching IB value and a
    // row of G leaves the registers directly -- no transposition through LDS, no
    // intra-wave fences (the first version spent 1.8 k cycles per row on them).
    const int y_end = wave == kPrepWaves - 1 ? py + 1 : ra1;
    for (int yv = ra0; yv < y_end; ++yv) {
      const int yw = py - yv;
      // the pixels that move the column sums to row yv + 1: requested now, added
      // at the end of the trip (their LDS latency hides behind the scans)
      int nxt_a[kPrepCols], nxt_b[kPrepCols];
  #pragma unroll
      for (int k = 0; k < kPrepCols; ++k) {
        const int x = xl + k;
        const bool live = yv < py && x < px;
        nxt_a[k] = live ? pix[0][yv * px + x] : 0;
        nxt_b[k] = live ? pix[1][(yw - 1) * px + (px - 1 - x)] : 0;
      }
      int pa[kPrepCols], pb[kPrepCols];
      int sa = 0, sb = 0;
  #pragma unroll
      for (int k = 0; k < kPrepCols; ++k) {
        sa += xl + k < px ? colA[k] : 0;
        sb += xl + k < px ? colB[k] : 0;
        pa[k] = sa;
        pb[k] = sb;
      }
      const int inc_a = wave_scan_incl(sa), inc_b = wave_scan_incl(sb);
      const int ea = inc_a - sa, eb = inc_b - sb;   // exclusive prefixes of the lane totals
      const int ta = __builtin_amdgcn_readlane(inc_a, 63);  // IrawA[yv][px]
      const int tb = __builtin_amdgcn_readlane(inc_b, 63);  // IrawB[py - yv][px]
      // centred integral images: I'[y][x] = Iraw[y][x] - c y x
      // (c y x < 255 * 256 * 192 < 2^24: 24-bit multiplies, full rate; the 32-bit
      // v_mul_lo_u32 is a quarter-rate instruction and a row had twelve of them)
      const int cay = ca * yv, cby = cb * yw;
      auto ia = [&](int raw, int x) { return static_cast<float>(raw - __mul24(cay, x)); };
      auto ib = [&](int raw, int x) { return static_cast<float>(raw - __mul24(cby, x)); };
      const float ia_px = ia(ta, px), ib_px = ib(tb, px);
      if (yv < py) {
  #pragma unroll
        for (int k = 0; k < kPrepCols; ++k) {
          const int xv = xl + k + 1;
          if (xv < px)
            G[yv * px + xv] = g_entry(mua, mub, ia(ea + pa[k], xv), ib(tb - (eb + pb[k]), px - xv));
        }
        if (lane == 0) {
          G[yv * px] = g_entry(mua, mub, ia(0, 0), ib_px);
          rrowA[yv] = -mub * ia_px;
          rrowB[yv] = mua * ib_px;
        }
      }
      if (yv == 0) {
  #pragma unroll
        for (int k = 0; k < kPrepCols; ++k) {
          const int xv = xl + k + 1;
          if (xv < px) rcolB[xv] = mua * ib(tb - (eb + pb[k]), px - xv);
        }
        if (lane == 0) {
          rcolB[0] = mua * ib_px;
          aux[4 * a.aux_n + 1] = -mua * ib_px;
        }
      }
      if (yv == py) {
  #pragma unroll
        for (int k = 0; k < kPrepCols; ++k) {
          const int xv = xl + k + 1;
          if (xv < px) rcolA[xv] = -mub * ia(ea + pa[k], xv);
        }
        if (lane == 0) {
          rcolA[0] = -mub * ia(0, 0);
          aux[4 * a.aux_n + 0] = -mub * ia_px;
        }
      }
      // advance to row yv + 1
  #pragma unroll
      for (int k = 0; k < kPrepCols; ++k) {
        colA[k] += nxt_a[k];
        colB[k] -= nxt_b[k];
      }
    }
  }
  if (a.prune && threadIdx.x < kBoundTiles) {
    // |surface[dy][dx]| = |sum over the overlap of (a - mean_a)(b - mean_b)|
    //   <= sqrt(E_A(rows of the overlap) E_B(rows of the overlap))     (Cauchy-Schwarz,
    // the column range only shrinks the sums), and the row sets are nested in
    // |dy|: the bound of a tile widened by g rows is the one of its row nearest
    // the centre.  g = tile_guard(p): the rows from which a hot element or the
    // first peak's window can make the peak kernels read the tile -- min_distance
    // and peak_radius rows, 2 peak_radius only for the tiles under a window that
    // the surface border pushed back.  (row_pre was finished before the barrier
    // of phase 3a.)
    const int p = threadIdx.x;
    const int lo = 16 * p - (py - 1), hi = min(lo + 15, py - 1);
    float bound = INFINITY;  // tiles that do not exist are never asked for
    if (lo <= py - 1) {
      const int g = tile_guard(a, p);
      int d = 0;
      if (lo > 0) d = max(0, lo - g);
      if (hi < 0) d = min(0, hi + g);
      // out[dy] = sum_yb a[yb + dy] b[yb]:  dy >= 0: a rows [dy, py), b rows [0, py - dy)
      const double ea = d >= 0 ? row_pre[0][py] - row_pre[0][d] : row_pre[0][py + d];
      const double eb = d >= 0 ? row_pre[1][py - d] : row_pre[1][py] - row_pre[1][-d];
      // margins: float rounding of the correction terms in the kernel (< 1 abs)
      bound = static_cast<float>(sqrt(fmax(ea, 0.0) * fmax(eb, 0.0)) * 1.0005 + 4.0);
    }
    a.tbound[(long long)b * kBoundStride + p] = bound;
  }
  if (a.prune && wave == 1) {
    // The same along x for the outermost prune_k[j] column tiles on either side
    // (the correlation kernel has row-loop variants without them): column
    // energies, lane l owns columns 3 l .. 3 l + 2 (post patch: mirrored).
    const double mua_d = static_cast<double>(s_c[0]) + static_cast<double>(s_mu[0]);
    const double mub_d = static_cast<double>(s_c[1]) + static_cast<double>(s_mu[1]);
    double ea[kPrepCols], eb[kPrepCols];
#pragma unroll
    for (int k = 0; k < kPrepCols; ++k) {
      const int x = xl + k;
      int sa = 0, sb = 0;
      if (LAZY) {   // raw column totals, natural order (post patch: mirrored here)
        const int* tot = lazy_bsum;
        sa = x < px ? tot[x] : 0;
        sb = x < px ? tot[(py >> 4) * px + (px - 1 - x)] : 0;
      } else {
        for (int w2 = 0; w2 < kPrepWaves; ++w2) {
          sa += band_tot[0][w2][x];
          sb += band_tot[1][w2][x];
        }
      }
      ea[k] = x < px ? fmax(col_sq[0][x] - 2.0 * mua_d * sa + mua_d * mua_d * py, 0.0) : 0.0;
      eb[k] = x < px ? fmax(col_sq[1][x] - 2.0 * mub_d * sb + mub_d * mub_d * py, 0.0) : 0.0;
    }
    auto wave_sum = [&](double v) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
      return v;
    };
    // bound of every shift with |dx| >= |d| (d of either sign), all dy:
    //   out[., dx] = sum a[., xa] b[., xa - dx]:  dx >= 0: a cols [dx, px), b cols [0, px - dx)
    auto bound_x = [&](int d) {
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int k = 0; k < kPrepCols; ++k) {
        const int xa = xl + k, xb = px - 1 - (xl + k);  // actual columns of the two entries
        const bool in_a = d >= 0 ? xa >= d : xa < px + d;
        const bool in_b = d >= 0 ? xb < px - d : xb >= -d;
        if (xa < px && in_a) sa += ea[k];
        if (xa < px && in_b) sb += eb[k];
      }
      return static_cast<float>(sqrt(wave_sum(sa) * wave_sum(sb)) * 1.0005 + 4.0);
    };
    float c1d[4];  // 1-D bounds of the outer prune_k[j] column tiles (wave-uniform)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ks = a.prune_k[j];
      c1d[j] = INFINITY;  // no such variant: never taken
      if (ks > 0 && j < 2) {  // (the two widest variants rely on the 2-D bound alone)
        // nearest-to-centre columns of the outer tiles: kx = 16 ks - 1 (left),
        // kx = 16 (nq - ks) (right); dx = kx - (px - 1); widened by the guard
        const int dl = min(0, 16 * ks - px + a.guard_x);
        const int dr = max(0, 16 * (a.nq - ks) - (px - 1) - a.guard_x);
        c1d[j] = fmaxf(bound_x(dl), bound_x(dr));
      }
    }
    if (lane == 0) {
      a.tbound[(long long)b * kBoundStride + kBoundTiles + 0] = c1d[0];
      a.tbound[(long long)b * kBoundStride + kBoundTiles + 1] = c1d[1];
      // |surface - S| = |mA' SB + mB' SA - mA' mB' N| over any overlap, with
      // |SA| <= sqrt(N sum a'^2) (a' = pixel - centre; exact integer totals from
      // the block table): what the seed probe of the correlation kernel subtracts
      const unsigned long long ta = blk_acc[0][(py - 1) >> 4][(px - 1) >> 4];
      const unsigned long long tb2 = blk_acc[1][(py - 1) >> 4][(px - 1) >> 4];
      const double nn = static_cast<double>(py) * px;
      const double ca_d = s_c[0], cb_d = s_c[1];
      const double e_a = fmax(static_cast<double>(ta >> 32) -
                                  2.0 * ca_d * static_cast<double>(ta & 0xffffffffull) + ca_d * ca_d * nn, 0.0);
      const double e_b = fmax(static_cast<double>(tb2 >> 32) -
                                  2.0 * cb_d * static_cast<double>(tb2 & 0xffffffffull) + cb_d * cb_d * nn, 0.0);
      const double ma = fabs(static_cast<double>(s_mu[0])), mb = fabs(static_cast<double>(s_mu[1]));
      a.tbound[(long long)b * kBoundStride + kBoundCorr] = static_cast<float>(
          (ma * sqrt(nn * e_b) + mb * sqrt(nn * e_a) + ma * mb * nn) * 1.001 + 8.0);
    }
    // 2-D: row tile p (rows of its guard-widened innermost shift) x the outer column
    // tiles of prune_k[1..3], from the block energies of the covering block
    // rectangles (rounded outwards: still an upper bound).  Lane = 2 p + side.
    // energy about the mean of the block rectangle [r0, r1) x [c0, c1) of side s
    auto rect_energy = [&](int s, int r0, int r1, int c0, int c1) {
      auto at = [&](int r, int c) {
        return (r < 0 || c < 0) ? 0ull : blk_acc[s][r][c];
      };
      // inclusion-exclusion, field by field
      const unsigned long long lo_mask = 0xffffffffull;
      const unsigned long long a11 = at(r1 - 1, c1 - 1), a01 = at(r0 - 1, c1 - 1);
      const unsigned long long a10 = at(r1 - 1, c0 - 1), a00 = at(r0 - 1, c0 - 1);
      const double sq = static_cast<double>(a11 >> 32) - static_cast<double>(a01 >> 32) -
                        static_cast<double>(a10 >> 32) + static_cast<double>(a00 >> 32);
      const double sm = static_cast<double>(a11 & lo_mask) - static_cast<double>(a01 & lo_mask) -
                        static_cast<double>(a10 & lo_mask) + static_cast<double>(a00 & lo_mask);
      const double cnt = static_cast<double>(min(16 * r1, py) - 16 * r0) *
                         static_cast<double>(min(16 * c1, px) - 16 * c0);
      const double mu = s == 0 ? mua_d : mub_d;
      return fmax(sq - 2.0 * mu * sm + mu * mu * cnt, 0.0);
    };
    const int p = lane >> 1, side = lane & 1;
    const int lo = 16 * p - (py - 1), hi = min(lo + 15, py - 1);
    const int g = tile_guard(a, p);   // (rows; along x the band stays guard_x)
    int dyy = 0;
    if (lo > 0) dyy = max(0, lo - g);
    if (hi < 0) dyy = min(0, hi + g);
    // out[dy][dx] = sum a[yb + dy][xa] b[yb][xa - dx]
    const int ra0 = dyy >= 0 ? dyy : 0, ra1 = dyy >= 0 ? py : py + dyy;
    const int rb0 = dyy >= 0 ? 0 : -dyy, rb1 = dyy >= 0 ? py - dyy : py;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      const int ks = a.prune_k[j];
      float bound = INFINITY;
      if (ks > 0 && lo <= py - 1) {
        const int dxx = side == 0 ? min(0, 16 * ks - px + a.guard_x)
                                  : max(0, 16 * (a.nq - ks) - (px - 1) - a.guard_x);
        const int ca0 = dxx >= 0 ? dxx : 0, ca1 = dxx >= 0 ? px : px + dxx;
        const int cb0 = dxx >= 0 ? 0 : -dxx, cb1 = dxx >= 0 ? px - dxx : px;
        double ea2 = 0.0, eb2 = 0.0;
        if (ca1 > ca0 && ra1 > ra0)
          ea2 = rect_energy(0, ra0 >> 4, (ra1 + 15) >> 4, ca0 >> 4, (ca1 + 15) >> 4);
        if (cb1 > cb0 && rb1 > rb0)
          eb2 = rect_energy(1, rb0 >> 4, (rb1 + 15) >> 4, cb0 >> 4, (cb1 + 15) >> 4);
        bound = static_cast<float>(sqrt(ea2 * eb2) * 1.0005 + 4.0);
      }
      bound = fmaxf(bound, __shfl_xor(bound, 1, 64));  // left and right outer tiles
      bound = fminf(bound, c1d[j]);
      if (side == 0 && p < kBoundTiles)
        a.tbound[(long long)b * kBoundStride + 32 + 3 * p + (j - 1)] = bound;
    }
  }
#ifdef SFM_MFMA_TIMING
  PTICK(4)
  if (b == 100 && lane == 0 && (wave == 0 || wave == WAVES - 1))
    printf("PREP wave %d: load %lld reduce %lld bands %lld sweep %lld\n", wave, pt[1] - pt[0],
           pt[2] - pt[1], pt[3] - pt[2], pt[4] - pt[3]);
#endif
}

constexpr int kPrepWavesAlone = 8;   // bands of rows swept concurrently (stand-alone kernel)
// LAZY: three workgroups per CU (51 KB of LDS each; <= 80 VGPRs at six waves per SIMD)
constexpr int kPrepLazyWavesPerSimd = 6;
template <bool LAZY>
__global__ void __launch_bounds__(64 * kPrepWavesAlone, LAZY ? kPrepLazyWavesPerSimd : 1)
mfma_prep_same_kernel(MfmaArgs a) {
  if (a.work_counter && blockIdx.x == 0 && threadIdx.x == 0)
    reset_patch_queue(a);
  if (a.clk && blockIdx.x == 0 && threadIdx.x == 0) a.clk[2] = a.clk[3] = a.clk[4] = 0;  // tile counts
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ PrepTables<kPrepWavesAlone, kBoundRows, LAZY> tables;
  prep_same_body<kPrepWavesAlone, kBoundRows, LAZY>(a, blockIdx.x, smem, &tables);
}

// Masked path prep: clamped origins in image and mask, masked mean, centre.
__global__ void __launch_bounds__(kThreads) mfma_prep_masked_kernel(MfmaArgs a) {
  __shared__ int red[4][kThreads];
  const int b = blockIdx.x, s = blockIdx.y;
  const int py = s == 0 ? a.P[0] : a.Q[0];
  const int px = s == 0 ? a.P[1] : a.Q[1];
  const int H = a.ishape[s][0], W = a.ishape[s][1];
  const int sy = a.starts[s][b * 2 + 0], sx = a.starts[s][b * 2 + 1];
  const int y0 = min(max(sy, 0), H - py), x0 = min(max(sx, 0), W - px);
  const unsigned char* mask = a.mask[s];
  const int MH = a.mshape[s][0], MW = a.mshape[s][1];
  const int my0 = mask ? min(max(sy, 0), MH - py) : 0;
  const int mx0 = mask ? min(max(sx, 0), MW - px) : 0;
  int mn = 255, mx = 0, sum = 0, cnt = 0;
  // 16 pixels per work item: one 16-byte load of pixels and one of the mask
  // (byte loads only in the last, partial item of a row)
  const int n_chunks = (px + 15) >> 4;
  const int n_items = py * n_chunks;
  auto tally = [&](const unsigned* pw, const unsigned* mw, int nx) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int v = static_cast<int>((pw[j >> 2] >> (8 * (j & 3))) & 0xffu);
      const bool ok = j < nx && ((mw[j >> 2] >> (8 * (j & 3))) & 0xffu) == 0;
      mn = ok ? min(mn, v) : mn;
      mx = ok ? max(mx, v) : mx;
      sum += ok ? v : 0;
      cnt += ok ? 1 : 0;
    }
  };
  if ((px & 15) == 0) {
    // whole 16-byte items only: four items per round, their eight loads issued
    // as one straight-line group (items past the end repeat the last one and
    // are ignored; without a mask the image stands in and its bytes are dropped)
    const unsigned char* mbase = mask ? mask + (long long)my0 * MW + mx0
                                      : a.img[s] + (long long)y0 * W + x0;
    const long long mpitch = mask ? MW : W;
    const unsigned mkeep = mask ? 0xffffffffu : 0u;
    constexpr int kRound = 4;
    for (int item0 = threadIdx.x; item0 < n_items; item0 += kThreads * kRound) {
      unsigned pw[kRound][4], mw[kRound][4];
#pragma unroll
      for (int u = 0; u < kRound; ++u) {
        const int item = min(item0 + u * kThreads, n_items - 1);
        const int y = item / n_chunks, x = 16 * (item - y * n_chunks);
        __builtin_memcpy(pw[u], a.img[s] + (long long)(y0 + y) * W + x0 + x, 16);
        __builtin_memcpy(mw[u], mbase + y * mpitch + x, 16);
      }
#pragma unroll
      for (int u = 0; u < kRound; ++u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) mw[u][k] &= mkeep;
        tally(pw[u], mw[u], item0 + u * kThreads < n_items ? 16 : 0);
      }
    }
  } else {
    for (int item = threadIdx.x; item < n_items; item += kThreads) {
      const int y = item / n_chunks, ch = item - y * n_chunks;
      const int x = 16 * ch, nx = min(16, px - x);
      const unsigned char* ip = a.img[s] + (long long)(y0 + y) * W + x0 + x;
      const unsigned char* mp = mask ? mask + (long long)(my0 + y) * MW + mx0 + x : nullptr;
      unsigned pw[4] = {0, 0, 0, 0}, mw[4] = {0, 0, 0, 0};
      if (nx == 16) {
        __builtin_memcpy(pw, ip, 16);
        if (mp) __builtin_memcpy(mw, mp, 16);
      } else {
        for (int j = 0; j < nx; ++j) {
          pw[j >> 2] |= static_cast<unsigned>(ip[j]) << (8 * (j & 3));
          if (mp) mw[j >> 2] |= static_cast<unsigned>(mp[j]) << (8 * (j & 3));
        }
      }
      tally(pw, mw, nx);
    }
  }
  red[0][threadIdx.x] = mn;
  red[1][threadIdx.x] = mx;
  red[2][threadIdx.x] = sum;
  red[3][threadIdx.x] = cnt;
  __syncthreads();
  for (int k = kThreads / 2; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      red[0][threadIdx.x] = min(red[0][threadIdx.x], red[0][threadIdx.x + k]);
      red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + k]);
      red[2][threadIdx.x] += red[2][threadIdx.x + k];
      red[3][threadIdx.x] += red[3][threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mn = red[0][0];
    mx = red[1][0];
    sum = red[2][0];
    cnt = red[3][0];
    PatchParams* p = &a.pp[b];
    p->y0[s] = y0;
    p->x0[s] = x0;
    p->my0[s] = my0;
    p->mx0[s] = mx0;
    if (a.nvalid) a.nvalid[b * 2 + s] = cnt;
    int c = 128;
    float mu = 0.f;
    if (cnt > 0) {
      // nanmean over the unmasked pixels (flow_field.py:340-347)
      const float mean =
          a.use_mean ? a.mean : static_cast<float>(sum) / static_cast<float>(cnt);
      c = static_cast<int>(rintf(fminf(fmaxf(mean, 0.f), 255.f)));
      c = min(max(c, mx - 127), mn + 128);
      mu = a.use_mean ? a.mean - static_cast<float>(c)
                      : static_cast<float>((static_cast<double>(sum) -
                                            static_cast<double>(c) * cnt) /
                                           static_cast<double>(cnt));
    }
    p->c[s] = c;
    p->mu[s] = mu;
  }
}

// One element of the Padfield assembly (flow_field.py:113-131).  Inputs are
// exact integers: xc = sum a'b', s_a / s_b = sums of a' / b', sq_a / sq_b =
// sums of a'^2 / b'^2, n = number of pixel pairs, all over the pairs valid on
// both sides at this shift (a', b' = pixel - integer centre).
//
// The reference subtracts the masked patch means first and then removes the
// overlap means again; in exact arithmetic the patch means (and the centres)
// cancel, and multiplying numerator and denominator by n leaves
//     NCC = (n xc - s_a s_b) / sqrt((n sq_a - s_a^2)(n sq_b - s_b^2)),
// three differences of integers below 2^53: exact in double, no division and
// no cancellation error.  `den` (the reference's denominator, = den_n / n) is
// only compared with the batch tolerance, so float precision is enough for it.
struct PadfieldTerms {
  double num_n;  // n * numerator
  float den_n;   // n * denominator
  float den, ov;
};

__device__ __forceinline__ PadfieldTerms padfield_terms(int xc, int s_a, int s_b, int n,
                                                        double sq_a, double sq_b) {
  PadfieldTerms t;
  const double nd = n, sa = s_a, sb = s_b;
  const double pd = fmax(fma(nd, sq_a, -(sa * sa)), 0.0);
  const double cd = fmax(fma(nd, sq_b, -(sb * sb)), 0.0);
  t.num_n = fma(nd, static_cast<double>(xc), -(sa * sb));
  t.den_n = __builtin_amdgcn_sqrtf(static_cast<float>(pd * cd));  // 1 ulp
  t.ov = fmaxf(static_cast<float>(n), 1.1920928955078125e-07f);
  t.den = t.den_n * __builtin_amdgcn_rcpf(t.ov);
  return t;
}

// SQHI / SQLO products back to the sum of squares (exact in double).
__device__ __forceinline__ double square_sum(int hi, int lo, int n) {
  return 128.0 * static_cast<double>(hi) + static_cast<double>(lo) +
         8192.0 * static_cast<double>(n);
}

// One workgroup: classes and the list of extra passes in patch order.
__global__ void __launch_bounds__(1024) masked_classify_kernel(MaskedFastArgs g) {
  __shared__ int wsum[16];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int b0 = 0; b0 < g.batch; b0 += 1024) {
    const int b = b0 + threadIdx.x;
    int cls = 0;
    if (b < g.batch)
      cls = g.all_passes ? 3
                         : (g.nvalid[2 * b] < g.P[0] * g.P[1] ? 1 : 0) +
                               (g.nvalid[2 * b + 1] < g.Q[0] * g.Q[1] ? 2 : 0);
    const int k = b < g.batch ? (cls == 0 ? 0 : cls == 3 ? 7 : 3) : 0;
    const int incl = wave_scan_incl(k);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = s_base;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    const int first = base + incl - k;
    if (b < g.batch) {
      g.cls[b] = cls;
      g.first[b] = first;
      // class 1: VALID_A * {VAL, SQHI, SQLO}_B; class 2: {VAL, SQHI, SQLO}_A * VALID_B
      for (int j = 0; j < k; ++j) {
        const int pass =
            cls == 3 ? 1 + j : cls == 1 ? (j == 0 ? 2 : 5 + j) : (j == 0 ? 1 : 3 + j);
        g.items[first + j] = b * 8 + pass;
      }
    }
    __syncthreads();
    if (threadIdx.x == 1023) s_base = base + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *g.n_items = s_base;
  // A lower bound of the batch maximum of the overlap, known before any product:
  // at the zero shift a same-size patch pair overlaps in at least
  // nvalid_A + nvalid_B - Py Px pixels (= Py Px for a clean pair).  The raw pass of
  // a' * b' uses it to leave out row tiles that the overlap rule zeroes anyway.
  // One bound per reference batch (`group` patches; zeroed by the host).
  if (g.P[0] == g.Q[0] && g.P[1] == g.Q[1])
    for (int b0 = 0; b0 < g.batch; b0 += 1024) {
      const int b = b0 + threadIdx.x;
      int lb = 0, gid = -1;
      if (b < g.batch) {
        lb = g.nvalid[2 * b] + g.nvalid[2 * b + 1] - g.P[0] * g.P[1];
        gid = b / g.group;
      }
      // one atomic per wave where its 64 patches share a batch (same-address atomics
      // serialise in the L2)
      const int g0 = __builtin_amdgcn_readfirstlane(gid);
      if (__ballot(gid != g0) == 0) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) lb = max(lb, __shfl_xor(lb, d, 64));
        if (lane == 0 && g0 >= 0 && lb > 0) atomicMax(&g.ov_lb[g0], lb);
      } else if (gid >= 0 && lb > 0) {
        atomicMax(&g.ov_lb[gid], lb);
      }
    }
}

// Inclusive integral images T[y][x] = sum over rows <= y, columns <= x of the
// planes a patch's box sums need (masked pixels count as 0):
//   class 0: a', a'^2, b', b'^2;  class 1: a', a'^2, valid_a;  class 2: b', b'^2, valid_b
// Wave w of the workgroup builds table w: a lane owns four adjacent columns
// (one dword of pixels per row), so a row costs one wave scan; the running
// column sums of the row prefixes stay in registers while it walks down.
__global__ void __launch_bounds__(kThreads) masked_tables_kernel(MaskedFastArgs g) {
  const int b = blockIdx.x;
  const int cls = g.cls[b];
  const int lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (cls == 3 || (cls != 0 && t == 3)) return;
  const int s = cls == 0 ? t >> 1 : cls - 1;
  const int kind = cls == 0 ? (t & 1) : t;  // 0 value, 1 square, 2 valid
  const int py = s ? g.Q[0] : g.P[0], px = s ? g.Q[1] : g.P[1];
  const PatchParams pp = g.pp[b];
  const int c = pp.c[s];
  const int W = g.ishape[s][1], MW = g.mshape[s][1];
  const unsigned char* src = g.img[s] + (long long)pp.y0[s] * W + pp.x0[s];
  const unsigned char* msk =
      cls != 0 && g.mask[s] ? g.mask[s] + (long long)pp.my0[s] * MW + pp.mx0[s] : nullptr;
  int* T = g.tab + ((long long)b * 4 + t) * g.tab_elems;
  constexpr int kAhead = 8;
  // Columns 4 lane .. 4 lane + 3; a lane whose dword would cross the end of the
  // row fetches the last whole dword of the row instead (unconditional loads: a
  // load under a per-lane condition ends up in its own block and the loads of
  // a batch would be waited for one by one).
  const int x0 = 4 * lane;
  const int xl = min(x0, max(px - 4, 0));
  const bool vec = (px & 3) == 0 && px >= 4;
  int acc[4] = {0, 0, 0, 0};
  // The loads of a batch of rows must be ONE straight-line group (any branch
  // between them, even a wave-uniform one, gets a wait of its own: measured,
  // eight serial round trips per batch): the mask pointer falls back to the
  // image (its bytes are then ignored) and narrow patches take another loop.
  // (Cutting the rows into bands swept by more waves was measured slower:
  // 192 vs 127 us per 1024 patches.)
  const unsigned char* mbase = msk ? msk : src;
  const long long mpitch = msk ? MW : W;
  const unsigned mkeep = msk ? 0xffffffffu : 0u;
  const bool wide = px >= 4;
  for (int y0 = 0; y0 < py; y0 += kAhead) {
    unsigned pw[kAhead], mw[kAhead];
    if (wide) {
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int yc = min(y0 + u, py - 1);
        __builtin_memcpy(&pw[u], src + (long long)yc * W + xl, 4);
        __builtin_memcpy(&mw[u], mbase + yc * mpitch + xl, 4);
      }
#pragma unroll
      for (int u = 0; u < kAhead; ++u) mw[u] &= mkeep;
    } else {  // patches narrower than a dword: byte by byte
      for (int u = 0; u < kAhead; ++u) {
        const int yc = min(y0 + u, py - 1);
        pw[u] = mw[u] = 0;
        for (int j = 0; j < px; ++j) {
          pw[u] |= static_cast<unsigned>(src[(long long)yc * W + j]) << (8 * j);
          if (msk) mw[u] |= static_cast<unsigned>(msk[(long long)yc * MW + j]) << (8 * j);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int y = y0 + u;
      const bool row_in = y < py;  // (rows beyond the patch repeat the last one: not stored)
      int v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // a re-based dword (row tail) holds column x0 + j in byte j + x0 - xl
        const bool in = x0 + j < px;
        const int sh = in ? 8 * (j + x0 - xl) : 0;
        const int pv = static_cast<int>((pw[u] >> sh) & 0xffu) - c;
        const bool valid = in && ((mw[u] >> sh) & 0xffu) == 0;
        const int val = kind == 2 ? 1 : kind == 1 ? pv * pv : pv;
        v[j] = valid ? val : 0;
      }
      const int p1 = v[0] + v[1], p2 = p1 + v[2], p3 = p2 + v[3];
      const int incl = wave_scan_incl(p3);
      const int excl = incl - p3;
      acc[0] += excl + v[0];
      acc[1] += excl + p1;
      acc[2] += excl + p2;
      acc[3] += incl;
      if (vec) {
        if (row_in && x0 < px)
          *reinterpret_cast<v4i*>(T + y * px + x0) = v4i{acc[0], acc[1], acc[2], acc[3]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (row_in && x0 + j < px) T[y * px + x0 + j] = acc[j];
      }
    }
  }
}

// Batch maxima of a CLEAN same-size pair (class 0, P == Q) without visiting its
// 4 P^2 shifts.  den(dy, dx) = sqrt(SSD_A(rect) SSD_B(rect)) in exact arithmetic,
// SSD = sum of squared deviations from the rectangle's own mean, which only grows
// with the rectangle; the overlap rectangles of a shift are (rows of dy) x (columns
// of dx) on both sides, so  den(dy, dx) <= min(den(dy, 0), den(0, dx)).  The float
// value the assembly computes (padfield_terms: < 2^-20 relative error) can therefore
// exceed the largest value found on the two axes only where BOTH axis values are
// within 1e-5 of it -- for textured patches the zero shift alone.  The kernel
// evaluates the axes (row / column totals of the integral images), then every
// shift of the candidate cross product with the assembly's own expression, and
// merges the maximum: the same bits as the sweep over all shifts
// (masked_phase_rows<0, false>), which these patches then skip.  The overlap
// maximum of a clean pair is Py Px (zero shift).  One wave per patch.
constexpr int kAxisMaxPairs = 2048;

__device__ __forceinline__ float axis_den(const int (*I)[kAxisMaxLen + 1], int P, int other,
                                          int d) {
  // shift d along one axis, zero along the other: side A rows [a0, a1), side B rows
  // [a0 - d, a1 - d); I[t][i] = total of rows (columns) < i of table t
  const int a0 = max(0, d), a1 = min(P, P + d);
  const int s_a = I[0][a1] - I[0][a0];
  const double sq_a = static_cast<double>(I[1][a1] - I[1][a0]);
  const int s_b = I[2][a1 - d] - I[2][a0 - d];
  const double sq_b = static_cast<double>(I[3][a1 - d] - I[3][a0 - d]);
  return padfield_terms(0, s_a, s_b, (a1 - a0) * other, sq_a, sq_b).den;
}

__global__ void __launch_bounds__(64) masked_axis_max_kernel(MaskedFastArgs g) {
  const int b = blockIdx.x;
  if (g.cls[b] != 0) return;
  __shared__ int R[4][kAxisMaxLen + 1], Cc[4][kAxisMaxLen + 1];
  __shared__ short cand[2][2 * kAxisMaxLen];
  __shared__ int n_cand[2];
  const int lane = threadIdx.x;
  const int Py = g.P[0], Px = g.P[1];
  const int* tab = g.tab + (long long)b * 4 * g.tab_elems;
  // totals of the rows / columns before index i (inclusive tables: last column / row)
  for (int i = lane; i < Py; i += 64)
#pragma unroll
    for (int t = 0; t < 4; ++t) R[t][i + 1] = tab[t * g.tab_elems + (long long)i * Px + Px - 1];
  for (int i = lane; i < Px; i += 64)
#pragma unroll
    for (int t = 0; t < 4; ++t) Cc[t][i + 1] = tab[t * g.tab_elems + (long long)(Py - 1) * Px + i];
  if (lane < 4) R[lane][0] = Cc[lane][0] = 0;
  if (lane < 2) n_cand[lane] = 0;
  __syncthreads();
  constexpr int kPer = (2 * kAxisMaxLen + 63) / 64;   // shifts per lane and axis
  float dy_den[kPer], dx_den[kPer];
  float amax = 0.f;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int ky = lane + 64 * u, kx = lane + 64 * u;
    dy_den[u] = ky < 2 * Py - 1 ? axis_den(R, Py, Px, ky - (Py - 1)) : -1.f;
    dx_den[u] = kx < 2 * Px - 1 ? axis_den(Cc, Px, Py, kx - (Px - 1)) : -1.f;
    amax = fmaxf(amax, fmaxf(dy_den[u], dx_den[u]));
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
  // candidate rows / columns: axis value within 1e-5 of the axis maximum
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    if (dy_den[u] >= 0.f && dy_den[u] * 1.00001f >= amax)
      cand[0][atomicAdd(&n_cand[0], 1)] = static_cast<short>(lane + 64 * u - (Py - 1));
    if (dx_den[u] >= 0.f && dx_den[u] * 1.00001f >= amax)
      cand[1][atomicAdd(&n_cand[1], 1)] = static_cast<short>(lane + 64 * u - (Px - 1));
  }
  __syncthreads();
  float mden = amax;
  const int ny_c = n_cand[0], nx_c = n_cand[1];
  // (amax == 0: every denominator is exactly 0.)  A patch with wide flat margins
  // can have thousands of candidate shifts: it takes the ordinary sweep instead.
  const bool sweep = amax > 0.f && ny_c * nx_c > kAxisMaxPairs;
  if (lane == 0) g.sweep0[b] = sweep ? 1 : 0;
  if (sweep) return;
  if (amax > 0.f && ny_c * nx_c > 1) {
    // the shifts off the axes that could reach the maximum: the assembly's expression
    // on the four box sums (inclusive tables: corner (y1 - 1, x1 - 1) etc.)
    for (int i = lane; i < ny_c * nx_c; i += 64) {
      const int dy = cand[0][i / nx_c], dx = cand[1][i % nx_c];
      const int ya0 = max(0, dy), ya1 = min(Py, Py + dy);
      const int xa0 = max(0, dx), xa1 = min(Px, Px + dx);
      int box[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int* T = tab + t * g.tab_elems;
        const int y0 = t < 2 ? ya0 : ya0 - dy, y1 = t < 2 ? ya1 : ya1 - dy;
        const int x0 = t < 2 ? xa0 : xa0 - dx, x1 = t < 2 ? xa1 : xa1 - dx;
        int v = T[(long long)(y1 - 1) * Px + x1 - 1];
        if (y0 > 0) v -= T[(long long)(y0 - 1) * Px + x1 - 1];
        if (x0 > 0) v -= T[(long long)(y1 - 1) * Px + x0 - 1];
        if (y0 > 0 && x0 > 0) v += T[(long long)(y0 - 1) * Px + x0 - 1];
        box[t] = v;
      }
      mden = fmaxf(mden, padfield_terms(0, box[0], box[2], (ya1 - ya0) * (xa1 - xa0),
                                        static_cast<double>(box[1]), static_cast<double>(box[3])).den);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mden = fmaxf(mden, __shfl_xor(mden, d, 64));
  }
  if (lane == 0) {
    unsigned int* mx = g.maxima + 2 * (b / g.group);
    const unsigned db = __float_as_uint(mden);
    const unsigned ob = __float_as_uint(static_cast<float>(Py * Px));
    if (db > __atomic_load_n(&mx[0], __ATOMIC_RELAXED)) atomicMax(&mx[0], db);
    if (ob > __atomic_load_n(&mx[1], __ATOMIC_RELAXED)) atomicMax(&mx[1], ob);
  }
}

// Padfield assembly from the integer data.  FINAL = false: batch maxima of the
// denominator and the overlap only; FINAL = true: the normalised surface
// (flow_field.py:132-156) with the tolerance / overlap threshold of those maxima.
// Grid (row blocks, batch); a wave takes whole surface rows; where box sums
// are used it first differences the integral images over the row range of the
// shift into 1-D arrays in LDS (D[x] = sum over those rows, columns < x), so
// that a box sum is two LDS reads.
constexpr int kAsmMaxCols = 208;

struct PhaseOut {
  float mden, mov, rmax;
};

// The rows of one wave for a patch of class CLS (compile-time: every register
// array below is indexed with constants).  D0 / D1: this wave's LDS arrays,
//   class 0: D0[x] = (a', a'^2) sums, D1[x] = (b', b'^2) sums,
//   class 1: D0[x] = (a', a'^2),      D1[x].x = valid_a count,
//   class 2: D0[x] = (b', b'^2),      D1[x].x = valid_b count
// over the row range of the shift and columns < x.
template <int CLS, bool FINAL>
__device__ __forceinline__ void masked_phase_rows(const MaskedFastArgs& g, int b,
                                                  int row_block, int2* D0, int2* D1,
                                                  float tol, float px_thr,
                                                  PhaseOut* po) {
  constexpr int kTabs = CLS == 0 ? 4 : CLS == 3 ? 0 : 3;
  constexpr int kRaw = CLS == 0 ? 1 : CLS == 3 ? 8 : 4;  // product surfaces read
  constexpr int kTabCols = 3;  // table columns per lane: Px <= 192
  constexpr int kOutCols = 5;  // surface columns per lane: Sx <= 319 (patches <= 160 wide)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int Py = g.P[0], Px = g.P[1], Qy = g.Q[0], Qx = g.Q[1];
  const int Sy = g.S[0], Sx = g.S[1];
  const int* raw0 = g.raw0 + (long long)b * g.raw_stride;
  const int* rawd = g.rawd + (long long)g.first[b] * g.raw_stride;
  const int* tab = g.tab + (long long)b * 4 * g.tab_elems;
  // Every global load of a row is issued before the first one is used: the
  // integral-image rows of the NEXT surface row travel while this one is
  // assembled, and the product surfaces of a row are requested together.
  int thi[kTabs ? kTabs : 1][kTabCols], tlo[kTabs ? kTabs : 1][kTabCols];
  const int row_base = (row_block * kWaves + wave) * kAsmRowsPerWave;
  // FINAL: a surface row whose largest possible overlap, ny * Qx, is below the
  // overlap threshold (flow_field.py:151-155) is zero whatever its terms are
  // (overlap <= ny * Qx for every class): nothing is loaded or assembled for it.
  // With a clean patch in the batch the threshold is 0.3 Py Px: 30 % of the rows.
  auto dead_row = [&](int ky) {
    if (!FINAL || !g.dead_rows) return false;
    const int dy = ky - (Qy - 1);
    const int ny = min(Py, Qy + dy) - max(0, dy);
    return static_cast<float>(ny * Qx) < px_thr;
  };
  auto fetch_tables = [&](int ky) {
    if (ky >= Sy || dead_row(ky)) return;
    const int dy = ky - (Qy - 1);
    const int ya0 = max(0, dy), ya1 = min(Py, Qy + dy);
#pragma unroll
    for (int j = 0; j < kTabs; ++j) {
      // side of table j: class 0: A A B B, class 1: A A A, class 2: B B B
      const bool side_b = CLS == 2 || (CLS == 0 && j >= 2);
      const int w = side_b ? Qx : Px;
      const int y0 = side_b ? ya0 - dy : ya0, y1 = side_b ? ya1 - dy : ya1;
      const int* T = tab + j * g.tab_elems;
#pragma unroll
      for (int k = 0; k < kTabCols; ++k) {
        // (clamped addresses, unconditional loads: see masked_tables_kernel)
        const int x = min(lane + 64 * k, w - 1);
        thi[j][k] = T[(y1 - 1) * w + x];  // y1 >= 1 on every valid row
        const int lo = T[max(y0 - 1, 0) * w + x];
        tlo[j][k] = y0 > 0 ? lo : 0;
      }
    }
  };
  // product surfaces: row r of the current surface row, also one row ahead
  int rv[kRaw][kOutCols];
  auto fetch_raw = [&](int ky) {
    if (ky >= Sy || dead_row(ky)) return;
    const long long row = (long long)ky * g.pitch;
#pragma unroll
    for (int c = 0; c < kOutCols; ++c) {
      const int kx = lane + 64 * c;
#pragma unroll
      for (int q = 0; q < kRaw; ++q) {
        if (!FINAL && q == 0) continue;  // the maxima do not involve a' * b'
        const int* src = q == 0 ? raw0 : rawd + (long long)(q - 1) * g.raw_stride;
        rv[q][c] = src[row + min(kx, Sx - 1)];
      }
    }
  };
  if (kTabs) fetch_tables(row_base);
  fetch_raw(row_base);
  for (int i = 0; i < kAsmRowsPerWave; ++i) {
    const int ky = row_base + i;
    const bool row_ok = ky < Sy;
    const int dy = ky - (Qy - 1);
    const int ya0 = max(0, dy), ya1 = min(Py, Qy + dy);
    const int ny = ya1 - ya0;
    const bool dead = row_ok && dead_row(ky);
    if (kTabs) {
      __syncthreads();  // previous row's arrays consumed
      if (row_ok && !dead) {
#pragma unroll
        for (int k = 0; k < kTabCols; ++k) {
          const int x = lane + 64 * k + 1;
          D0[x] = make_int2(thi[0][k] - tlo[0][k], thi[1 % (kTabs ? kTabs : 1)][k] -
                                                       tlo[1 % (kTabs ? kTabs : 1)][k]);
          D1[x] = make_int2(thi[2 % (kTabs ? kTabs : 1)][k] - tlo[2 % (kTabs ? kTabs : 1)][k],
                            kTabs == 4 ? thi[3 % (kTabs ? kTabs : 1)][k] -
                                             tlo[3 % (kTabs ? kTabs : 1)][k]
                                       : 0);
        }
        if (lane == 0) {
          D0[0] = make_int2(0, 0);
          D1[0] = make_int2(0, 0);
        }
      }
      __syncthreads();
      if (i + 1 < kAsmRowsPerWave) fetch_tables(ky + 1);
    }
    if (!row_ok) continue;
    const long long row = (long long)ky * g.pitch;
    if (dead) {  // (FINAL only) the whole row is zero
      if (i + 1 < kAsmRowsPerWave) fetch_raw(ky + 1);
#pragma unroll
      for (int c = 0; c < kOutCols; ++c) {
        const int kx = lane + 64 * c;
        if (kx < Sx) g.out[(long long)b * g.elems + row + kx] = 0.f;
      }
      po->rmax = fmaxf(po->rmax, 0.f);
      continue;
    }
    // this row's products move to `cur`; the next row's loads are issued now
    int cur[kRaw][kOutCols];
#pragma unroll
    for (int c = 0; c < kOutCols; ++c)
#pragma unroll
      for (int q = 0; q < kRaw; ++q) cur[q][c] = (!FINAL && q == 0) ? 0 : rv[q][c];
    if (i + 1 < kAsmRowsPerWave) fetch_raw(ky + 1);
#pragma unroll
    for (int c = 0; c < kOutCols; ++c) {
      const int kx = lane + 64 * c;
      if (kx < Sx) {
        const int dx = kx - (Qx - 1);
        const int xa0 = max(0, dx), xa1 = min(Px, Qx + dx);
        const int xb0 = xa0 - dx, xb1 = xa1 - dx;
        int s_a, s_b, n;
        double sq_a, sq_b;
        if (CLS == 0) {
          const int2 a1 = D0[xa1], a0 = D0[xa0], b1 = D1[xb1], b0 = D1[xb0];
          n = ny * (xa1 - xa0);
          s_a = a1.x - a0.x;
          sq_a = a1.y - a0.y;
          s_b = b1.x - b0.x;
          sq_b = b1.y - b0.y;
        } else if (CLS == 1) {
          const int2 a1 = D0[xa1], a0 = D0[xa0];
          n = D1[xa1].x - D1[xa0].x;
          s_a = a1.x - a0.x;
          sq_a = a1.y - a0.y;
          s_b = cur[1 % kRaw][c];
          sq_b = square_sum(cur[2 % kRaw][c], cur[3 % kRaw][c], n);
        } else if (CLS == 2) {
          const int2 b1 = D0[xb1], b0 = D0[xb0];
          n = D1[xb1].x - D1[xb0].x;
          s_b = b1.x - b0.x;
          sq_b = b1.y - b0.y;
          s_a = cur[1 % kRaw][c];
          sq_a = square_sum(cur[2 % kRaw][c], cur[3 % kRaw][c], n);
        } else {
          s_a = cur[1 % kRaw][c];
          s_b = cur[2 % kRaw][c];
          n = cur[3 % kRaw][c];
          sq_a = square_sum(cur[4 % kRaw][c], cur[5 % kRaw][c], n);
          sq_b = square_sum(cur[6 % kRaw][c], cur[7 % kRaw][c], n);
        }
        const PadfieldTerms t = padfield_terms(cur[0][c], s_a, s_b, n, sq_a, sq_b);
        if (FINAL) {
          float v = t.den > tol ? static_cast<float>(t.num_n) / t.den_n : 0.f;
          v = fminf(fmaxf(v, -1.f), 1.f);
          if (t.ov < px_thr) v = 0.f;
          g.out[(long long)b * g.elems + row + kx] = v;
          po->rmax = fmaxf(po->rmax, v);
        } else {
          po->mden = fmaxf(po->mden, t.den);
          po->mov = fmaxf(po->mov, t.ov);
        }
      }
    }
  }
}

// End of an assembly workgroup: surface maximum (FINAL) or batch maxima.
template <bool FINAL>
__device__ __forceinline__ void phase_finish(const MaskedFastArgs& g, int b, int row_block,
                                             const PhaseOut& po) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float mden = po.mden, mov = po.mov, rmax = po.rmax;
  if (FINAL) {
    // surface maximum for the peak search (monotonic uint image of the float)
    if (g.smax) {
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, d, 64));
      if (g.blkmax) {
        // and the maximum of this workgroup's 32 rows: the peak sweep skips blocks
        // that hold nothing above its threshold
        __shared__ float bred[kWaves];
        if (lane == 0) bred[wave] = rmax;
        __syncthreads();
        if (threadIdx.x == 0) {
          float m = bred[0];
          for (int w = 1; w < kWaves; ++w) m = fmaxf(m, bred[w]);
          g.blkmax[(long long)b * g.row_blocks + row_block] = m;
        }
      }
      if (lane == 0 && rmax > -INFINITY) {
        const unsigned u = __float_as_uint(rmax);
        const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        if (o > __atomic_load_n(&g.smax[b], __ATOMIC_RELAXED)) atomicMax(&g.smax[b], o);
      }
    }
  } else {
    // one pair of atomics per workgroup, and only when it can raise a maximum
    // (tens of thousands of same-address atomics serialise in the L2)
    __shared__ float red[2][kWaves];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      mden = fmaxf(mden, __shfl_xor(mden, d, 64));
      mov = fmaxf(mov, __shfl_xor(mov, d, 64));
    }
    if (lane == 0) {
      red[0][wave] = mden;
      red[1][wave] = mov;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      float m = red[threadIdx.x][0];
      for (int w = 1; w < kWaves; ++w) m = fmaxf(m, red[threadIdx.x][w]);
      const unsigned bits = __float_as_uint(m);
      unsigned int* mx = g.maxima + 2 * (b / g.group) + threadIdx.x;
      if (bits > __atomic_load_n(mx, __ATOMIC_RELAXED)) atomicMax(mx, bits);
    }
  }
}

template <bool FINAL>
__global__ void __launch_bounds__(kThreads) masked_phase_kernel(MaskedFastArgs g) {
  __shared__ int2 D[kWaves][2][kAsmMaxCols];
  // Workgroups are dealt to the 8 XCDs round robin; the row blocks of a patch
  // share its integral images, so they are mapped to ONE XCD (one L2): XCD x
  // takes the x-th eighth of the (patch, row block) list.  Grid = 8 * chunk.
  const int chunk = gridDim.x >> 3;
  const int item = g.xcd_map ? (blockIdx.x & 7) * chunk + (blockIdx.x >> 3) : blockIdx.x;
  const int b = item / g.row_blocks;
  if (b >= g.batch) return;
  const int row_block = item - b * g.row_blocks;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cls = g.cls[b];
  float tol = 0.f, px_thr = 0.f;
  if (FINAL) {
    const unsigned int* mx = g.maxima + 2 * (b / g.group);
    tol = 1e3f * 1.1920928955078125e-07f * __uint_as_float(mx[0]);
    px_thr = 0.3f * __uint_as_float(mx[1]);
  }
  PhaseOut po = {0.f, 0.f, -INFINITY};
  if (cls == 3) return;  // masked_phase3_kernel
  if (!FINAL && cls == 0 && g.axis_max && !g.sweep0[b]) return;  // masked_axis_max_kernel
  switch (cls) {
    case 0: masked_phase_rows<0, FINAL>(g, b, row_block, D[wave][0], D[wave][1], tol, px_thr, &po); break;
    case 1: masked_phase_rows<1, FINAL>(g, b, row_block, D[wave][0], D[wave][1], tol, px_thr, &po); break;
    default: masked_phase_rows<2, FINAL>(g, b, row_block, D[wave][0], D[wave][1], tol, px_thr, &po); break;
  }
  phase_finish<FINAL>(g, b, row_block, po);
}

// Class 3 (both sides masked): all eight products come from memory and no
// row structure is needed, so the surface is walked flat, four elements per
// thread with 16-byte loads, the next four in flight while these are assembled.
template <bool FINAL>
__global__ void __launch_bounds__(kThreads) masked_phase3_kernel(MaskedFastArgs g) {
  const int chunk = gridDim.x >> 3;
  const int item = g.xcd_map ? (blockIdx.x & 7) * chunk + (blockIdx.x >> 3) : blockIdx.x;
  const int b = item / g.row_blocks;
  if (b >= g.batch || g.cls[b] != 3) return;
  const int row_block = item - b * g.row_blocks;
  const int Sy = g.S[0], Sx = g.S[1];
  float tol = 0.f, px_thr = 0.f;
  if (FINAL) {
    const unsigned int* mx = g.maxima + 2 * (b / g.group);
    tol = 1e3f * 1.1920928955078125e-07f * __uint_as_float(mx[0]);
    px_thr = 0.3f * __uint_as_float(mx[1]);
  }
  const long long e0 = (long long)row_block * kWaves * kAsmRowsPerWave * g.pitch;
  const int n4 = static_cast<int>(
      min((long long)kWaves * kAsmRowsPerWave * g.pitch, g.elems - e0) >> 2);
  const v4i* src[8];
  src[0] = reinterpret_cast<const v4i*>(g.raw0 + (long long)b * g.raw_stride + e0);
#pragma unroll
  for (int q = 1; q < 8; ++q)
    src[q] = reinterpret_cast<const v4i*>(g.rawd + (long long)(g.first[b] + q - 1) * g.raw_stride + e0);
  float* out = g.out + (long long)b * g.elems + e0;
  PhaseOut po = {0.f, 0.f, -INFINITY};
  v4i nxt[8];
  // FINAL: rows whose largest possible overlap is below the overlap threshold are
  // zero (see masked_phase_rows): their eight product rows are not read
  auto dead_row = [&](int ky) {
    if (!FINAL || !g.dead_rows) return false;
    const int dy = ky - (g.Q[0] - 1);
    const int ny = min(g.P[0], g.Q[0] + dy) - max(0, dy);
    return static_cast<float>(ny * g.Q[1]) < px_thr;
  };
  auto fetch = [&](int f) {
    const int fc = min(f, n4 - 1);
    if (dead_row(static_cast<int>((e0 + 4LL * fc) / g.pitch))) return;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (!FINAL && q == 0) continue;  // the maxima do not involve a' * b'
      nxt[q] = src[q][fc];
    }
  };
  fetch(threadIdx.x);
  for (int f = threadIdx.x; f < n4; f += kThreads) {
    v4i cur[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) cur[q] = (!FINAL && q == 0) ? v4i{0, 0, 0, 0} : nxt[q];
    fetch(f + kThreads);
    const long long e = e0 + 4LL * f;
    const int ky = static_cast<int>(e / g.pitch);
    const int kx0 = static_cast<int>(e - (long long)ky * g.pitch);
    if (dead_row(ky)) {  // (rows past Sy: ny <= 0, dead as well; padding, never read)
      *reinterpret_cast<float4*>(out + 4 * f) = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ky < Sy && kx0 < Sx) po.rmax = fmaxf(po.rmax, 0.f);
      continue;
    }
    float v4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = cur[3][j];
      const PadfieldTerms t =
          padfield_terms(cur[0][j], cur[1][j], cur[2][j], n, square_sum(cur[4][j], cur[5][j], n),
                         square_sum(cur[6][j], cur[7][j], n));
      const bool ok = ky < Sy && kx0 + j < Sx;
      if (FINAL) {
        float v = t.den > tol ? static_cast<float>(t.num_n) / t.den_n : 0.f;
        v = fminf(fmaxf(v, -1.f), 1.f);
        if (t.ov < px_thr) v = 0.f;
        v4[j] = v;
        if (ok) po.rmax = fmaxf(po.rmax, v);
      } else if (ok) {
        po.mden = fmaxf(po.mden, t.den);
        po.mov = fmaxf(po.mov, t.ov);
      }
    }
    if (FINAL) *reinterpret_cast<float4*>(out + 4 * f) = make_float4(v4[0], v4[1], v4[2], v4[3]);
  }
  phase_finish<FINAL>(g, b, row_block, po);
}

// First-peak search of one finished surface from what the correlation kernel
// left behind: the surface maximum and the hot list (every element that
// exceeded threshold_rel * running maximum when its tile was produced).
// Same result as peaks_first_kernel in sfm_xcorr.hip: peak = element that
// equals its (2 m + 1)^2 zero-padded window maximum and exceeds
// threshold_rel * max(surface) (flow_field.py:238-262).
__device__ __forceinline__ bool peak_better(float v, int i, float bv, int bi) {
  return v > bv || (v == bv && i < bi);
}

// First peak of one surface by ONE WAVE (the kernel below runs four surfaces per
// workgroup, a wave each: 40 401 workgroups of a few hundred hot elements were
// priced by their dispatch and by a chain of dependent round trips per
// workgroup).  The first hot-list entry of every lane is requested together with
// the surface's maximum and fill count, the candidate slots are counted in LDS
// (a returning global atomic per candidate was a round trip of its own), and the
// arg-max runs on the shuffle network: no barrier anywhere.
__device__ void wave_first_peak(const MfmaArgs& a, int b, const float* surf,
                                int Sy, int Sx, int* cand_lds) {
  const int lane = threadIdx.x & 63;
  // (unconditional: entries beyond the fill count are stale and ignored)
  const float hv0 = a.hot_val[(long long)b * a.hot_cap + min(lane, a.hot_cap - 1)];
  const int hi0 = a.hot_idx[(long long)b * a.hot_cap + min(lane, a.hot_cap - 1)];
  const float mx = a.v1[b];          // the surface maximum on entry
  const int n_hot = a.hot_count[b];
  if (lane == 0) *cand_lds = 0;
  // (the reset, the other lanes' atomics and the read-back below are LDS operations of ONE
  // wave, which the hardware runs in program order; the fences keep the compiler from
  // reordering them around the divergent loops in between)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int pitch = a.sx_pitch;
  const int m = a.min_distance;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  // Tests one element that exceeds the threshold and records it if it is a
  // window maximum.
  auto consider = [&](int y, int x, float v) {
    // window maximum from clamped addresses: unconditional loads (all in flight
    // together); a clamped position repeats an element of the window, which
    // cannot change the maximum
    float wm = -INFINITY;
    const bool outside = y - m < 0 || y + m >= Sy || x - m < 0 || x + m >= Sx;
    if (m == 2) {  // the default min_distance: 25 loads in flight instead of a loop of waits
      float w[25];
#pragma unroll
      for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx)
          w[(dy + 2) * 5 + dx + 2] = surf[(long long)min(max(y + dy, 0), Sy - 1) * pitch +
                                          min(max(x + dx, 0), Sx - 1)];
#pragma unroll
      for (int k = 0; k < 25; ++k) wm = fmaxf(wm, w[k]);
    } else {
      for (int dy = -m; dy <= m; ++dy) {
        const float* wrow = surf + (long long)min(max(y + dy, 0), Sy - 1) * pitch;
        for (int dx = -m; dx <= m; ++dx) wm = fmaxf(wm, wrow[min(max(x + dx, 0), Sx - 1)]);
      }
    }
    if (outside) wm = fmaxf(wm, 0.f);
    if (v != wm) return;
    const int i = y * Sx + x;
    if (peak_better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
    const int slot = atomicAdd(cand_lds, 1);
    if (slot < a.cand_cap) {
      a.cand_val[(long long)b * a.cand_cap + slot] = v;
      a.cand_idx[(long long)b * a.cand_cap + slot] = i;
    }
    if (i == 0) a.zero_is_peak[b] = 1;
  };
  if (mx > 0.f) {
    const float thr = a.threshold_rel * mx;
    if (n_hot <= a.hot_cap) {
      const float* hv = a.hot_val + (long long)b * a.hot_cap;
      const int* hi = a.hot_idx + (long long)b * a.hot_cap;
      for (int e = lane; e < n_hot; e += 64) {
        const float v = e == lane ? hv0 : hv[e];
        if (!(v > thr)) continue;
        const int i = e == lane ? hi0 : hi[e];
        const int y = i / Sx;
        consider(y, i - y * Sx, v);
      }
    } else {
      // Hot list overflowed (flat surfaces): sweep the stored surface.
      const int n4 = (Sx + 3) >> 2;
      const int skipped = a.skipmask ? a.skipmask[b] : 0;  // pruned row tiles: not stored
      for (int y = 0; y < Sy; ++y) {
        if ((skipped >> (y >> 4)) & 1) continue;
        const float* row = surf + (long long)y * pitch;
        for (int c4 = lane; c4 < n4; c4 += 64) {
          const float4 q4 = *reinterpret_cast<const float4*>(row + 4 * c4);
          const float vals[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (vals[t] > thr && 4 * c4 + t < Sx) consider(y, 4 * c4 + t, vals[t]);
        }
      }
    }
  }
  // (value, index) arg-max across the wave, first index wins ties (a total
  // order: any reduction tree finds the same winner).
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const float ov = __shfl_xor(bv, d, 64);
    const int oi = __shfl_xor(bi, d, 64);
    if (peak_better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) {
    a.cand_count[b] = *cand_lds;   // (behind every lane's atomics in this wave's LDS queue)
    const float v1 = bv;
    const int i1 = v1 == -INFINITY ? 0 : bi;  // argmax of an all -inf row is 0
    a.idx1[b] = i1;
    a.v1[b] = v1;
    sfm::set_bit_once(&a.bitmap[(long long)(b / a.group) * a.bitmap_words + (i1 >> 5)],
                       1u << (i1 & 31));
  }
}

// One WAVE per surface, four surfaces per workgroup; v1[b] holds the surface
// maximum on entry.
__global__ void __launch_bounds__(kThreads) mfma_first_peak_kernel(MfmaArgs a) {
  __shared__ int s_cand[kWaves];
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x * kWaves + wave;
  if (b >= a.batch) return;
  wave_first_peak(a, b, a.surface + b * a.s_stride, a.S[0], a.S[1], &s_cand[wave]);
}

}  // namespace

// Patch statistics, centres and correction tables of the mode.
int launch_prep(const MfmaArgs& a, int mode, const Variant& v, hipStream_t st) {
  const size_t pixels = (size_t)a.P[0] * a.P[1];
  if (mode == kModeSameExactLazyG) {   // no pixels in LDS: the packed row / half-band column words
    const size_t lazy_lds =
        sizeof(unsigned) * (2 * (size_t)a.P[0] * (a.P[1] / 16) + 2 * 2 * (size_t)(a.P[0] / 16) * a.P[1]);
    if (int rc = sfm::set_lds(&mfma_prep_same_kernel<true>, lazy_lds)) return rc;
    hipLaunchKernelGGL(mfma_prep_same_kernel<true>, dim3(a.batch),
                       dim3(64 * kPrepWavesAlone), lazy_lds, st, a);
  } else if (mode != kModeGeneral) {
    const size_t prep_lds = 2 * ((pixels + 15) & ~(size_t)15);
    if (int rc = sfm::set_lds(&mfma_prep_same_kernel<false>, prep_lds)) return rc;
    hipLaunchKernelGGL(mfma_prep_same_kernel<false>, dim3(a.batch),
                       dim3(64 * kPrepWavesAlone), prep_lds, st, a);
  } else {
    // search-window variants: the wide prep pass (see mfma_prep_wide_kernel) where its
    // padded LDS copy of a patch fits next to its static arrays; mfma_prep_kernel
    // (pixels + its reduction words: within the eligibility bound) writes the same tables
    const size_t wide_lds = (size_t)a.P[0] * (16 * ((a.P[1] + 15) / 16) + 16);
    if (v.nca > 10 && a.P[1] <= kWidePrepMaxCols &&
        wide_lds + kWidePrepStaticLds <= kLdsPerCu) {
      if (int rc = sfm::set_lds(&mfma_prep_wide_kernel, wide_lds)) return rc;
      hipLaunchKernelGGL(mfma_prep_wide_kernel, dim3(a.batch, 2), dim3(64 * kWidePrepWaves),
                         wide_lds, st, a);
    } else {
      if (int rc = sfm::set_lds(&mfma_prep_kernel, pixels)) return rc;
      hipLaunchKernelGGL(mfma_prep_kernel, dim3(a.batch, 2), dim3(kThreads), pixels, st, a);
    }
  }
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int launch_prep_masked(const MfmaArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(mfma_prep_masked_kernel, dim3(a.batch, 2), dim3(kThreads), 0,
                     st, a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int launch_first_peak(const MfmaArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(mfma_first_peak_kernel, dim3((a.batch + kWaves - 1) / kWaves), dim3(kThreads), 0, st, a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int launch_masked_tables(const MaskedFastArgs& g, hipStream_t st) {
  hipLaunchKernelGGL(masked_classify_kernel, dim3(1), dim3(1024), 0, st, g);
  hipLaunchKernelGGL(masked_tables_kernel, dim3(g.batch), dim3(kThreads), 0, st, g);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int launch_masked_assembly(const MaskedFastArgs& g, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(((long long)g.row_blocks * g.batch + 7) / 8 * 8));
  if (g.axis_max)
    hipLaunchKernelGGL(masked_axis_max_kernel, dim3(g.batch), dim3(64), 0, st, g);
  hipLaunchKernelGGL(masked_phase_kernel<false>, grid, dim3(kThreads), 0, st, g);
  hipLaunchKernelGGL(masked_phase3_kernel<false>, grid, dim3(kThreads), 0, st, g);
  hipLaunchKernelGGL(masked_phase_kernel<true>, grid, dim3(kThreads), 0, st, g);
  hipLaunchKernelGGL(masked_phase3_kernel<true>, grid, dim3(kThreads), 0, st, g);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace mfma
}  // namespace sfm
