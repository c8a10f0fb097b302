// Patch cross-correlation on the int8 matrix cores of gfx950 (CDNA4).
//
// Device replacement for masked_xcorr(use_jax=True) of the reference
// (flow_field.py:36-89, unmasked branch) + the mean subtraction of
// _batched_xcorr (flow_field.py:340-353) for uint8 2-D patches: the reference
// evaluates  out[dy, dx] = sum_{y,x} (A[y+dy, x+dx] - mA) (B[y, x] - mB)
// with zero-padded FFTs; here the sum is evaluated exactly.
//
// 1. Integer core.  With per-patch integer centres cA, cB (chosen so that
//    a' = a - cA and b' = b - cB fit int8) the product sum S = sum a' b' is an
//    exact int32 and
//        out = S - mA' SB - mB' SA + mA' mB' N
//    where mA' = mA - cA (|mA'| <= 0.5 unless clamped), SA / SB are the sums
//    of a' / b' over the overlap rectangle of the shift (box sums from a
//    per-patch integral image) and N the overlap area.
//
// 2. The product sum as a GEMM on v_mfma_i32_16x16x64_i8.  For an output tile
//    of 16 dy values (M) x 16 dx values (N) the contraction index is
//    k = (yb, xa): A-operand[dy, k] = a'[yb + dy, xa] and
//    B-operand[k, dx] = b'[yb, xa - dx].  One MFMA consumes four k-slots
//    (lane group g = lane >> 4 <-> patch row yb0 + g) of 16 consecutive xa
//    each (one "chunk" ca):
//      - the A fragment of lane (m, g) is an aligned 16-byte row segment
//        a'[yb0 + g + dy0 + m, 16 ca ..] read with ds_read_b128 from an LDS
//        copy of the pre patch that is zero padded above and below, so
//        shifts that run off the patch contribute zeros;
//      - the B fragment of lane (n, g) is b'[yb0 + g, 16 (ca - q) + t - n + ..]:
//        a byte-shifted window of row yb0 + g that depends on ca and the
//        output tile q only through c = ca - q.  Each lane reads the 4 NCE + 1
//        aligned dwords covering its windows once per row group and funnel
//        shifts them (v_alignbyte_b32) into NCE fragments, which are then
//        used against every A chunk: NCA x NCE MFMAs per row group into
//        NCA + NCE - 1 accumulator tiles, all from 14 LDS loads + NCE*4 VALU ops.
//    A wave owns one 16-row dy tile at a time and all dx tiles of it; tiles
//    only visit the patch rows that overlap (zero skipping), so the MFMA work
//    is ~1.24x the algorithmic 2 P^4 flop for P = Q = 160.
//
// 3. Epilogue.  For P == Q (the production case) every overlap rectangle is
//    anchored at a patch corner, and with yv = dy mod Py, xv = dx mod Px,
//    ey = -sign(dy), ex = -sign(dx) the whole correction collapses to
//        ey ex G[yv][xv] + ey Rrow[dx>=0][yv] + ex Rcol[dy>=0][xv] + const
//                        + mA' mB' ny nx
//    with ONE combined float table per patch,
//        G[yv][xv] = -mB' IA[yv][xv] - mA' IB[Py - yv][Px - xv]
//    (IA / IB = integral images of a' / b'), and four 1-D arrays, all written
//    by the prep kernel: one coalesced gather per output instead of eight.
//    For P != Q (post_patch_size) the general 8-lookup box-sum form is used.
//
// 4. Schedule.  Workgroups are persistent (two per CU) and take patches from
//    a dynamic queue (the issue arbiter favours the older workgroup of a CU);
//    staging is one global round trip (unaligned 16-byte loads of both
//    patches), the table G is pulled into L2 by LDS-direct loads nothing waits
//    for; the first-peak search runs on what the kernel leaves behind (surface
//    maximum + hot list) in mfma_first_peak_kernel.  One launch carries several
//    reference batches (SfmXcorrDesc.group keeps their coupling apart).
//
// 5. Masked images (MODE raw): the same kernel forms exact integer products of
//    operand planes (value, validity, split square); eight passes + an f64
//    assembly kernel give Padfield's normalised correlation.
//
// 6. Search-window geometry (pre patch 161 .. 320 wide against a post patch of up to
//    160): one workgroup of eight waves per CU, a tile job is one column half of a
//    row tile (see the kernel).
//
// LDS per workgroup (P = Q = 160): pre patch (Py + 34) x 176 B + post patch
// (Qy + 3) x 208 B = 68 KB -> two workgroups (8 waves) per CU.  Row pitches
// 176 / 208 keep the b128 / b32 fragment reads bank-conflict free.
//
// The row loop exists in three forms: A chunk outermost with in-place prefetch
// (every mode but the general one), the column-half loop of the search-window
// variants, and the plain B-outer loop of the general mode with up to ten chunks.
// The waves of a workgroup draw dy tiles from a shared longest-first list through
// an LDS counter: the four SIMDs do not run at the same speed (each shares its
// matrix pipe with a wave of the other workgroup of the CU), and a static deal
// spent ~17 % of a workgroup's time waiting for its slowest wave.
//
// Build switches (measurement builds): SFM_MFMA_TIMING
// (in-kernel phase ticks), SFM_ABLATE_EPILOGUE, SFM_DEV_ONLY_WIDE.
//
// The translation units of the path and what they share:
//   sfm_mfma_kernel.h   the correlation kernel and its launch templates;
//                       sfm_mfma_g<NCA>x<NCE>.hip instantiates one chunk geometry each
//   sfm_xcorr_mfma.hip  the kernels around it (prep, masked assembly, first peak) and
//                       their launches
//   sfm_mfma_host.hip   the host driver: layout, workspace, mode choice, sfm::mfma_i8_*
// Here: the constants, PatchParams, LdsTail, MfmaArgs, MaskedFastArgs, the modes, the
// list of chunk geometries, the device helpers more than one unit uses and the launch
// functions the driver calls.
#ifndef SFM_MFMA_H_
#define SFM_MFMA_H_

#include "sfm_xcorr_units.h"

#include <cstddef>

namespace sfm {
namespace mfma {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr size_t kLdsPerCu = 160 * 1024;
// search-window variants: one workgroup per CU, two waves per SIMD (twelve spill and lose)
constexpr int kWideWaves = 8;
constexpr int kWideThreads = 64 * kWideWaves;
constexpr int kPadTop = 16;     // zero rows above the pre patch in LDS
constexpr int kPadBottom = 18;  // zero rows below
constexpr int kMaxTileJobs = 96;   // capacity of MfmaArgs::order (dy tiles, or their column halves)
// Row-loop variants of the correlation kernel: outer column tiles (each side)
// left out when their bound allows it.  With 20 column tiles (P = 160) and an
// NCC peak of 0.9+ the outer 4 qualify for most patches, the outer 3 for all.
__host__ __device__ constexpr int col_skip_hi(int nq) { return nq / 5; }
__host__ __device__ constexpr int col_skip_lo(int nq) { return 3 * nq / 20; }
__host__ __device__ constexpr int col_skip_2(int nq) { return nq / 4; }       // per-row-tile
__host__ __device__ constexpr int col_skip_3(int nq) { return 3 * nq / 10; }  // variants
// the narrowest row loop: the four central column tiles (entered only in flight, see
// narrow_after in the kernel)
__host__ __device__ constexpr int col_skip_c(int nq) { return (nq - 4) / 2; }
// tbound layout per patch: [0, 30) row tiles; [30], [31] outer col_skip_lo / _hi column
// tiles (any dy); [32 + 3 p + j] row tile p with the outer col_skip_hi / _2 / _3 column
// tiles (2-D bound from 16 x 16 block energies)
constexpr int kBoundStride = 256;   // floats per patch: bounds, then the row-energy prefixes
constexpr int kBoundTiles = 30;    // dy tiles per patch with a pruning bound
constexpr int kBoundCorr = 122;    // tbound slot: bound of the mean-correction terms
constexpr int kBlkRows = 16, kBlkCols = 12;  // 16 x 16 pixel blocks of a patch (<= 256 x 192)
constexpr int kBoundRows = 256;    // patch rows the prep kernel keeps energies for
// tbound[kRowPre + 64 s + k] (uint bits): sum over rows < min(4 k, rows) of side s of
// sum_x (pixel - centre)^2 -- the energies of the int8 operands, exact integers
// (< 2^31 for every patch the matrix path takes); k <= 63, i.e. rows <= kEarlyRows
constexpr int kRowPre = 128;
constexpr int kEarlyRows = 252;
// Measurement build: run statistics of a launch in the free words behind the queue head --
// [1] waves finished; then (first patch of a run, inside a run) pairs: [2], [3] patches,
// [4], [5] redone tiles, [6], [7] patches whose seed block was the block of their maximum.
constexpr int kRunStatWords = 7;

struct PatchParams {  // written by the prep kernel, one per patch
  int y0[2], x0[2];   // clamped patch origin in the image (pre, post)
  int c[2];           // integer centres
  float mu[2];        // mean - centre
  int my0[2], mx0[2]; // masked path: clamped patch origin in the mask arrays
};

// Operand planes of the masked (Padfield) path, all int8:
//   VAL    (pixel - centre) on valid pixels, 0 on masked ones
//   VALID  1 on valid pixels
//   SQHI / SQLO  with s = VAL^2:  s = 128 (SQHI + 64) + SQLO on valid pixels
enum Plane { kPlaneVal = 0, kPlaneValid = 1, kPlaneSqHi = 2, kPlaneSqLo = 3 };

// The correlation kernel's state words in dynamic LDS, behind the two patches and the
// aux arrays (MfmaArgs::r_bytes).  The kernel takes its pointers from this struct and
// the host the launch size: the size decides the workgroups per CU.
struct LdsTail {
  // [0] float bits of the running maximum of the current surface, [1] hot-list fill
  // count of the current patch, [2] next patch of the workgroup (queue), [3] tile
  // counter of the current patch
  int head[4];
  float tb[kBoundStride];   // pruning bounds of the current patch (a.prune)
  // Pruning state of the workgroup:
  //   [0] (row tile << 8 | column tile) that held the maximum of the previous patch:
  //       where the next patch is probed first
  //   [1] bit mask of the row tiles pruned in the current patch
  //   [2] anything pruned in the current patch?  [3] patches done  [4] probe this patch?
  int best[8];
  // Lazy stores, per patch: [0] row tiles that should be stored (requests of
  // tiles that may be hot), [1] tiles finished, [2] tiles stored, [3] tiles
  // claimed for recomputation
  int lz[4];
  float lz_tmax[31];        // maximum of finished tile p (tiles 0 .. 30)
  int lz_prev;              // tile mask of what the previous patch needed
  // Column side of the lazy stores: [0], [1] lowest / highest column tile that
  // held a possibly hot element in this patch, [2], [3] the same of the previous
  // patch of the workgroup
  int lz_cq[4];
  // outer column tiles row tile p dropped inside its row loop (0: none beyond the
  // a-priori ones)
  int lz_ks[32];
  int lz_rows[31];          // first | last << 8 row (0 .. 15) of tile p with a possibly hot element
  int pad[5];               // unused; keeps the launch size where it has always been
};
constexpr size_t kLdsTailHead = offsetof(LdsTail, tb);   // what the raw (masked) launch has
static_assert(kLdsTailHead == 16 && offsetof(LdsTail, best) == 16 + 1024 &&
                  offsetof(LdsTail, lz) == 1072 && offsetof(LdsTail, lz_tmax) == 1088 &&
                  offsetof(LdsTail, lz_prev) == 1212 && offsetof(LdsTail, lz_cq) == 1216 &&
                  offsetof(LdsTail, lz_ks) == 1232 && offsetof(LdsTail, lz_rows) == 1360 &&
                  offsetof(LdsTail, pad) == 1484 && sizeof(LdsTail) == 16 + 1024 + 464,
              "the LDS size of a launch decides the workgroups per CU");

struct MfmaArgs {
  const unsigned char* img[2];
  int ishape[2][2];   // [side][y, x]
  const int* starts[2];
  int P[2], Q[2];     // pre / post patch [y, x]
  int S[2];           // surface [y, x]
  int batch;
  int use_mean;
  float mean;
  PatchParams* pp;
  int* integ[2];      // general path: [B, (py+1) * (px+1)] per side
  long long integ_stride[2];
  float* gtab;        // same-size path: [B, Py * Px] combined table G
  float* aux;         // same-size path: [B, 4 * aux_n + 4] 1-D arrays + consts
  int aux_n;          // max(Py, Px) + 1
  float* surface;     // [B, 16 NP, 16 NQ] (padded to whole tiles)
  // LDS geometry
  int pa, pb;         // row pitches (bytes)
  int ml;             // left margin of the post patch rows (bytes)
  int a_bytes, b_bytes;
  int r_bytes;        // aux arrays / reduction scratch behind the patches
  // tile schedule: all dy tiles, longest first; the waves of a workgroup draw
  // from it through an LDS counter (ints: scalar loads from the kernarg segment)
  int order[kMaxTileJobs];
  int n_order;
  // fused first-peak search (flow_field.py:238-262); see FusedPeaks
  int do_peaks;
  float threshold_rel;
  int min_distance;
  int cand_cap;
  int* idx1;
  float* v1;
  int* zero_is_peak;
  int* cand_count;
  float* cand_val;
  int* cand_idx;
  unsigned* bitmap;
  int group, bitmap_words;
  int hot_cap;        // per-surface capacity of the hot list
  int* hot_count;     // [B]
  float* hot_val;     // [B, hot_cap]
  int* hot_idx;       // [B, hot_cap] flat index ky * Sx + kx
  int* skipmask;      // [B] bit p: row tile p was pruned, its surface rows are not stored
  int sx_pitch;       // padded surface: row pitch (floats) = 16 * NQ
  // raw-product mode (masked path)
  const unsigned char* mask[2];
  int mshape[2][2];
  int plane[2];       // Plane of the pre / post operand
  int* raw_out;       // [batch, raw_stride] int32 products (rows x sx_pitch used)
  long long raw_stride;
  int* nvalid;        // [batch, 2] un-masked pixels per patch side (prep output)
  // extra masked passes: item i = (patch list[i] >> 3, kMaskedPasses[list[i] & 7]),
  // i < *n_list; its products go to raw_out[i]
  const int* list;
  const int* n_list;
  // a' * b' pass of the masked path: lower bound of the batch maximum of the overlap
  // (masked_classify_kernel); row tiles below 0.3 x it are zeroed by the overlap rule
  const int* ov_lb;   // [groups]
  int ov_group;       // patches per reference batch (maxima are per batch)
  long long s_stride; // padded surface: floats per patch = 16 * NP * sx_pitch
  // dynamic patch queue (NULL: static striding over the workgroups)
  int* work_counter;
  // Queue ticket t -> patches (launch_one): tickets below n_runs are the run of `run`
  // consecutive patches from t * run, later ones the single patch run_end + (t - n_runs);
  // run_end = n_runs * run.  (run = 1, n_runs = run_end = 0: ticket t is patch t.)
  int run, n_runs, run_end;
  // shader-clock probe: workgroup 0 leaves (core cycles, 10 ns wall ticks) of its
  // residency here (bench.py reports the sustained clock under this kernel);
  // clk[2]: dy tiles skipped by the pruning (low word) / drawn (high word), whole
  // launch; clk[3]: column tiles left out of the computed dy tiles (low word) / dy tiles
  // abandoned inside their row loop (high word); clk[4]: matrix
  // instructions issued by the row loops (count_tiles)
  long long* clk;
  int prio_mode;      // experiment knob: 0 natural, 1 alternate per tile, 2 static
  // exact pruning of dy tiles (fused-peaks mode): tbound[b][p] bounds |surface|
  // over tile p widened by tile_guard(p) rows (prep output; see the tile loop)
  float* tbound;      // [batch, kBoundStride]; the last two entries: outer column tiles
  int prune;
  int touch_all;      // lazy modes: pull the whole correction table into L2, not only the requested tiles' rows (SFM_MFMA_TOUCH_ALL=1)
  int narrow;         // lazy modes: row loops drop provably cold outer column tiles in flight (SFM_MFMA_NARROW=0: off)
  int early;          // lazy modes: abandon provably cold tiles inside the row loop (least distance of two tests, row groups; 0 = off)
  int count_tiles;    // report the pruning counts through clk (timing hooks on)
  int probe;          // seed the running maximum from a probe block (see the kernel)
  int guard, guard_x;
  // The row band in exact terms (need_tiles / tile_guard below): the first peak's
  // sharpness window is win = min(2 peak_radius + 1, Sy) rows tall and starts at
  // clamp(row - win / 2, 0, win_top), win_top = Sy - win; the max filter reads
  // guard_md = min_distance rows either side of a hot element.  `guard` (twice the
  // radius) is what a window pushed back inside the surface can reach: it stays
  // the band of the tiles under such a window, and all there is along x.
  int win, win_top, guard_md;
  // Correction table built where it is read (kModeSameExactLazyG): the prep kernel
  // leaves, instead of G, the centred column sums above every 16th patch row --
  // c16[side][I][x] = sum_{y < 16 I} (pixel[y][x] - centre), I <= Py / 16, ints (and
  // the prefixes T of the post patch's centred row sums) -- and a tile that is about
  // to run its epilogue first forms its 16 table rows from them and the int8 patches
  // in LDS, writes them into G (now a per-patch scratch in L2: ten kilobytes that the
  // same lanes read back at once) and runs the ordinary epilogue.
  int* c16;           // [B, c16_stride]: [2][Py / 16 + 1][Px] column sums, then T[Py + 1]
  long long c16_stride;
  int nq;             // column tiles of the kernel variant
  int prune_k[4];     // outer column tiles (each side) of the row-loop variants (ascending)
};

// Row tiles [*lo_t, *hi_t] that must be in memory when the rows [r_lo, r_hi] of the
// surface may hold hot elements: what the peak kernels can read on their account
// is the sharpness window of a first peak in one of these rows (its start is
// monotone in the row, so the two ends cover the rows between) and the max-filter
// rows of every hot element.  Scalar when its arguments are.
__device__ __forceinline__ void need_tiles(const MfmaArgs& a, int r_lo, int r_hi, int* lo_t,
                                           int* hi_t) {
  const int w_lo = min(max(r_lo - (a.win >> 1), 0), a.win_top);
  const int w_hi = min(max(r_hi - (a.win >> 1), 0), a.win_top) + a.win - 1;
  const int lo = max(min(w_lo, r_lo - a.guard_md), 0);
  const int hi = min(max(w_hi, r_hi + a.guard_md), a.win_top + a.win - 1);
  *lo_t = lo >> 4;
  *hi_t = min(hi >> 4, a.n_order - 1);
}

// A-priori pruning: the rows around row tile p whose elements must all be cold
// before the tile may be left out.  A tile that a window pushed back inside the
// surface can cover (it touches the first or the last `win` rows) is read from up
// to `guard` rows away; any other tile from a hot element within guard_md rows or
// a first peak within win / 2.
__device__ __forceinline__ int tile_guard(const MfmaArgs& a, int p) {
  const int t0 = 16 * p, t1 = min(16 * p + 15, a.S[0] - 1);
  return (t0 <= a.win - 1 || t1 >= a.win_top) ? a.guard : max(a.guard_md, a.win >> 1);
}

// 16 image bytes at an arbitrary byte offset (global memory takes unaligned
// dwordx4 loads); only the last bytes of the image need the guarded path.
__device__ __forceinline__ v4i load_16_bytes(const unsigned char* img, long long off,
                                             long long img_bytes) {
  // ONE unconditional load from an address clamped into the image (a load
  // under a per-lane condition gets its own basic block, and the loads of a
  // staging round would be waited for one by one); at the very end of the image
  // the bytes are shifted into place afterwards and the rest is zero.
  // img_bytes >= 16 (mfma_i8_eligible).
  const long long last = img_bytes - 16;
  const long long o = off > last ? last : off;
  v4i v;
  __builtin_memcpy(&v, img + o, 16);
  const long long sh = off - o;
  if (sh != 0) {
    unsigned __int128 x;
    __builtin_memcpy(&x, &v, 16);
    x = sh >= 16 ? 0 : x >> (8 * static_cast<int>(sh));
    __builtin_memcpy(&v, &x, 16);
  }
  return v;
}

constexpr int kPrepCols = 3;  // columns per lane: Px <= 192

// One entry of the correction table, G = -mB' IA'[yv][xv] - mA' IB'[Py - yv][Px - xv],
// from the two (exact, integer-valued) integral-image entries: ONE expression for
// the prep kernel's table and for the table rows built in the correlation kernel's
// epilogue (a product, then a fused multiply-add -- pinned, so that the compiler
// cannot contract the two sites differently: the surfaces must agree bit for bit).
__device__ __forceinline__ float g_entry(float mua, float mub, float ia, float ib) {
  return __fmaf_rn(-mua, ib, __fmul_rn(-mub, ia));
}

// Wave-wide inclusive add scan on the DPP network (row shifts inside each
// 16-lane row, then row broadcasts), ~12 VALU ops instead of 6 LDS permutes.
__device__ __forceinline__ int wave_scan_incl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return v;
}

// ---------------------------------------------------------------------------
// Masked path, fast form.  Of the eight Padfield products only a' * b' always
// needs the matrix cores: a product with the VALID plane of a side WITHOUT
// masked pixels is a box sum of the other operand over the overlap rectangle,
// read from per-patch integral images.  Per patch:
//   class 0  no masked pixel on either side   1 matrix pass, 4 tables
//   class 1  pre side masked, post side clean 4 passes, 3 tables (pre planes)
//   class 2  pre side clean, post side masked 4 passes, 3 tables (post planes)
//   class 3  both sides masked                8 passes
// The assembly runs twice over the integer data (batch maxima first, then the
// normalised surface) instead of spilling numerator, denominator and overlap
// surfaces in between.
// ---------------------------------------------------------------------------
struct MaskedFastArgs {
  const PatchParams* pp;
  const int* nvalid;    // [batch, 2]
  int* cls;             // [batch] class
  int* first;           // [batch] index of the patch's first extra product surface
  int* items;           // extra passes: patch * 8 + index into kMaskedPasses
  int* n_items;
  int* tab;             // [batch, 4, tab_elems] inclusive integral images
  long long tab_elems;  // Py * Px
  const int* raw0;      // [batch, elems]   a' * b'
  const int* rawd;      // [n_items, elems] extra products
  long long elems;      // padded surface elements per patch
  long long raw_stride; // ints between consecutive product surfaces
  int pitch;
  const unsigned char* img[2];
  const unsigned char* mask[2];
  int ishape[2][2], mshape[2][2];
  int P[2], Q[2], S[2];
  int batch;
  int xcd_map;
  int all_passes;       // test switch: every patch takes the eight passes (class 3)
  int dead_rows;        // final phase: skip rows below the overlap threshold (SFM_MASKED_DEADROWS=0: off)
  int row_blocks;       // workgroups per surface in the assembly kernels
  int axis_max;         // class 0 maxima come from masked_axis_max_kernel (P == Q)
  int* sweep0;          // [batch] 1: a class 0 patch whose maxima need the sweep after all
  int group;            // patches per reference batch: maxima / ov_lb are per batch
  int* ov_lb;           // [groups] lower bound of the batch maximum of the overlap
  unsigned int* maxima; // [groups, 2]
  float* out;           // [batch, elems] final normalised surface
  unsigned int* smax;   // [batch] or NULL: per-surface maximum (ordered bits)
  float* blkmax;        // [batch, row_blocks] or NULL: maximum of every block of 32 surface rows
};

constexpr int kAxisMaxLen = 192;   // patch side (matrix path: <= 160 wide, <= 192 tall)
// masked assembly kernels: surface rows per wave; a workgroup's rows are one block of the
// block maxima that the peak search reads
constexpr int kAsmRowsPerWave = 8;
static_assert(kWaves * kAsmRowsPerWave == kMaskedBlkRows, "blkmax blocks");

// kModeSameExact: P == Q and Px == 16 NCA (production 160, 128, 96, 64, 48): the
// per-column sign / index arithmetic of the epilogue becomes compile-time.
constexpr int kModeGeneral = 0, kModeSame = 1, kModeRaw = 2, kModeSameExact = 3;
// Lazy surface stores (r4), the flow path's form of kModeSame / kModeSameExact.
// The flow path never returns the surface, and the peak kernels read a few
// hundred of its 102 400 values: the 5 x 5 window of every hot element, the
// 11 x 11 sharpness window of the first peak, the hot elements themselves.  A
// row tile is therefore stored only if it may hold a hot element (its maximum
// exceeds threshold_rel x the running maximum, the test that also feeds the hot
// list) or holds a row that the peak kernels can read on account of a hot row of
// such a tile (need_tiles: the clamped sharpness window of a first peak there and
// min_distance rows either side; 5 rows for the defaults, up to 2 peak_radius only
// next to the surface border).  A tile learns that it is needed from a request
// mask in LDS if the hot neighbour finished first; if it had already finished
// without storing, it is recomputed at the end of the patch (redo mask; rare, because
// tiles are drawn innermost first and the peak sits there).  What is left
// un-stored has the property of a pruned tile -- no element of it is above
// threshold_rel x the final maximum, none is within min_distance rows of one that
// is, none lies in the first peak's window -- and goes into the same skip mask
// for the overflow sweeps of the peak kernels.  Values and decisions that reach
// the output are unchanged: bit-identical results.
constexpr int kModeSameLazy = 4, kModeSameExactLazy = 5;
// kModeSameExactLazy with the correction table built in the epilogue of the tiles
// that are stored (chosen by choose_mode; Py a multiple of 16): no table G in memory.
constexpr int kModeSameExactLazyG = 6;

// Instantiated chunk geometries (NCA, NCE), ascending: NCA >= ceil(Px / 16),
// NCE >= floor((Qx + 14) / 16) + 1.  (15, 11), (20, 11): search-window geometry, pre
// patches up to 240 / 320 wide.  kVariants and launch_mode (sfm_mfma_host.hip)
// are generated from this list; each geometry unit checks that it is on it.
#define SFM_MFMA_GEOMETRIES(X) \
  X(3, 4) X(4, 5) X(5, 6) X(6, 7) X(7, 8) X(8, 9) X(10, 11) X(15, 11) X(20, 11)

struct Variant {
  int nca, nce;
};
#define SFM_MFMA_VARIANT(nca, nce) {nca, nce},
constexpr Variant kVariants[] = {SFM_MFMA_GEOMETRIES(SFM_MFMA_VARIANT)};
#undef SFM_MFMA_VARIANT
constexpr bool listed_geometry(int nca, int nce) {
  for (const Variant& v : kVariants)
    if (v.nca == nca && v.nce == nce) return true;
  return false;
}

// --- sfm_xcorr_mfma.hip: the launches ----------------------------------------
// Patch statistics, centres and correction tables of the mode.
int launch_prep(const MfmaArgs& a, int mode, const Variant& v, hipStream_t st);
// Masked path prep (grid: batch x 2 sides).
int launch_prep_masked(const MfmaArgs& a, hipStream_t st);
// First peaks of the finished surfaces from the hot lists.
int launch_first_peak(const MfmaArgs& a, hipStream_t st);
// Masked path, before the raw products: classes, pass list, integral images.
int launch_masked_tables(const MaskedFastArgs& g, hipStream_t st);
// After them: the axis maxima (g.axis_max) and the two assembly phases, maxima first.
int launch_masked_assembly(const MaskedFastArgs& g, hipStream_t st);

// sfm_mfma_kernel.h: the correlation kernel, one explicit instantiation per geometry unit.
template <int NCA, int NCE>
int launch_variant(const MfmaArgs& a, int mode, int grid, size_t lds, hipStream_t st);

}  // namespace mfma
}  // namespace sfm

#endif  // SFM_MFMA_H_
