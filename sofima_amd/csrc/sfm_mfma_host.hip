// Host driver of the matrix-core correlation path: eligibility, LDS layout, workspace,
// argument blocks, mode choice and the sfm::mfma_i8_* entry points.  The kernels and
// their launches are in sfm_mfma_kernel.h (one unit per chunk geometry) and
// sfm_xcorr_mfma.hip; sfm_mfma.h has the overview and what the units share.
#include "sfm_mfma.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace sfm {
namespace mfma {
namespace {

bool exact_enabled() {
  return sfm::measure_option_on("SFM_MFMA_EXACT");
}

// SFM_MFMA_PRUNE=0: every dy tile is computed (tests, measurements).
bool prune_enabled() {
  return sfm::option_on("SFM_MFMA_PRUNE");
}

int pick_variant(int px, int qx) {
  const int nca = (px + 15) / 16, nce = (qx + 14) / 16 + 1;
  for (size_t i = 0; i < sizeof(kVariants) / sizeof(kVariants[0]); ++i)
    if (kVariants[i].nca >= nca && kVariants[i].nce >= nce) return static_cast<int>(i);
  return -1;
}

struct Layout {
  int nca, nce, pa, pb, ml, a_bytes, b_bytes;
};

Layout make_layout(const SfmXcorrDesc* d, const Variant& v) {
  Layout l;
  l.nca = v.nca;
  l.nce = v.nce;
  const int py = d->patch[1], qy = d->post_patch[1], qx = d->post_patch[2];
  // Pre patch rows: 16 * NCA data bytes, pitch = odd multiple of 16 bytes so
  // that 16 consecutive rows hit 16 different 16-byte LDS slots.
  int pa16 = v.nca;
  if ((pa16 & 1) == 0) pa16 += 1;
  l.pa = pa16 * 16;
  l.a_bytes = (py + kPadTop + kPadBottom) * l.pa;
  // Post patch rows: left margin so that every lane window starts >= 0.
  const int cq0 = v.nce - 1;
  int ml = 16 * cq0 + 16 - qx;
  if (ml < 0) ml = 0;
  ml = (ml + 15) / 16 * 16;
  l.ml = ml;
  // Furthest byte touched: window start (n = 0) + 16 * NCE + 4 bytes read-ahead.
  int need = ml + qx - 1 - 16 * cq0 + 16 * v.nce + 4;
  need = std::max(need, ml + (qx + 15) / 16 * 16);
  int pb16 = (need + 15) / 16;
  // pitch / 4 mod 32 in {20, 12, ...}: keep 4 consecutive rows on distinct
  // banks for the dword reads: use pitch = 16 * odd with (pitch / 4) % 8 == 4.
  while (((pb16 * 4) % 8) != 4) ++pb16;
  l.pb = pb16 * 16;
  l.b_bytes = (qy + 3) * l.pb;
  l.a_bytes = (l.a_bytes + 15) / 16 * 16;
  l.b_bytes = (l.b_bytes + 15) / 16 * 16;
  return l;
}

bool same_size(const SfmXcorrDesc* d) {
  return d->patch[1] == d->post_patch[1] && d->patch[2] == d->post_patch[2] &&
         d->patch[2] <= 64 * kPrepCols;  // columns per lane in the prep kernel
}

struct Ws {
  int* c16;
  long long c16_stride;
  PatchParams* pp;
  int* integ[2];
  long long stride[2];
  float* gtab;
  float* aux;
  int aux_n;
  float* tbound;
  int* counter;
  size_t bytes;
};

Ws carve_ws(const SfmXcorrDesc* d, void* base) {
  sfm::Carver c(base);
  Ws w;
  std::memset(&w, 0, sizeof(w));
  const size_t B = d->batch;
  w.pp = c.take<PatchParams>(B);
  w.counter = c.take<int>(64);  // queue head, clk probe
  if (same_size(d)) {
    w.aux_n = std::max(d->patch[1], d->patch[2]) + 1;
    w.gtab = c.take<float>(B * d->patch[1] * d->patch[2]);
    w.aux = c.take<float>(B * (4 * w.aux_n + 4));
    w.tbound = c.take<float>(B * kBoundStride);
    // column sums above every 16th row + row-sum prefixes (kModeSameExactLazyG)
    w.c16_stride = 2LL * (d->patch[1] / 16 + 1) * d->patch[2] + d->patch[1] + 1;
    w.c16_stride = (w.c16_stride + 63) / 64 * 64;
    w.c16 = c.take<int>(B * (size_t)w.c16_stride);
  } else {
    w.stride[0] = (long long)(d->patch[1] + 1) * (d->patch[2] + 1);
    w.stride[1] = (long long)(d->post_patch[1] + 1) * (d->post_patch[2] + 1);
    w.integ[0] = c.take<int>(B * w.stride[0]);
    w.integ[1] = c.take<int>(B * w.stride[1]);
  }
  w.bytes = c.total();
  return w;
}

// Geometry, image pointers, LDS layout and the tile schedule shared by every mode.
int fill_common(const SfmXcorrDesc* d, const Layout& l, MfmaArgs* ap) {
  MfmaArgs& a = *ap;
  std::memset(&a, 0, sizeof(a));
  a.img[0] = static_cast<const unsigned char*>(d->pre_image);
  a.img[1] = static_cast<const unsigned char*>(d->post_image);
  a.mask[0] = d->pre_mask;
  a.mask[1] = d->post_mask;
  for (int k = 0; k < 2; ++k) {
    a.ishape[0][k] = d->pre_shape[1 + k];
    a.ishape[1][k] = d->post_shape[1 + k];
    a.mshape[0][k] = d->pre_mask_shape[1 + k];
    a.mshape[1][k] = d->post_mask_shape[1 + k];
    a.P[k] = d->patch[1 + k];
    a.Q[k] = d->post_patch[1 + k];
    a.S[k] = a.P[k] + a.Q[k] - 1;
  }
  a.starts[0] = d->pre_starts;
  a.starts[1] = d->post_starts;
  a.batch = d->batch;
  a.use_mean = d->use_mean;
  a.mean = d->mean;
  {
    int rows = 0, pitch = 0;
    sfm::mfma_i8_padded_dims(d, &rows, &pitch);
    a.sx_pitch = pitch;
    a.s_stride = (long long)rows * pitch;
  }
  a.pa = l.pa;
  a.pb = l.pb;
  a.ml = l.ml;
  a.a_bytes = l.a_bytes;
  a.b_bytes = l.b_bytes;
  // Schedule: dy tiles sorted by the number of patch rows they visit, longest first.
  const int np = (a.S[0] + 15) / 16;
  std::vector<std::pair<int, int>> work;
  for (int p = 0; p < np; ++p) {
    const int dy0 = 16 * p - (a.Q[0] - 1);
    const int ylo = std::max(0, -dy0 - 15), yhi = std::min(a.Q[0], a.P[0] - dy0);
    work.push_back({std::max(0, (yhi - ylo + 3) / 4), p});
  }
  std::sort(work.begin(), work.end(),
            [](const std::pair<int, int>& x, const std::pair<int, int>& y) {
              return x.first > y.first || (x.first == y.first && x.second < y.second);
            });
  if (work.size() > sizeof(a.order) / sizeof(a.order[0]))
    return sfm::fail(SFM_ERR_INVALID, "too many dy tiles");
  a.n_order = static_cast<int>(work.size());
  for (size_t i = 0; i < work.size(); ++i) a.order[i] = work[i].second;
  if (l.nca > 10) {
    // search-window variants: a tile job is one column half of a row tile (p | half << 8)
    if (2 * work.size() > sizeof(a.order) / sizeof(a.order[0]))
      return sfm::fail(SFM_ERR_INVALID, "too many dy tiles");
    a.n_order = static_cast<int>(2 * work.size());
    for (size_t i = 0; i < work.size(); ++i) {
      a.order[2 * i] = work[i].second;
      a.order[2 * i + 1] = work[i].second | (1 << 8);
    }
  }
  return SFM_OK;
}

// Masked path.  Pass index -> operand planes (pre, post); pass 0 runs for every
// patch, the others only where a side has masked pixels (masked_classify_kernel).
const int kMaskedPasses[8][2] = {
    {kPlaneVal, kPlaneVal},     {kPlaneVal, kPlaneValid},  {kPlaneValid, kPlaneVal},
    {kPlaneValid, kPlaneValid}, {kPlaneSqHi, kPlaneValid}, {kPlaneSqLo, kPlaneValid},
    {kPlaneValid, kPlaneSqHi},  {kPlaneValid, kPlaneSqLo}};

// SFM_MASKED_FAST=0 (tests): every patch takes all eight passes.
bool masked_all_passes() {
  return !sfm::option_on("SFM_MASKED_FAST");
}

struct MaskedWs {
  PatchParams* pp;
  int *nvalid, *cls, *first, *items, *n_items, *ov_lb, *sweep0, *tab, *raw0, *rawd;
  int group, n_groups;
  long long tab_elems, raw_stride;
  size_t bytes;
};

MaskedWs carve_masked(const SfmXcorrDesc* d, void* base) {
  sfm::Carver c(base);
  MaskedWs w;
  std::memset(&w, 0, sizeof(w));
  int rows = 0, pitch = 0;
  sfm::mfma_i8_padded_dims(d, &rows, &pitch);
  const size_t B = d->batch;
  w.pp = c.take<PatchParams>(B);
  w.nvalid = c.take<int>(2 * B);
  w.cls = c.take<int>(B);
  w.first = c.take<int>(B);
  w.items = c.take<int>(7 * B);
  w.n_items = c.take<int>(16);
  // reference batches in this call: the tolerances are maxima over a batch
  w.group = d->group > 0 && d->group < d->batch ? d->group : d->batch;
  w.n_groups = (d->batch + w.group - 1) / w.group;
  w.ov_lb = c.take<int>(w.n_groups);
  w.sweep0 = c.take<int>(B);
  // + 64 ints: consecutive tables (and product surfaces below) of a patch are read
  // together; strides that are multiples of 4 KB would put them on one memory channel
  w.tab_elems = (long long)d->patch[1] * d->patch[2] + 64;
  w.tab = c.take<int>(B * 4 * (size_t)w.tab_elems);
  w.raw_stride = (long long)rows * pitch + 64;
  w.raw0 = c.take<int>(B * (size_t)w.raw_stride);
  w.rawd = c.take<int>(B * 7 * (size_t)w.raw_stride);
  w.bytes = c.total();
  return w;
}

// --- mfma_i8_surface in steps ------------------------------------------------

// Workspace pointers, the output surface and the measurement knobs.
void fill_workspace(const Ws& w, float* surface, MfmaArgs* ap) {
  MfmaArgs& a = *ap;
  a.pp = w.pp;
  a.integ[0] = w.integ[0];
  a.integ[1] = w.integ[1];
  a.integ_stride[0] = w.stride[0];
  a.integ_stride[1] = w.stride[1];
  a.gtab = w.gtab;
  a.c16 = w.c16;
  a.c16_stride = w.c16_stride;
  a.aux = w.aux;
  a.aux_n = w.aux_n;
  a.tbound = w.tbound;  // read (not used) by every same-size launch
  a.surface = surface;
  a.work_counter = sfm::measure_option_on("SFM_MFMA_QUEUE") ? w.counter : nullptr;
  a.clk = reinterpret_cast<long long*>(w.counter + 16);
  a.prio_mode = sfm::measure_option_int("SFM_MFMA_PRIO", 0);
}

// Fused first-peak search: its buffers, and the exact pruning of dy tiles that
// cannot matter to the peak statistics.
void fill_peaks(const SfmXcorrDesc* d, const sfm::FusedPeaks& fp, bool same, const Variant& v,
                MfmaArgs* ap) {
  MfmaArgs& a = *ap;
  a.do_peaks = 1;
  a.threshold_rel = d->threshold_rel;
  a.min_distance = d->min_distance;
  a.cand_cap = fp.cand_cap;
  a.idx1 = fp.idx1;
  a.v1 = fp.v1;
  a.zero_is_peak = fp.zero_is_peak;
  a.cand_count = fp.cand_count;
  a.cand_val = fp.cand_val;
  a.cand_idx = fp.cand_idx;
  a.bitmap = fp.bitmap;
  a.group = fp.group;
  a.bitmap_words = fp.bitmap_words;
  a.hot_cap = fp.hot_cap;
  a.hot_count = fp.hot_count;
  a.hot_val = fp.hot_val;
  a.hot_idx = fp.hot_idx;
  a.skipmask = fp.skipmask;
  a.guard = std::max(d->min_distance, 2 * d->peak_radius[1]);
  a.guard_x = std::max(d->min_distance, 2 * d->peak_radius[2]);
  // rows: the sharpness window as peaks_second_kernel places it, and the max filter
  a.win = std::min(2 * std::max(d->peak_radius[1], 0) + 1, a.S[0]);
  a.win_top = a.S[0] - a.win;
  a.guard_md = d->min_distance;
  if (sfm::measure_option_tri("SFM_MFMA_GUARD_2R") == 1) {
    // the band as it was: `guard` rows around every hot row and every tile (a
    // window of one row and a max filter of `guard` rows ask for exactly that)
    a.win = 1;
    a.win_top = a.S[0] - 1;
    a.guard_md = a.guard;
  }
  a.nq = v.nca + v.nce - 1;
  a.prune_k[0] = col_skip_lo(a.nq);
  a.prune_k[1] = col_skip_hi(a.nq);
  a.prune_k[2] = col_skip_2(a.nq);
  a.prune_k[3] = col_skip_3(a.nq);
  a.probe = sfm::measure_option_on("SFM_MFMA_PROBE");  // "0": no seed probe
  a.count_tiles = sfm::profiling() ? 1 : 0;
  // least number of row groups between two tests inside the row loop of the
  // lazy modes ("0": no tests); each test schedules the next, see check_after
  a.early = sfm::option_int("SFM_MFMA_EARLY", 1);
  a.touch_all = sfm::measure_option_tri("SFM_MFMA_TOUCH_ALL") == 1;
  a.narrow = sfm::option_int("SFM_MFMA_NARROW", 64);   // widest narrowing allowed (0: off)
  if (a.early < 0 || a.P[0] > kEarlyRows) a.early = 0;
  a.prune = same && prune_enabled() && a.n_order <= kBoundTiles &&
            a.P[0] <= 16 * kBlkRows && a.P[1] <= 16 * kBlkCols &&
            a.P[0] <= kBoundRows && d->threshold_rel > 0.f && d->threshold_rel <= 1.f &&
            a.guard >= 0;
}

constexpr int mode_of(bool same, bool exact, bool lazy, bool lazy_g) {
  return !same ? kModeGeneral
         : exact ? (lazy_g ? kModeSameExactLazyG : lazy ? kModeSameExactLazy : kModeSameExact)
                 : (lazy ? kModeSameLazy : kModeSame);
}

int choose_mode(const SfmXcorrDesc* d, const Variant& v, const MfmaArgs& a, bool same,
                bool peaks) {
  const bool exact = same && d->patch[2] == 16 * v.nca && exact_enabled();
  // lazy surface stores: the flow path only (fused peak search: nobody else
  // reads the surface), tile masks of 31 bits, SFM_MFMA_LAZY=0 switches it off
  bool lazy = same && peaks && a.n_order <= 31 && a.skipmask != nullptr;
  if (!sfm::option_on("SFM_MFMA_LAZY")) lazy = false;
  // The correction table built in the epilogue of the tiles that are stored instead
  // of by the prep kernel (kModeSameExactLazyG): pays where few tiles reach an
  // epilogue, i.e. with the pruning on (the un-pruned launch, every tile finished,
  // keeps the table).  SFM_MFMA_LAZYG=0: off.
  const bool lazy_g = exact && lazy && a.prune && sfm::option_on("SFM_MFMA_LAZYG") &&
                      a.P[0] % 16 == 0 && a.P[0] <= 160 && a.P[1] <= 160 && a.P[0] >= 32;
  return mode_of(same, exact, lazy, lazy_g);
}

// The correlation kernel of geometry kVariants[vi]: the unit that instantiates it.
int launch_mode(int vi, const MfmaArgs& a, int mode, int grid, size_t lds,
                hipStream_t st) {
  const Variant v = vi >= 0 && vi < static_cast<int>(sizeof(kVariants) / sizeof(kVariants[0]))
                        ? kVariants[vi] : Variant{0, 0};
#define SFM_MFMA_CASE(NCA, NCE) \
  if (v.nca == NCA && v.nce == NCE) return launch_variant<NCA, NCE>(a, mode, grid, lds, st);
  SFM_MFMA_GEOMETRIES(SFM_MFMA_CASE)
#undef SFM_MFMA_CASE
  return sfm::fail(SFM_ERR_INVALID, "no MFMA variant");
}

}  // namespace
}  // namespace mfma

using namespace mfma;

bool mfma_i8_eligible(const SfmXcorrDesc* d) {
  if (!d || d->ndim != 2 || d->dtype != SFM_DTYPE_U8) return false;
  if (d->patch[0] != 1 || d->post_patch[0] != 1) return false;
  const int py = d->patch[1], px = d->patch[2];
  const int qy = d->post_patch[1], qx = d->post_patch[2];
  const int vi = pick_variant(px, qx);
  if (vi < 0) return false;
  if (py < 1 || qy < 1 || qy > py || qx > px) return false;
  if (kVariants[vi].nca <= 10) {
    if ((long long)py * px > 32768) return false;      // prep kernel LDS copy
  } else {
    // search-window variants: un-masked, the prep kernel's LDS copy of a patch and the
    // correlation kernel's two patches + scratch within one CU's LDS
    if (d->pre_mask || d->post_mask) return false;
    // (general mode only, launch_variant: a same-size pair 161 wide is the one shape that
    // picks these variants and the same-size mode -- it takes another path)
    if (same_size(d)) return false;
    if ((long long)py * px > 140 * 1024) return false;
    const Layout l = make_layout(d, kVariants[vi]);
    if ((size_t)l.a_bytes + l.b_bytes + 8 * 1024 > kLdsPerCu) return false;
  }
  if ((long long)qy * qx * 16384 > 0x7fffffffLL) return false;  // int32 sums
  if ((py + qy - 1 + 15) / 16 > kMaxTileJobs) return false;
  // (the staging loads are 16 bytes wide and clamped into the image)
  if ((long long)d->pre_shape[1] * d->pre_shape[2] < 16 ||
      (long long)d->post_shape[1] * d->post_shape[2] < 16)
    return false;
  if ((reinterpret_cast<uintptr_t>(d->pre_image) & 3) ||
      (reinterpret_cast<uintptr_t>(d->post_image) & 3))
    return false;
  return true;
}

size_t mfma_i8_workspace_bytes(const SfmXcorrDesc* d) {
  if (d->pre_mask || d->post_mask) return carve_masked(d, nullptr).bytes;
  return carve_ws(d, nullptr).bytes;
}

void mfma_i8_padded_dims(const SfmXcorrDesc* d, int* rows, int* pitch) {
  const int vi = pick_variant(d->patch[2], d->post_patch[2]);
  const int sy = d->patch[1] + d->post_patch[1] - 1;
  *rows = (sy + 15) / 16 * 16;
  *pitch = vi < 0 ? 0 : 16 * (kVariants[vi].nca + kVariants[vi].nce - 1);
}

int mfma_i8_surface(const SfmXcorrDesc* d, void* ws_base, float* surface,
                    const FusedPeaks* fp) {
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const int vi = pick_variant(d->patch[2], d->post_patch[2]);
  if (vi < 0) return fail(SFM_ERR_INVALID, "patch too wide for the MFMA path");
  const Layout l = make_layout(d, kVariants[vi]);
  const Ws w = carve_ws(d, ws_base);
  MfmaArgs a;
  if (int rc = fill_common(d, l, &a)) return rc;
  fill_workspace(w, surface, &a);
  const bool same = same_size(d);
  if (fp) fill_peaks(d, *fp, same, kVariants[vi], &a);
  const int mode = choose_mode(d, kVariants[vi], a, same, fp != nullptr);
  // Region behind the patches: the four 1-D correction arrays, reused as the
  // arg-max scratch of the fused peak search, then the state words (LdsTail).
  size_t r_bytes = same ? (size_t)4 * w.aux_n * 4 : 0;
  r_bytes = std::max(r_bytes, (size_t)kThreads * 8);
  r_bytes = (r_bytes + 15) / 16 * 16;
  a.r_bytes = static_cast<int>(r_bytes);
  if (int rc = launch_prep(a, mode, kVariants[vi], st)) return rc;
  const size_t lds = (size_t)l.a_bytes + l.b_bytes + r_bytes + sizeof(LdsTail);
  const int grid = d->batch;  // capped to the resident workgroups in launch_one
  if (int rc = launch_mode(vi, a, mode, grid, lds, st)) return rc;
  if (fp) return launch_first_peak(a, st);
  return SFM_OK;
}

// Masked (Padfield) correlation on the matrix cores: writes the normalised
// surface, padded to whole tiles [batch, rows, pitch]; `maxima` = scratch for
// the batch maxima (flow_field.py:137, 151), two words per reference batch
// (`d->group` patches); `smax` (optional, zeroed by the caller) receives the
// ordered bits of every surface maximum.
int mfma_i8_masked(const SfmXcorrDesc* d, void* ws_base, float* surface,
                   unsigned int* maxima, unsigned int* smax, float* blkmax) {
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const int vi = pick_variant(d->patch[2], d->post_patch[2]);
  if (vi < 0) return fail(SFM_ERR_INVALID, "patch too wide for the MFMA path");
  const Layout l = make_layout(d, kVariants[vi]);
  MaskedWs w = carve_masked(d, ws_base);
  MfmaArgs a;
  if (int rc = fill_common(d, l, &a)) return rc;
  for (int k = 0; k < 2; ++k)
    if (a.mask[k] && (a.mshape[k][0] < (k ? a.Q[0] : a.P[0]) ||
                      a.mshape[k][1] < (k ? a.Q[1] : a.P[1])))
      return fail(SFM_ERR_INVALID, "mask smaller than patch");
  a.pp = w.pp;
  a.prio_mode = 1;
  a.nvalid = w.nvalid;
  if (int rc = launch_prep_masked(a, st)) return rc;
  SFM_HIP_CHECK(hipMemsetAsync(maxima, 0, 2 * w.n_groups * sizeof(unsigned int), st));
  SFM_HIP_CHECK(hipMemsetAsync(w.ov_lb, 0, w.n_groups * sizeof(int), st));
  size_t r_bytes = (size_t)kThreads * 8;
  a.r_bytes = static_cast<int>(r_bytes);
  const size_t lds = (size_t)l.a_bytes + l.b_bytes + r_bytes + kLdsTailHead;
  MaskedFastArgs g;
  std::memset(&g, 0, sizeof(g));
  g.pp = w.pp;
  g.nvalid = w.nvalid;
  g.cls = w.cls;
  g.first = w.first;
  g.items = w.items;
  g.n_items = w.n_items;
  g.tab = w.tab;
  g.tab_elems = w.tab_elems;
  g.raw0 = w.raw0;
  g.rawd = w.rawd;
  g.elems = a.s_stride;
  g.raw_stride = w.raw_stride;
  a.raw_stride = w.raw_stride;
  g.pitch = a.sx_pitch;
  for (int k = 0; k < 2; ++k) {
    g.img[k] = a.img[k];
    g.mask[k] = a.mask[k];
    g.ishape[k][0] = a.ishape[k][0];
    g.ishape[k][1] = a.ishape[k][1];
    g.mshape[k][0] = a.mshape[k][0];
    g.mshape[k][1] = a.mshape[k][1];
    g.P[k] = a.P[k];
    g.Q[k] = a.Q[k];
    g.S[k] = a.S[k];
  }
  g.batch = d->batch;
  g.all_passes = masked_all_passes() ? 1 : 0;
  g.dead_rows = sfm::option_on("SFM_MASKED_DEADROWS");
  g.xcd_map = sfm::option_on("SFM_PHASE_XCD");
  g.maxima = maxima;
  {
    // class 0 maxima from the axes (SFM_MASKED_AXISMAX=0: the sweep over all shifts)
    g.axis_max = sfm::option_on("SFM_MASKED_AXISMAX") && a.P[0] == a.Q[0] && a.P[1] == a.Q[1] &&
                 a.P[0] <= kAxisMaxLen && a.P[1] <= kAxisMaxLen;
  }
  g.group = w.group;
  g.ov_lb = w.ov_lb;
  g.sweep0 = w.sweep0;
  g.out = surface;
  g.smax = smax;
  g.blkmax = smax ? blkmax : nullptr;
  const int rows_per_wg = kWaves * kAsmRowsPerWave;
  g.row_blocks = (a.S[0] + rows_per_wg - 1) / rows_per_wg;
  if (int rc = launch_masked_tables(g, st)) return rc;
  MfmaArgs c = a;
  c.plane[0] = kMaskedPasses[0][0];
  c.plane[1] = kMaskedPasses[0][1];
  c.raw_out = w.raw0;
  c.ov_lb = g.dead_rows ? w.ov_lb : nullptr;
  c.ov_group = w.group;
  if (int rc = launch_mode(vi, c, kModeRaw, d->batch, lds, st)) return rc;
  c.ov_lb = nullptr;  // the other products feed the maxima of every element
  c.raw_out = w.rawd;
  c.list = w.items;
  c.n_list = w.n_items;
  const long long extra = 7LL * d->batch;
  if (int rc = launch_mode(vi, c, kModeRaw, static_cast<int>(std::min<long long>(extra, 1 << 20)),
                           lds, st))
    return rc;
  return launch_masked_assembly(g, st);
}

}  // namespace sfm
