// The fine flows of a tile montage, filtered as one ragged batch:
//
//   sfm_filter_tile_flows  <->  per tile pair, flow_utils.clean_flow
//                               (flow_utils.py:37-78) followed by
//                               flow_utils.reconcile_flows (:81-135) of that flow
//
// A montage has thousands of tile pairs of a few thousand vectors each, every
// pair with its own extent.  One launch filters them all: one workgroup per
// pair, the pair's two channels and one int per vector in LDS from the load to
// the store.  A stage computes a `bad` flag per vector from the stage's input,
// and the flags are applied behind a workgroup barrier, so a stage never sees
// its own masking.  Values are only copied or replaced by NaN.  The window,
// border and comparison rules are those of sfm_flowutils.hip (sfm_flowfilter.h);
// borders, windows and the invalid count are those of the pair's own [h, w].
#include "sfm_common.h"
#include "sfm_flowfilter.h"

#include <hip/hip_runtime.h>

namespace {

using namespace sfm::flowfilter;

constexpr int kBlock = 256;
// LDS of a workgroup: channel 0, channel 1 (float) and the flag / parent (int)
// of every vector, then the invalid count.
constexpr size_t kLdsBytes = 160 * 1024;
constexpr size_t kNodeBytes = 2 * sizeof(float) + sizeof(int);
constexpr size_t kTailBytes = 64;
// 13648 vectors fit; the cap is that rounded down to whole waves: 13632
constexpr int kMaxNodes = static_cast<int>((kLdsBytes - kTailBytes) / kNodeBytes) / 64 * 64;
// the parent array lives in LDS
constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;

struct TileArgs {
  const float* flows;  // [C, n, Y, X]
  float* out;          // [2, n, Y, X]
  const int* extents;  // [n, 2]
  int C, n, Y, X;
  int cap;             // vectors the LDS arrays of this launch hold
  int do_clean, do_reconcile;
  double min_ratio, min_sharp, max_mag, clean_dev;  // compared in double, see SfmCleanFlowDesc
  double max_grad, max_dev;
  long long min_patch;
};

// NaN where the stage's flag is set.  Every thread visits the vectors it flagged
// itself; the barriers separate the flags from the reads of the next stage.
__device__ __forceinline__ void apply_flags(float* v0, float* v1, const int* flag, int nodes) {
  __syncthreads();
  for (int i = threadIdx.x; i < nodes; i += kBlock)
    if (flag[i]) {
      v0[i] = NAN;
      v1[i] = NAN;
    }
  __syncthreads();
}

__global__ void __launch_bounds__(kBlock) tile_flows_kernel(TileArgs a) {
  extern __shared__ float lds[];
  float* v0 = lds;
  float* v1 = lds + a.cap;
  int* aux = reinterpret_cast<int*>(lds + 2 * a.cap);  // stage flag, then parent / size
  int* n0 = aux + a.cap;                               // invalid vectors of the pair
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  const int h = a.extents[2 * p], w = a.extents[2 * p + 1];
  const int nodes = h * w;  // <= cap (checked by the entry point)
  const long long plane = (long long)a.Y * a.X;
  const long long cs = (long long)a.n * plane;  // channel stride
  const float* in = a.flows + p * plane;
  const auto at0 = [&](int yy, int xx) { return v0[yy * w + xx]; };
  const auto at1 = [&](int yy, int xx) { return v1[yy * w + xx]; };

  if (tid == 0) *n0 = 0;
  for (int i = tid; i < nodes; i += kBlock) {
    const int y = i / w, x = i - y * w;
    const long long g = (long long)y * a.X + x;
    v0[i] = in[g];
    v1[i] = in[cs + g];
  }
  __syncthreads();

  // -- clean_flow: one flag from the four tests, all of them on the unmasked
  //    input (flow_utils.py:74 takes the median before any masking)
  if (a.do_clean) {
    for (int i = tid; i < nodes; i += kBlock) {
      const int y = i / w, x = i - y * w;
      bool bad = false;
      if (a.C == 4) {
        const long long g = (long long)y * a.X + x;
        bad = peak_bad(in[2 * cs + g], in[3 * cs + g], a.min_sharp, a.min_ratio);
      }
      const float c0 = v0[i], c1 = v1[i];
      // np.max over the components propagates NaN, and NaN > t is false
      if (!isnan(c0) && !isnan(c1)) {
        if (a.max_mag > 0.0) bad = bad || above(fmaxf(fabsf(c0), fabsf(c1)), a.max_mag);
        if (a.clean_dev > 0.0)
          bad = bad || deviation_bad(fabsf(median3x3(at0, y, x, h, w) - c0),
                                     fabsf(median3x3(at1, y, x, h, w) - c1), a.clean_dev);
      }
      aux[i] = bad;
    }
    apply_flags(v0, v1, aux, nodes);
  }
  if (a.do_reconcile) {
    // -- gradient: a neighbour beyond the pair's own border is 0
    if (a.max_grad > 0.0) {
      for (int i = tid; i < nodes; i += kBlock) {
        const int y = i / w, x = i - y * w;
        const float l = x > 0 ? v0[i - 1] : 0.f;
        const float r = x + 1 < w ? v0[i + 1] : 0.f;
        const float u = y > 0 ? v1[i - w] : 0.f;
        const float d = y + 1 < h ? v1[i + w] : 0.f;
        aux[i] = gradient_bad(v0[i], v1[i], l, r, u, d, a.max_grad);
      }
      apply_flags(v0, v1, aux, nodes);
    }
    // -- deviation from the 3 x 3 median of nan_to_num, reflected at the pair's border
    if (a.max_dev > 0.0) {
      for (int i = tid; i < nodes; i += kBlock) {
        const int y = i / w, x = i - y * w;
        aux[i] = deviation_bad(fabsf(median3x3(at0, y, x, h, w) - v0[i]),
                               fabsf(median3x3(at1, y, x, h, w) - v1[i]), a.max_dev);
      }
      apply_flags(v0, v1, aux, nodes);
    }
    // -- small components, 4-connected: union-find in LDS
    if (a.min_patch > 0) {
      for (int i = tid; i < nodes; i += kBlock) {
        const bool valid = !isnan(v0[i]) && !isnan(v1[i]);
        aux[i] = valid ? i : -1;
        if (!valid) atomicAdd(n0, 1);
      }
      __syncthreads();
      for (int i = tid; i < nodes; i += kBlock) {
        if (load_parent<kScope>(aux, i) < 0) continue;
        const int y = i / w, x = i - y * w;
        // right and down neighbours: the cross structure
        if (x + 1 < w && load_parent<kScope>(aux, i + 1) >= 0) unite<kScope>(aux, i, i + 1);
        if (y + 1 < h && load_parent<kScope>(aux, i + w) >= 0) unite<kScope>(aux, i, i + w);
      }
      __syncthreads();
      // parent[i] <- root.  The tree is final, and an entry another thread has
      // compressed meanwhile is still an ancestor.
      for (int i = tid; i < nodes; i += kBlock) {
        int r = load_parent<kScope>(aux, i);
        if (r < 0) continue;
        for (int q = load_parent<kScope>(aux, r); q != r; q = load_parent<kScope>(aux, r)) r = q;
        __hip_atomic_store(aux + i, r, __ATOMIC_RELAXED, kScope);
      }
      __syncthreads();
      // a root holds -(size + 1) from here on: -2 for itself ...
      for (int i = tid; i < nodes; i += kBlock)
        if (aux[i] == i) aux[i] = -2;
      __syncthreads();
      // ... and one less for every other vector of its component
      for (int i = tid; i < nodes; i += kBlock)
        if (aux[i] >= 0) atomicAdd(aux + aux[i], -1);
      __syncthreads();
      // np.unique counts the background label too: when 0 < n0 < min_patch_size the
      // invalid vectors of the pair become all-NaN as well
      const int invalid = *n0;
      for (int i = tid; i < nodes; i += kBlock) {
        const int q = aux[i];
        const int cnt = q == -1 ? invalid : -(q >= 0 ? aux[q] : q) - 1;
        if (cnt < a.min_patch) {
          v0[i] = NAN;
          v1[i] = NAN;
        }
      }
      __syncthreads();
    }
  }

  float* out = a.out + p * plane;
  for (long long j = tid; j < plane; j += kBlock) {
    const int y = static_cast<int>(j / a.X), x = static_cast<int>(j - (long long)y * a.X);
    const bool inside = y < h && x < w;
    out[j] = inside ? v0[y * w + x] : NAN;
    out[cs + j] = inside ? v1[y * w + x] : NAN;
  }
}

}  // namespace

extern "C" int sfm_filter_tile_flows_max_nodes(void) { return kMaxNodes; }

extern "C" int sfm_filter_tile_flows(const SfmTileFlowsDesc* d, float* out) {
  if (!d || !d->flows || !d->extents || !d->extents_device || !out)
    return sfm::fail(SFM_ERR_INVALID, "filter_tile_flows: NULL argument");
  if (d->channels != 2 && d->channels != 4)
    return sfm::fail(SFM_ERR_INVALID, "filter_tile_flows: %d channels, need 2 or 4",
                     d->channels);
  if (d->n < 0 || d->padded_shape[0] < 1 || d->padded_shape[1] < 1)
    return sfm::fail(SFM_ERR_INVALID, "filter_tile_flows: bad batch size / padded shape");
  if (d->n == 0) return SFM_OK;
  int largest = 0;
  for (int p = 0; p < d->n; ++p) {
    const int h = d->extents[2 * p], w = d->extents[2 * p + 1];
    if (h < 1 || w < 1 || h > d->padded_shape[0] || w > d->padded_shape[1])
      return sfm::fail(SFM_ERR_INVALID,
                       "filter_tile_flows: pair %d has extent [%d, %d] outside [1, 1] .. [%d, %d]",
                       p, h, w, d->padded_shape[0], d->padded_shape[1]);
    const long long nodes = (long long)h * w;
    if (nodes > kMaxNodes)
      return sfm::fail(SFM_ERR_INVALID,
                       "filter_tile_flows: pair %d has %lld vectors, a workgroup holds %d", p,
                       nodes, kMaxNodes);
    largest = nodes > largest ? static_cast<int>(nodes) : largest;
  }
  TileArgs a;
  a.flows = d->flows;
  a.out = out;
  a.extents = d->extents_device;
  a.C = d->channels;
  a.n = d->n;
  a.Y = d->padded_shape[0];
  a.X = d->padded_shape[1];
  // LDS is sized by the largest pair of the launch: batches of small strips get
  // several workgroups per CU
  a.cap = (largest + 3) & ~3;
  a.do_clean = d->do_clean != 0;
  a.do_reconcile = d->do_reconcile != 0;
  a.min_ratio = d->min_peak_ratio;
  a.min_sharp = d->min_peak_sharpness;
  a.max_mag = d->max_magnitude;
  a.clean_dev = d->clean_max_deviation;
  a.max_grad = d->max_gradient;
  a.max_dev = d->max_deviation;
  a.min_patch = d->min_patch_size;
  const size_t lds = (size_t)a.cap * kNodeBytes + kTailBytes;
  static_assert((size_t)((kMaxNodes + 3) & ~3) * kNodeBytes + kTailBytes <= kLdsBytes,
                "the largest pair fits the LDS of a CU");
  if (int rc = sfm::set_lds(&tile_flows_kernel, lds)) return rc;
  hipLaunchKernelGGL(tile_flows_kernel, dim3(static_cast<unsigned>(d->n)), dim3(kBlock), lds,
                     static_cast<hipStream_t>(d->stream), a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}
