// Flow-field clean-up on the device: the
// quality filter that runs between flow estimation and mesh relaxation.
//
//   sfm_clean_flow      <->  flow_utils.clean_flow (flow_utils.py:37-78)
//   sfm_mask_irregular  <->  map_utils.mask_irregular (map_utils.py:737-786)
//   sfm_range_mask      <->  the dynamic-range mask of stitch_rigid._estimate_offset
//                            (stitch_rigid.py:47-60)
//   sfm_flow_starts     <->  the start-coordinate / targeting arithmetic of
//                            flow_field() (flow_field.py:620-680)
//   sfm_flow_scatter    <->  the result scatter of flow_field() (:701-709)
//   sfm_flow_select     <->  patch selection and np.where of flow_field()
//                            (:570-589, :607, :614-618), one launch
//   sfm_missing_flow_update <-> the accept / update step of a look-back round
//                            of EstimateMissingFlow (processor/flow.py:785, :806-828)
//
// One thread per vector.  The field is small (one vector per patch), so the
// point of the kernel is that the flow can stay in HBM from the correlation
// peaks to the mesh relaxation; it is bound by launch latency.
#include "sfm_common.h"
#include "sfm_flowfilter.h"

#include <hip/hip_runtime.h>

namespace {

// window, border and comparison rules shared with sfm_tileflows.hip
using namespace sfm::flowfilter;

constexpr int kBlock = 256;

struct CleanArgs {
  const float* flow;
  float* out;
  int dim, channels;
  int Z, Y, X;
  double min_ratio, min_sharp, max_mag, max_dev;  // compared in double, see SfmCleanFlowDesc
};

// Median of the (1|3) x 3 x 3 window of nan_to_num(comp) around (z, y, x).
__device__ float window_median(const float* comp, const CleanArgs& a, int z, int y,
                               int x) {
  float w[27];
  int n = 0;
  const int zr = a.dim == 3 ? 1 : 0;
  for (int dz = -zr; dz <= zr; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int zz = reflect(z + dz, a.Z), yy = reflect(y + dy, a.Y),
                  xx = reflect(x + dx, a.X);
        insert_sorted(w, n, nan_to_num(comp[((long long)zz * a.Y + yy) * a.X + xx]));
      }
  return w[n / 2];
}

__global__ void __launch_bounds__(kBlock) clean_flow_kernel(CleanArgs a) {
  const long long n_vec = (long long)a.Z * a.Y * a.X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n_vec) return;
  const int x = static_cast<int>(i % a.X);
  const int y = static_cast<int>((i / a.X) % a.Y);
  const int z = static_cast<int>(i / ((long long)a.X * a.Y));
  bool bad = false;
  if (a.channels == a.dim + 2) {
    bad = peak_bad(a.flow[a.dim * n_vec + i], a.flow[(a.dim + 1) * n_vec + i], a.min_sharp,
                   a.min_ratio);
  }
  float v[3];
  bool any_nan = false;
  for (int c = 0; c < a.dim; ++c) {
    v[c] = a.flow[c * n_vec + i];
    any_nan = any_nan || isnan(v[c]);
  }
  // np.max over the components propagates NaN, and NaN > t is false
  if (!any_nan) {
    if (a.max_mag > 0.0) {
      float m = 0.f;
      for (int c = 0; c < a.dim; ++c) m = fmaxf(m, fabsf(v[c]));
      bad = bad || above(m, a.max_mag);
    }
    if (a.max_dev > 0.0) {
      float m = 0.f;
      for (int c = 0; c < a.dim; ++c) {
        const float med = window_median(a.flow + c * n_vec, a, z, y, x);
        m = fmaxf(m, fabsf(med - v[c]));
      }
      bad = bad || above(m, a.max_dev);
    }
  }
  for (int c = 0; c < a.dim; ++c) a.out[c * n_vec + i] = bad ? NAN : v[c];
}

// T: element type of the map (float, or double for sfm_mask_irregular_f64)
template <typename T>
struct IrregArgs {
  T* map;              // [2, Y, X]
  unsigned char* bad;  // [Y, X]
  int* n_valid;        // counting fill only
  int Y, X, iters;
  double sx, sy, lo_x, lo_y, hi_x, hi_y;
};

// bad before dilation (map_utils.py:768-775); out-of-range nodes are not bad.
template <typename T>
__device__ __forceinline__ bool irregular_at(const IrregArgs<T>& a, int y, int x) {
  if (y < 0 || y >= a.Y || x < 0 || x >= a.X) return false;
  const long long n = (long long)a.Y * a.X, i = (long long)y * a.X + x;
  // np.diff in the map's type, padded with 0 at the far edge; the float64 stride
  // scalar promotes the sum, and the comparisons, to double (NumPy >= 2)
  const double dx = static_cast<double>(x + 1 < a.X ? a.map[i + 1] - a.map[i] : T(0)) + a.sx;
  const double dy =
      static_cast<double>(y + 1 < a.Y ? a.map[n + i + a.X] - a.map[n + i] : T(0)) + a.sy;
  return dx < a.lo_x || dy < a.lo_y || dx > a.hi_x || dy > a.hi_y;
}

// `iters` dilations with the full 3 x 3 structure == OR over the square window
// of radius `iters` (border value 0).
template <typename T>
__global__ void __launch_bounds__(kBlock) irregular_mark_kernel(IrregArgs<T> a) {
  const long long n = (long long)a.Y * a.X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  const int x = static_cast<int>(i % a.X), y = static_cast<int>(i / a.X);
  bool bad = false;
  for (int dy = -a.iters; dy <= a.iters && !bad; ++dy)
    for (int dx = -a.iters; dx <= a.iters; ++dx)
      if (irregular_at(a, y + dy, x + dx)) {
        bad = true;
        break;
      }
  a.bad[i] = bad ? 1 : 0;
}

// Second launch: the NaN fill must not feed back into the differences above.
// COUNT: also add up the nodes that keep a component that is not NaN, one
// atomic per wave.
template <typename T, bool COUNT>
__global__ void __launch_bounds__(kBlock) irregular_fill_kernel(IrregArgs<T> a) {
  const long long n = (long long)a.Y * a.X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  const bool bad = i < n && a.bad[i];
  if (bad) {
    a.map[i] = NAN;
    a.map[n + i] = NAN;
  }
  if (COUNT) {
    const bool valid = i < n && !bad && !(isnan(a.map[i]) && isnan(a.map[n + i]));
    const int cnt = __popcll(__ballot(valid));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(a.n_valid, cnt);
  }
}

template <typename T>
int mask_irregular(const SfmMaskIrregularDesc* d, T* coord_map, uint8_t* bad, int* n_valid) {
  if (!d || !coord_map || !bad)
    return sfm::fail(SFM_ERR_INVALID, "mask_irregular: NULL argument");
  if (d->shape[0] < 1 || d->shape[1] < 1 || d->dilation_iters < 0)
    return sfm::fail(SFM_ERR_INVALID, "mask_irregular: bad shape / iterations");
  IrregArgs<T> a;
  a.map = coord_map;
  a.bad = bad;
  a.n_valid = n_valid;
  a.Y = d->shape[0];
  a.X = d->shape[1];
  a.iters = d->dilation_iters;
  a.sx = d->stride[0];
  a.sy = d->stride[1];
  a.lo_x = d->min_dist[0];
  a.lo_y = d->min_dist[1];
  a.hi_x = d->max_dist[0];
  a.hi_y = d->max_dist[1];
  const long long n = (long long)a.Y * a.X;
  const unsigned grid = static_cast<unsigned>((n + kBlock - 1) / kBlock);
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  if (n_valid) SFM_HIP_CHECK(hipMemsetAsync(n_valid, 0, sizeof(int), st));
  hipLaunchKernelGGL(irregular_mark_kernel<T>, dim3(grid), dim3(kBlock), 0, st, a);
  // the float entry has no counter, the double entry always has one
  constexpr bool kCount = sizeof(T) == sizeof(double);
  hipLaunchKernelGGL((irregular_fill_kernel<T, kCount>), dim3(grid), dim3(kBlock), 0, st, a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace

extern "C" int sfm_mask_irregular(const SfmMaskIrregularDesc* d, float* coord_map,
                                  uint8_t* bad) {
  return mask_irregular<float>(d, coord_map, bad, nullptr);
}

extern "C" int sfm_mask_irregular_f64(const SfmMaskIrregularDesc* d, double* coord_map,
                                      uint8_t* bad, int32_t* n_valid) {
  if (!n_valid) return sfm::fail(SFM_ERR_INVALID, "mask_irregular: NULL argument");
  return mask_irregular<double>(d, coord_map, bad, n_valid);
}

// ---------------------------------------------------------------------------
// Dynamic-range mask (stitch_rigid.py:47-60):
//   (maximum_filter(img, size) - minimum_filter(img, size)) < range_limit  [| extra]
// scipy.ndimage filters, mode "reflect", origin 0: the window of pixel i covers
// [i - size / 2, i - size / 2 + size - 1] per axis.  uint8 images subtract in
// uint8 (max >= min: no wrap), float images in float32; the difference, exact
// in double, is compared with the limit in double.  The host passes the
// double that reproduces NumPy's comparison for the image dtype and the kind
// of scalar it was given (stitch_rigid._range_limit).
// ---------------------------------------------------------------------------
namespace {

__device__ __forceinline__ int reflect_any(int i, int n) {
  // whole-period reflection: valid for any overhang
  if (n == 1) return 0;
  const int period = 2 * n;
  int m = i % period;
  if (m < 0) m += period;
  return m < n ? m : period - 1 - m;
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
range_mask_kernel(const T* __restrict__ img, const uint8_t* __restrict__ extra,
                  uint8_t* __restrict__ out, int Y, int X, int size, double limit) {
  const long long n = (long long)Y * X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  const int y = static_cast<int>(i / X), x = static_cast<int>(i % X);
  const int lo = size / 2;
  T mx = img[i], mn = img[i];
  for (int dy = 0; dy < size; ++dy) {
    const int yy = reflect_any(y - lo + dy, Y);
    for (int dx = 0; dx < size; ++dx) {
      const int xx = reflect_any(x - lo + dx, X);
      const T v = img[(long long)yy * X + xx];
      mx = v > mx ? v : mx;
      mn = v < mn ? v : mn;
    }
  }
  // both sides are exact in double
  const T diff = static_cast<T>(mx - mn);
  uint8_t m = static_cast<double>(diff) < limit ? 1 : 0;
  if (extra) m |= extra[i] != 0;
  out[i] = m;
}

}  // namespace

extern "C" int sfm_range_mask(const SfmRangeMaskDesc* d, uint8_t* out) {
  if (!d || !d->image || !out)
    return sfm::fail(SFM_ERR_INVALID, "range_mask: NULL argument");
  if (d->shape[0] < 1 || d->shape[1] < 1 || d->filter_size < 1)
    return sfm::fail(SFM_ERR_INVALID, "range_mask: bad shape / filter size");
  const long long n = (long long)d->shape[0] * d->shape[1];
  const long long grid = (n + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "range_mask: too large");
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  if (d->dtype == SFM_DTYPE_U8)
    hipLaunchKernelGGL(range_mask_kernel<uint8_t>, dim3(static_cast<unsigned>(grid)),
                       dim3(kBlock), 0, st, static_cast<const uint8_t*>(d->image),
                       d->extra_mask, out, d->shape[0], d->shape[1], d->filter_size,
                       d->range_limit);
  else if (d->dtype == SFM_DTYPE_F32)
    hipLaunchKernelGGL(range_mask_kernel<float>, dim3(static_cast<unsigned>(grid)),
                       dim3(kBlock), 0, st, static_cast<const float*>(d->image),
                       d->extra_mask, out, d->shape[0], d->shape[1], d->filter_size,
                       d->range_limit);
  else
    return sfm::fail(SFM_ERR_INVALID, "range_mask: dtype %d", d->dtype);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// Host loop of JAXMaskedXCorrWithStatsCalculator.flow_field on the device.
// ---------------------------------------------------------------------------
namespace {

struct StartsArgs {
  const int* pos;       // [n, nd] grid positions, [z]yx
  int n, nd;
  int step[3], patch[3], post_patch[3], pre_shape[3], post_shape[3];
  const float* tf[2];   // targeting fields [nd, *tshape] (xy[z] components) or NULL
  int tshape[2][3];
  int tstep[2][3];
  int* pre_starts;      // [n, nd]
  int* post_starts;
  int* tg[2];           // [n, nd] offsets applied to the pre / post starts ([z]yx)
};

// np.round (half to even) of a double
__device__ __forceinline__ long long round_even(double v) {
  return static_cast<long long>(rint(v));
}

// Integer patch shift from a targeting field, kept inside the image
// (flow_field.py:626-649 / :652-677).  `starts` is [z]yx.
__device__ void target_offset(const StartsArgs& a, int side, const int* starts,
                              const int* psize, const int* img_shape, int* off) {
  int q[3];
  long long cell = 0;
  long long plane = 1;
  for (int i = 0; i < a.nd; ++i) plane *= a.tshape[side][i];
  for (int i = 0; i < a.nd; ++i) {
    const double c = static_cast<double>(starts[i] + psize[i] / 2) /
                     static_cast<double>(a.tstep[side][i]);
    long long v = round_even(c);
    v = v < 0 ? 0 : (v > a.tshape[side][i] - 1 ? a.tshape[side][i] - 1 : v);
    q[i] = static_cast<int>(v);
    cell = cell * a.tshape[side][i] + q[i];
  }
  for (int i = 0; i < a.nd; ++i) {
    // field component for image axis i: components are x, y[, z] = reversed axes
    float f = a.tf[side][(long long)(a.nd - 1 - i) * plane + cell];
    if (isnan(f)) f = 0.f;
    if (isinf(f)) f = f > 0.f ? 3.4028234663852886e38f : -3.4028234663852886e38f;
    // .astype(int): truncation; out-of-range values are INT64_MIN in NumPy --
    // fields hold pixel offsets, far inside the int range
    int o = static_cast<int>(f);
    const int ns = starts[i] + o;
    o = o - (ns < 0 ? ns : 0);
    const int hi = ns + psize[i];
    const int over = (hi > img_shape[i] ? hi : img_shape[i]) - img_shape[i];
    off[i] = o - over;
  }
}

__global__ void __launch_bounds__(kBlock) flow_starts_kernel(StartsArgs a) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= a.n) return;
  int post[3], pre[3], off[3];
  for (int i = 0; i < a.nd; ++i) {
    post[i] = a.pos[b * a.nd + i] * a.step[i];
    // NumPy floor division (flow_field.py:620): -1 // 2 == -1, not 0
    const int diff = a.patch[i] - a.post_patch[i];
    const int p = post[i] - (diff >= 0 ? diff / 2 : -((-diff + 1) / 2));
    pre[i] = p < 0 ? 0 : p;
  }
  if (a.tf[0]) {
    target_offset(a, 0, pre, a.patch, a.pre_shape, off);
    for (int i = 0; i < a.nd; ++i) {
      pre[i] += off[i];
      a.tg[0][b * a.nd + i] = off[i];
    }
  }
  if (a.tf[1]) {
    target_offset(a, 1, post, a.post_patch, a.post_shape, off);
    for (int i = 0; i < a.nd; ++i) {
      post[i] += off[i];
      a.tg[1][b * a.nd + i] = off[i];
    }
  }
  for (int i = 0; i < a.nd; ++i) {
    a.pre_starts[b * a.nd + i] = pre[i] < 0 ? 0 : pre[i];
    a.post_starts[b * a.nd + i] = post[i] < 0 ? 0 : post[i];
  }
}

struct ScatterArgs {
  const float* peaks;   // [n, nd + 2]
  const int* pos;       // [n, nd]
  const int* tg[2];     // or NULL
  float* out;           // [nd + 2, *grid], NaN filled by the caller
  int n, nd;
  int grid[3];
};

__global__ void __launch_bounds__(kBlock) flow_scatter_kernel(ScatterArgs a) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= a.n) return;
  long long cell = 0, cells = 1;
  for (int i = 0; i < a.nd; ++i) {
    cell = cell * a.grid[i] + a.pos[b * a.nd + i];
    cells *= a.grid[i];
  }
  for (int c = 0; c < a.nd + 2; ++c) {
    float v = a.peaks[b * (a.nd + 2) + c];
    if (c < a.nd) {  // vector component c <-> image axis nd - 1 - c
      if (a.tg[0]) v = v + static_cast<float>(a.tg[0][b * a.nd + a.nd - 1 - c]);
      if (a.tg[1]) v = v - static_cast<float>(a.tg[1][b * a.nd + a.nd - 1 - c]);
    }
    a.out[c * cells + cell] = v;
  }
}

}  // namespace

extern "C" int sfm_flow_starts(const SfmFlowStartsDesc* d) {
  if (!d || !d->positions || !d->pre_starts || !d->post_starts)
    return sfm::fail(SFM_ERR_INVALID, "flow_starts: NULL argument");
  if (d->ndim != 2 && d->ndim != 3) return sfm::fail(SFM_ERR_INVALID, "flow_starts: ndim");
  if (d->n < 0) return sfm::fail(SFM_ERR_INVALID, "flow_starts: n");
  if (d->n == 0) return SFM_OK;
  StartsArgs a;
  a.pos = d->positions;
  a.n = d->n;
  a.nd = d->ndim;
  const int o = 3 - d->ndim;  // descriptors pad [z]yx to 3 entries in front
  for (int i = 0; i < d->ndim; ++i) {
    a.step[i] = d->step[o + i];
    a.patch[i] = d->patch[o + i];
    a.post_patch[i] = d->post_patch[o + i];
    a.pre_shape[i] = d->pre_shape[o + i];
    a.post_shape[i] = d->post_shape[o + i];
    if (a.step[i] < 1) return sfm::fail(SFM_ERR_INVALID, "flow_starts: step");
  }
  const float* tf[2] = {d->pre_targeting_field, d->post_targeting_field};
  const int32_t* tsh[2] = {d->pre_targeting_shape, d->post_targeting_shape};
  const int32_t* tst[2] = {d->pre_targeting_step, d->post_targeting_step};
  int* tg[2] = {d->pre_offsets, d->post_offsets};
  for (int s2 = 0; s2 < 2; ++s2) {
    a.tf[s2] = tf[s2];
    a.tg[s2] = tg[s2];
    if (tf[s2] && !tg[s2])
      return sfm::fail(SFM_ERR_INVALID, "flow_starts: offsets buffer missing");
    for (int i = 0; i < d->ndim; ++i) {
      a.tshape[s2][i] = tsh[s2][o + i];
      a.tstep[s2][i] = tst[s2][o + i];
      if (tf[s2] && (a.tshape[s2][i] < 1 || a.tstep[s2][i] < 1))
        return sfm::fail(SFM_ERR_INVALID, "flow_starts: targeting shape / step");
    }
  }
  a.pre_starts = d->pre_starts;
  a.post_starts = d->post_starts;
  hipLaunchKernelGGL(flow_starts_kernel, dim3((d->n + kBlock - 1) / kBlock), dim3(kBlock),
                     0, static_cast<hipStream_t>(d->stream), a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

extern "C" int sfm_flow_scatter(const SfmFlowScatterDesc* d) {
  if (!d || !d->peaks || !d->positions || !d->out)
    return sfm::fail(SFM_ERR_INVALID, "flow_scatter: NULL argument");
  if (d->ndim != 2 && d->ndim != 3) return sfm::fail(SFM_ERR_INVALID, "flow_scatter: ndim");
  if (d->n <= 0) return d->n == 0 ? SFM_OK : sfm::fail(SFM_ERR_INVALID, "flow_scatter: n");
  ScatterArgs a;
  a.peaks = d->peaks;
  a.pos = d->positions;
  a.tg[0] = d->pre_offsets;
  a.tg[1] = d->post_offsets;
  a.out = d->out;
  a.n = d->n;
  a.nd = d->ndim;
  for (int i = 0; i < d->ndim; ++i) a.grid[i] = d->grid[3 - d->ndim + i];
  hipLaunchKernelGGL(flow_scatter_kernel, dim3((d->n + kBlock - 1) / kBlock), dim3(kBlock),
                     0, static_cast<hipStream_t>(d->stream), a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// The look-back rounds of EstimateMissingFlow (processor/flow.py:739-838):
// every round selects the nodes that are still missing, correlates them and
// accepts what passes the thresholds.  The two kernels below are the planning
// and the accept / update step of a round; the correlation lies between them.
// ---------------------------------------------------------------------------
namespace {

constexpr int kSelectBlock = 1024;
constexpr int kSelectWaves = kSelectBlock / 64;

struct SelectArgs {
  const unsigned char* sel;
  const int* counts[2];   // pre, post masked-pixel counts or NULL
  int pitch[2], area[2];
  double max_masked[2];
  int* pos;               // [capacity, 2]
  int* n_out;             // n, total
  int ny, nx, sel_pitch, batch;
};

// ONE workgroup walks the grid in chunks of 1024 linear indices, so the order
// of `pos` is the row-major order of np.where with nothing to wait for: the
// rank inside a wave comes from a ballot, the 16 wave totals are summed through
// LDS, the base is carried from chunk to chunk in a register.
__global__ void __launch_bounds__(kSelectBlock) flow_select_kernel(SelectArgs a) {
  __shared__ int wave_total[2][kSelectWaves];
  __shared__ int last[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nodes = a.ny * a.nx;
  int base = 0;
  for (int start = 0, it = 0; start < nodes; start += kSelectBlock, ++it) {
    const int i = start + tid;
    bool keep = false;
    int y = 0, x = 0;
    if (i < nodes) {
      y = i / a.nx;
      x = i - y * a.nx;
      keep = a.sel[(long long)y * a.sel_pitch + x] != 0;
      for (int s = 0; s < 2; ++s)
        if (keep && a.counts[s]) {
          const int c = a.counts[s][(long long)y * a.pitch[s] + x];
          // s / np.prod(patch) >= max_masked, in float64 (flow_field.py:579)
          keep = !(static_cast<double>(c) / static_cast<double>(a.area[s]) >= a.max_masked[s]);
        }
    }
    const unsigned long long votes = __ballot(keep);
    const int rank = __popcll(votes & ((1ull << lane) - 1ull));
    int* totals = wave_total[it & 1];   // two buffers: one barrier per chunk
    if (lane == 0) totals[wave] = __popcll(votes);
    __syncthreads();
    int before = 0, chunk = 0;
    for (int w = 0; w < kSelectWaves; ++w) {
      const int t = totals[w];
      before += w < wave ? t : 0;
      chunk += t;
    }
    if (keep) {
      const int row = base + before + rank;
      a.pos[2 * row] = y;
      a.pos[2 * row + 1] = x;
      if (before + rank == chunk - 1) {   // the last one so far: the padding row
        last[0] = y;
        last[1] = x;
      }
    }
    base += chunk;
  }
  __syncthreads();
  const int n = base;
  const int total = (n + a.batch - 1) / a.batch * a.batch;
  // every batch is padded by repeating the LAST position (flow_field.py:614-618)
  if (n > 0) {
    const int ly = last[0], lx = last[1];
    for (int row = n + tid; row < total; row += kSelectBlock) {
      a.pos[2 * row] = ly;
      a.pos[2 * row + 1] = lx;
    }
  }
  if (tid == 0) {
    a.n_out[0] = n;
    a.n_out[1] = total;
  }
}

struct MissingArgs {
  const float* field;     // [4, sy, sx]
  float* out[3];          // [ny, nx] each
  unsigned char* mask;
  int* attempts;
  unsigned long long* filled;
  double min_ratio, min_sharp, max_mag;
  int ny, nx, sy, sx, delta_z, max_attempts;
};

__global__ void __launch_bounds__(kBlock) missing_flow_update_kernel(MissingArgs a) {
  const int n = a.ny * a.nx;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  bool update = false;
  if (i < n) {
    const int y = i / a.nx, x = i - y * a.nx;
    bool m = a.mask[i] != 0;
    int att = a.attempts[i];
    if (y < a.sy && x < a.sx) {
      const int fn = a.sy * a.sx, j = y * a.sx + x;
      const float f0 = a.field[j], f1 = a.field[fn + j];
      const float sharp = fabsf(a.field[2 * fn + j]), ratio = fabsf(a.field[3 * fn + j]);
      const bool valid = isfinite(f0);
      if (valid) att += 1;                 // counted whether or not the node is in the mask
      // clean_flow with max_deviation = 0; comparisons with NaN are false, as in NumPy
      bool bad = static_cast<double>(sharp) < a.min_sharp;
      bad = bad || (ratio > 0.f && static_cast<double>(ratio) < a.min_ratio);
      // np.max over the components propagates NaN, and NaN > t is false
      if (a.max_mag > 0.0 && !isnan(f0) && !isnan(f1))
        bad = bad || static_cast<double>(fmaxf(fabsf(f0), fabsf(f1))) > a.max_mag;
      update = m && valid && !bad;
      if (update) {
        a.out[0][i] = f0;
        a.out[1][i] = f1;
        a.out[2][i] = static_cast<float>(a.delta_z);
        m = false;
      }
    }
    // the cap the next round applies before it selects (processor/flow.py:785)
    m = m && att <= a.max_attempts;
    a.mask[i] = m ? 1 : 0;
    a.attempts[i] = att;
  }
  const int cnt = __popcll(__ballot(update));
  if ((threadIdx.x & 63) == 0 && cnt)
    atomicAdd(a.filled, static_cast<unsigned long long>(cnt));
}

}  // namespace

extern "C" int sfm_flow_select(const SfmFlowSelectDesc* d) {
  if (!d || !d->selection || !d->positions || !d->counts)
    return sfm::fail(SFM_ERR_INVALID, "flow_select: NULL argument");
  const long long ny = d->grid[0], nx = d->grid[1];
  if (ny < 1 || nx < 1 || ny * nx > 0x7fffffffLL - kSelectBlock)
    return sfm::fail(SFM_ERR_INVALID, "flow_select: bad grid");
  if (d->batch_size < 1) return sfm::fail(SFM_ERR_INVALID, "flow_select: batch size");
  if (d->selection_pitch < nx) return sfm::fail(SFM_ERR_INVALID, "flow_select: selection pitch");
  const long long padded = (ny * nx + d->batch_size - 1) / d->batch_size * d->batch_size;
  if (padded > 0x3fffffffLL || d->capacity < padded)
    return sfm::fail(SFM_ERR_INVALID, "flow_select: capacity %d below %lld rows",
                     d->capacity, padded);
  SelectArgs a;
  a.sel = d->selection;
  a.sel_pitch = d->selection_pitch;
  const int32_t* counts[2] = {d->pre_counts, d->post_counts};
  const int32_t* cgrid[2] = {d->pre_grid, d->post_grid};
  const int32_t cpitch[2] = {d->pre_pitch, d->post_pitch};
  const int32_t carea[2] = {d->pre_area, d->post_area};
  const double cmax[2] = {d->pre_max_masked, d->post_max_masked};
  for (int s = 0; s < 2; ++s) {
    a.counts[s] = counts[s];
    a.pitch[s] = cpitch[s];
    a.area[s] = carea[s];
    a.max_masked[s] = cmax[s];
    if (!counts[s]) continue;
    if (cgrid[s][0] < ny || cgrid[s][1] < nx)
      return sfm::fail(SFM_ERR_INVALID, "flow_select: count plane [%d, %d] smaller than the grid",
                       cgrid[s][0], cgrid[s][1]);
    if (cpitch[s] < cgrid[s][1] || carea[s] < 1)
      return sfm::fail(SFM_ERR_INVALID, "flow_select: count pitch / patch area");
  }
  a.pos = d->positions;
  a.n_out = d->counts;
  a.ny = static_cast<int>(ny);
  a.nx = static_cast<int>(nx);
  a.batch = d->batch_size;
  hipLaunchKernelGGL(flow_select_kernel, dim3(1), dim3(kSelectBlock), 0,
                     static_cast<hipStream_t>(d->stream), a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

extern "C" int sfm_missing_flow_update(const SfmMissingFlowDesc* d) {
  if (!d || !d->field || !d->out[0] || !d->out[1] || !d->out[2] || !d->mask || !d->attempts ||
      !d->filled)
    return sfm::fail(SFM_ERR_INVALID, "missing_flow_update: NULL argument");
  const long long ny = d->shape[0], nx = d->shape[1];
  if (ny < 1 || nx < 1 || ny * nx > 0x7fffffffLL - kBlock)
    return sfm::fail(SFM_ERR_INVALID, "missing_flow_update: bad shape");
  if (d->field_shape[0] < 1 || d->field_shape[1] < 1 || d->field_shape[0] > ny ||
      d->field_shape[1] > nx)
    return sfm::fail(SFM_ERR_INVALID, "missing_flow_update: field [%d, %d] outside the section",
                     d->field_shape[0], d->field_shape[1]);
  MissingArgs a;
  a.field = d->field;
  for (int c = 0; c < 3; ++c) a.out[c] = d->out[c];
  a.mask = d->mask;
  a.attempts = d->attempts;
  a.filled = reinterpret_cast<unsigned long long*>(d->filled);
  a.min_ratio = d->min_peak_ratio;
  a.min_sharp = d->min_peak_sharpness;
  a.max_mag = d->max_magnitude;
  a.ny = static_cast<int>(ny);
  a.nx = static_cast<int>(nx);
  a.sy = d->field_shape[0];
  a.sx = d->field_shape[1];
  a.delta_z = d->delta_z;
  a.max_attempts = d->max_attempts;
  const unsigned grid = static_cast<unsigned>((ny * nx + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(missing_flow_update_kernel, dim3(grid), dim3(kBlock), 0,
                     static_cast<hipStream_t>(d->stream), a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

extern "C" int sfm_clean_flow(const SfmCleanFlowDesc* d, float* out) {
  if (!d || !d->flow || !out)
    return sfm::fail(SFM_ERR_INVALID, "clean_flow: NULL argument");
  if (d->dim != 2 && d->dim != 3)
    return sfm::fail(SFM_ERR_INVALID, "clean_flow: dim must be 2 or 3");
  if (d->channels < d->dim || d->channels > d->dim + 2)
    return sfm::fail(SFM_ERR_INVALID, "clean_flow: %d channels for dim %d",
                     d->channels, d->dim);
  for (int i = 0; i < 3; ++i)
    if (d->shape[i] < 1) return sfm::fail(SFM_ERR_INVALID, "clean_flow: bad shape");
  CleanArgs a;
  a.flow = d->flow;
  a.out = out;
  a.dim = d->dim;
  a.channels = d->channels;
  a.Z = d->shape[0];
  a.Y = d->shape[1];
  a.X = d->shape[2];
  a.min_ratio = d->min_peak_ratio;
  a.min_sharp = d->min_peak_sharpness;
  a.max_mag = d->max_magnitude;
  a.max_dev = d->max_deviation;
  const long long n = (long long)a.Z * a.Y * a.X;
  const long long grid = (n + kBlock - 1) / kBlock;
  if (grid > 0x7fffffffLL) return sfm::fail(SFM_ERR_INVALID, "clean_flow: too large");
  hipLaunchKernelGGL(clean_flow_kernel, dim3(static_cast<unsigned>(grid)), dim3(kBlock),
                     0, static_cast<hipStream_t>(d->stream), a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

// ---------------------------------------------------------------------------
// flow_utils.reconcile_flows (flow_utils.py:81-135):
//
//   1. merge + gradient: one thread per vector; the merged ch0 / ch1 of the
//      x / y neighbours the gradient needs are merged again by the reading
//      thread (K loads each), so nothing is exchanged between threads;
//   2. 3 x 3 median deviation (same window code as clean_flow, always 2-D);
//   3. small components, per z slice, 4-connected: union-find on int32 vector
//      indices (Playne & Hawick 2018).  Parents only ever point to smaller
//      indices (hooks and path halving are atomicMin), so find and union
//      terminate by construction; every parent access inside the union launch
//      is an agent-scope atomic (per-XCD L2s are not coherent).  Then one pass
//      compresses and counts component sizes at the roots and the invalid
//      vectors per slice, and one pass masks.
// Stage 2 reads a copy of stage 1's output (workspace); stage 3 works in place.
// ---------------------------------------------------------------------------
namespace {

struct ReconcileArgs {
  const float* flows;  // [K, C, Z, Y, X]
  const float* src;    // stage input [C, Z, Y, X]
  float* dst;          // stage output [C, Z, Y, X]
  int* parent;         // [N]; -1 = invalid vector
  int* size;           // [N]; component size at the root
  int* n0;             // [Z]; invalid vectors per slice
  int K, C, Z, Y, X;
  double max_grad, max_dev, min_dz;  // compared in double, see SfmReconcileDesc
  long long min_patch;
};

// Channel `ch` of the merged flow at vector i: the first flow is taken, and a
// later one replaces all channels wherever channel 0 is still NaN (and, for 3
// channels, |dz| >= min_delta_z; NaN >= t is false).
__device__ __forceinline__ float merged_at(const ReconcileArgs& a, long long n, long long i,
                                          int ch) {
  const long long fs = (long long)a.C * n;
  float v0 = a.flows[i];
  float v = a.flows[ch * n + i];
  for (int k = 1; k < a.K; ++k) {
    const float* f = a.flows + k * fs;
    if (isnan(v0) && (a.C != 3 || static_cast<double>(fabsf(f[2 * n + i])) >= a.min_dz)) {
      v0 = f[i];
      v = f[ch * n + i];
    }
  }
  return v;
}

__global__ void __launch_bounds__(kBlock) reconcile_merge_kernel(ReconcileArgs a) {
  const long long n = (long long)a.Z * a.Y * a.X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  float v[3];
  for (int c = 0; c < a.C; ++c) v[c] = merged_at(a, n, i, c);
  bool bad = false;
  if (a.max_grad > 0.0) {
    // a missing neighbour is 0 (gradient_bad)
    const int x = static_cast<int>(i % a.X);
    const int y = static_cast<int>((i / a.X) % a.Y);
    const float l = x > 0 ? merged_at(a, n, i - 1, 0) : 0.f;
    const float r = x + 1 < a.X ? merged_at(a, n, i + 1, 0) : 0.f;
    const float u = y > 0 ? merged_at(a, n, i - a.X, 1) : 0.f;
    const float d = y + 1 < a.Y ? merged_at(a, n, i + a.X, 1) : 0.f;
    bad = gradient_bad(v[0], v[1], l, r, u, d, a.max_grad);
  }
  for (int c = 0; c < a.C; ++c) a.dst[c * n + i] = bad ? NAN : v[c];
}

// Median of the 3 x 3 window of nan_to_num(comp) in one z slice (reflect).
__device__ float median9(const float* comp, const ReconcileArgs& a, int z, int y, int x) {
  const float* plane = comp + (long long)z * a.Y * a.X;
  return median3x3([&](int yy, int xx) { return plane[(long long)yy * a.X + xx]; }, y, x, a.Y,
                   a.X);
}

__global__ void __launch_bounds__(kBlock) reconcile_median_kernel(ReconcileArgs a) {
  const long long n = (long long)a.Z * a.Y * a.X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  const int x = static_cast<int>(i % a.X);
  const int y = static_cast<int>((i / a.X) % a.Y);
  const int z = static_cast<int>(i / ((long long)a.X * a.Y));
  const float d0 = fabsf(median9(a.src, a, z, y, x) - a.src[i]);
  const float d1 = fabsf(median9(a.src + n, a, z, y, x) - a.src[n + i]);
  const bool bad = deviation_bad(d0, d1, a.max_dev);
  for (int c = 0; c < a.C; ++c) a.dst[c * n + i] = bad ? NAN : a.src[c * n + i];
}

// the parent array lives in global memory, shared by all workgroups
constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;

__global__ void __launch_bounds__(kBlock) ccl_init_kernel(ReconcileArgs a) {
  const long long n = (long long)a.Z * a.Y * a.X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  bool valid = true;
  for (int c = 0; c < a.C; ++c) valid = valid && !isnan(a.dst[c * n + i]);
  a.parent[i] = valid ? static_cast<int>(i) : -1;
  a.size[i] = 0;
}

__global__ void __launch_bounds__(kBlock) ccl_union_kernel(ReconcileArgs a) {
  const int n = a.Z * a.Y * a.X;  // <= INT32_MAX (checked by the entry point)
  const long long il = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (il >= n) return;
  const int i = static_cast<int>(il);
  if (load_parent<kScope>(a.parent, i) < 0) return;
  const int x = i % a.X;
  const int y = (i / a.X) % a.Y;
  // right and down neighbours of the same slice: the cross structure
  if (x + 1 < a.X && load_parent<kScope>(a.parent, i + 1) >= 0)
    unite<kScope>(a.parent, i, i + 1);
  if (y + 1 < a.Y && load_parent<kScope>(a.parent, i + a.X) >= 0)
    unite<kScope>(a.parent, i, i + a.X);
}

// parent[i] <- root; component sizes at the roots; invalid vectors per slice.
__global__ void __launch_bounds__(kBlock) ccl_count_kernel(ReconcileArgs a) {
  __shared__ int bg[kBlock];  // invalid count per slice touched by this block
  const long long n = (long long)a.Z * a.Y * a.X;
  const long long plane = (long long)a.Y * a.X;
  const long long first = blockIdx.x * (long long)kBlock;
  const long long i = first + threadIdx.x;
  const long long z0 = first / plane;
  bg[threadIdx.x] = 0;
  __syncthreads();
  const bool in = i < n;
  int r = -1;
  if (in) {
    r = a.parent[i];
    if (r >= 0) {
      // the tree is final: plain loads, and a stale entry is still an ancestor
      int q = a.parent[r];
      while (q != r) {
        r = q;
        q = a.parent[r];
      }
      a.parent[i] = r;
    } else {
      atomicAdd(&bg[i / plane - z0], 1);
    }
  }
  // lanes of a wave mostly share a root: one add for those of the first lane
  const bool act = r >= 0;
  const unsigned long long actm = __ballot(act);
  if (actm) {
    const int leader = __ffsll(static_cast<long long>(actm)) - 1;
    const int r0 = __shfl(r, leader);
    const unsigned long long same = __ballot(act && r == r0);
    if (static_cast<int>(__lane_id()) == leader) atomicAdd(&a.size[r0], __popcll(same));
    if (act && r != r0) atomicAdd(&a.size[r], 1);
  }
  __syncthreads();
  const long long last = (first + kBlock < n ? first + kBlock : n) - 1;
  if (threadIdx.x <= last / plane - z0 && bg[threadIdx.x] > 0)
    atomicAdd(&a.n0[z0 + threadIdx.x], bg[threadIdx.x]);
}

// np.unique counts the background label too: when 0 < n0 < min_patch_size the
// invalid vectors of the slice become all-NaN as well.
__global__ void __launch_bounds__(kBlock) ccl_mask_kernel(ReconcileArgs a) {
  const long long n = (long long)a.Z * a.Y * a.X;
  const long long i = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (i >= n) return;
  const int r = a.parent[i];
  const long long cnt = r >= 0 ? a.size[r] : a.n0[i / ((long long)a.Y * a.X)];
  if (cnt < a.min_patch)
    for (int c = 0; c < a.C; ++c) a.dst[c * n + i] = NAN;
}

struct ReconcileLayout {
  size_t copy, parent, size, n0, bytes;
};

ReconcileLayout reconcile_layout(const SfmReconcileDesc* d) {
  const size_t n = (size_t)d->shape[0] * d->shape[1] * d->shape[2];
  auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
  ReconcileLayout w{};
  size_t off = 0;
  if (d->max_deviation > 0.0) {
    w.copy = off;
    off += up((size_t)d->channels * n * sizeof(float));
  }
  if (d->min_patch_size > 0) {
    w.parent = off;
    off += up(n * sizeof(int));
    w.size = off;
    off += up(n * sizeof(int));
    w.n0 = off;
    off += up((size_t)d->shape[0] * sizeof(int));
  }
  w.bytes = off > 256 ? off : 256;
  return w;
}

}  // namespace

extern "C" size_t sfm_reconcile_flows_workspace_bytes(const SfmReconcileDesc* d) {
  if (!d) return 0;
  for (int i = 0; i < 3; ++i)
    if (d->shape[i] < 1) return 0;
  return reconcile_layout(d).bytes;
}

extern "C" int sfm_reconcile_flows(const SfmReconcileDesc* d, float* out) {
  if (!d || !d->flows || !out)
    return sfm::fail(SFM_ERR_INVALID, "reconcile_flows: NULL argument");
  if (d->channels != 2 && d->channels != 3)
    return sfm::fail(SFM_ERR_INVALID, "reconcile_flows: %d channels, need 2 or 3",
                     d->channels);
  if (d->num_flows < 1)
    return sfm::fail(SFM_ERR_INVALID, "reconcile_flows: no flows");
  for (int i = 0; i < 3; ++i)
    if (d->shape[i] < 1) return sfm::fail(SFM_ERR_INVALID, "reconcile_flows: bad shape");
  const long long n = (long long)d->shape[0] * d->shape[1] * d->shape[2];
  if (n > 0x7fffffffLL)
    return sfm::fail(SFM_ERR_INVALID, "reconcile_flows: %lld vectors exceed int32 indices", n);
  const ReconcileLayout w = reconcile_layout(d);
  if (!d->workspace || d->workspace_bytes < w.bytes)
    return sfm::fail(SFM_ERR_WORKSPACE, "reconcile_flows workspace needs %zu bytes, got %zu",
                     w.bytes, d->workspace_bytes);
  char* ws = static_cast<char*>(d->workspace);
  ReconcileArgs a{};
  a.flows = d->flows;
  a.K = d->num_flows;
  a.C = d->channels;
  a.Z = d->shape[0];
  a.Y = d->shape[1];
  a.X = d->shape[2];
  a.max_grad = d->max_gradient;
  a.max_dev = d->max_deviation;
  a.min_dz = d->min_delta_z;
  a.min_patch = d->min_patch_size;
  const unsigned grid = static_cast<unsigned>((n + kBlock - 1) / kBlock);
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const bool median = a.max_dev > 0.0;
  float* copy = reinterpret_cast<float*>(ws + w.copy);
  a.dst = median ? copy : out;
  hipLaunchKernelGGL(reconcile_merge_kernel, dim3(grid), dim3(kBlock), 0, st, a);
  SFM_LAUNCH_CHECK();
  if (median) {
    a.src = copy;
    a.dst = out;
    hipLaunchKernelGGL(reconcile_median_kernel, dim3(grid), dim3(kBlock), 0, st, a);
    SFM_LAUNCH_CHECK();
  }
  if (a.min_patch > 0) {
    a.dst = out;
    a.parent = reinterpret_cast<int*>(ws + w.parent);
    a.size = reinterpret_cast<int*>(ws + w.size);
    a.n0 = reinterpret_cast<int*>(ws + w.n0);
    SFM_HIP_CHECK(hipMemsetAsync(a.n0, 0, (size_t)a.Z * sizeof(int), st));
    hipLaunchKernelGGL(ccl_init_kernel, dim3(grid), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(ccl_union_kernel, dim3(grid), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(ccl_count_kernel, dim3(grid), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(ccl_mask_kernel, dim3(grid), dim3(kBlock), 0, st, a);
    SFM_LAUNCH_CHECK();
  }
  return SFM_OK;
}
