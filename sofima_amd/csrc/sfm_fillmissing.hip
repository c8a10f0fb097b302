// map_utils.fill_missing without its Delaunay branch (map_utils.py:227-304 with
// interpolate_first=False): every invalid node takes the bits of the nearest valid
// node, for gfx950.
//
// An exact Euclidean feature transform on the node lattice that carries the SOURCE
// node (its C-order index in [z, y, x]) instead of the distance:
//
//   fill_x_kernel       one wave per row: the nearest valid node of the row from the
//                       left (max scan) and from the right (min scan); the lower x of
//                       two equidistant ones.  Also the map's NaN flag and the "has a
//                       valid node" flag of every problem (z slice / volume).
//   fill_line_kernel    lines along y, then (3 channels) along z: every node takes the
//                       minimum over the line of (squared distance to the node that
//                       the line's entry carries, that node's index), compared as one
//                       64-bit integer -- so equidistant sources resolve to the lowest
//                       C-order index.  Brute force over the line from LDS.
//   fill_gather_kernel  copies the channels from the source nodes; all-invalid
//                       problems and NaN-free maps are decided here.
//
// Why the lowest index survives the separable passes: let m be the lowest-index node
// among the nearest of p.  No valid node of m's row lies closer in x to p's column
// than m (it would be nearer to p), and an equidistant one with lower x would be a
// nearest node of lower index: the x pass carries m at (m.z, m.y, p.x).  The same
// argument holds for the y pass at (m.z, p.y, p.x) and the z pass at p.
//
// Distances are exact uint32: with at most 16384 nodes per axis a squared distance is
// below 3 * 16383^2 < kNone, and kNone + (16384 + 96)^2 < 2^32, so "no source" needs
// no branch in the inner loop.  No floating-point arithmetic: channels move as bits.
#include "sfm_common.h"

#include <climits>
#include <cstdint>

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 64;   // line entries staged in LDS per step
constexpr int kRows = 8;     // outputs per thread of fill_line_kernel
constexpr int kMaxBlocks = 8192;
constexpr uint32_t kNone = 0xC0000000u;   // "squared distance" of an entry without source
constexpr unsigned long long kNoneKey = (static_cast<unsigned long long>(kNone) << 32) | 0xFFFFFFFFull;

static_assert(3LL * (SFM_FILL_MISSING_MAX_AXIS - 1) * (SFM_FILL_MISSING_MAX_AXIS - 1) < kNone,
              "a real squared distance must stay below kNone");
static_assert(kNone + static_cast<long long>(SFM_FILL_MISSING_MAX_AXIS + kChunk + kWaves * kRows) *
                          (SFM_FILL_MISSING_MAX_AXIS + kChunk + kWaves * kRows) < (1LL << 32),
              "kNone plus a squared line offset must not wrap");

template <typename U> struct Bits;
template <> struct Bits<uint32_t> {
  static constexpr uint32_t exp = 0x7f800000u, man = 0x007fffffu, qnan = 0x7fc00000u;
};
template <> struct Bits<uint64_t> {
  static constexpr uint64_t exp = 0x7ff0000000000000ull, man = 0x000fffffffffffffull,
                            qnan = 0x7ff8000000000000ull;
};

struct FillArgs {
  int ncomp, nz, ny, nx;
  int n;                  // nodes per channel, < 2^31
  int invalid_to_zero, extrapolate;
  const void* in;
  void* out;
  int* has_nan;           // [1]
  int* any_valid;         // [problems]
};

__device__ __forceinline__ void raise_flag(int* flag) {
  sfm::set_bit_once(reinterpret_cast<unsigned int*>(flag), 1u);
}

// Nearest valid node of every row along x.  src[node] = index of that node, or -1 for
// a row without valid node.  The left pass parks its result in src; the right pass is
// run by the same lanes on the same elements, so every lane reads back its own store.
template <typename U>
__global__ void __launch_bounds__(kBlock) fill_x_kernel(FillArgs a, int* __restrict__ src) {
  const U* in = static_cast<const U*>(a.in);
  const int lane = threadIdx.x & 63;
  const long long rows = static_cast<long long>(a.nz) * a.ny;
  int nan = 0;
  for (long long row = blockIdx.x * static_cast<long long>(kWaves) + (threadIdx.x >> 6); row < rows;
       row += static_cast<long long>(gridDim.x) * kWaves) {
    const int base = static_cast<int>(row * a.nx);
    int carry = -1;          // the last valid x at or before the chunk
    for (int x0 = 0; x0 < a.nx; x0 += 64) {
      const int x = x0 + lane;
      bool ok = x < a.nx;
      if (x < a.nx) {
        for (int c = 0; c < a.ncomp; ++c) {
          const U v = in[static_cast<long long>(c) * a.n + base + x];
          const bool special = (v & Bits<U>::exp) == Bits<U>::exp;   // inf or NaN
          ok = ok && !special;
          nan |= special && (v & Bits<U>::man) != 0;
        }
      }
      int v = ok ? x : -1;
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v = max(v, t);
      }
      v = max(v, carry);
      carry = __shfl(v, 63, 64);
      if (x < a.nx) src[base + x] = v;
    }
    if (lane == 0 && carry >= 0)
      raise_flag(a.any_valid + (a.ncomp == 2 ? static_cast<int>(row / a.ny) : 0));
    int rcarry = INT_MAX;    // the first valid x at or after the chunk
    for (int x0 = (a.nx - 1) / 64 * 64; x0 >= 0; x0 -= 64) {
      const int x = x0 + lane;
      const int left = x < a.nx ? src[base + x] : -1;
      int v = (x < a.nx && left == x) ? x : INT_MAX;
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_down(v, off, 64);
        if (lane + off < 64) v = min(v, t);
      }
      v = min(v, rcarry);
      rcarry = __shfl(v, 0, 64);
      int pick = -1;
      if (left >= 0 && (v == INT_MAX || x - left <= v - x)) pick = left;   // a tie: the lower x
      else if (v != INT_MAX) pick = v;
      if (x < a.nx) src[base + x] = pick < 0 ? -1 : base + pick;
    }
  }
  if (__any(nan) && lane == 0) raise_flag(a.has_nan);
}

// One pass along y (ALONG_Z false; blockIdx.z is z) or z (ALONG_Z true; blockIdx.z is
// y).  A workgroup takes 64 columns (lanes along x) and kWaves * kRows line positions,
// and walks the whole line in chunks of kChunk entries staged in LDS as 64-bit keys
// (squared distance from the entry to its source << 32 | source index).
template <bool ALONG_Z>
__global__ void __launch_bounds__(kBlock)
fill_line_kernel(FillArgs a, const int* __restrict__ src_in, int* __restrict__ src_out) {
  __shared__ unsigned long long s_key[kChunk][64];
  if (*a.has_nan == 0) return;   // nothing to fill: the gather copies the map
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane;
  const int o = blockIdx.z;
  const int len = ALONG_Z ? a.nz : a.ny;
  const int plane = a.ny * a.nx;
  const int step = ALONG_Z ? plane : a.nx;
  const int base = ALONG_Z ? o * a.nx : o * plane;
  const int t0 = blockIdx.y * (kWaves * kRows) + wave;
  unsigned long long best[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) best[r] = kNoneKey;
  for (int c0 = 0; c0 < len; c0 += kChunk) {
    for (int k = wave; k < kChunk; k += kWaves) {
      const int t = c0 + k;
      unsigned long long key = kNoneKey;
      if (t < len && x < a.nx) {
        const int s = src_in[base + t * step + x];
        if (s >= 0) {
          const int sz = ALONG_Z ? s / plane : o;   // the x and y passes stay in the slice
          const int rem = s - sz * plane;
          const int sy = rem / a.nx;
          const int dx = x - (rem - sy * a.nx);
          const int dy = (ALONG_Z ? o : t) - sy;
          const int dz = ALONG_Z ? t - sz : 0;
          key = (static_cast<unsigned long long>(static_cast<uint32_t>(dz * dz + dy * dy + dx * dx)) << 32) |
                static_cast<uint32_t>(s);
        }
      }
      s_key[k][lane] = key;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < kChunk; ++j) {
      const unsigned long long k0 = s_key[j][lane];
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int dt = t0 + kWaves * r - (c0 + j);
        const unsigned long long key =
            k0 + (static_cast<unsigned long long>(static_cast<uint32_t>(dt * dt)) << 32);
        best[r] = key < best[r] ? key : best[r];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int t = t0 + kWaves * r;
    if (t < len && x < a.nx)
      src_out[base + t * step + x] = static_cast<uint32_t>(best[r] >> 32) >= kNone
                                         ? -1 : static_cast<int>(static_cast<uint32_t>(best[r]));
  }
}

template <typename U>
__global__ void __launch_bounds__(kBlock) fill_gather_kernel(FillArgs a, const int* __restrict__ src) {
  const U* in = static_cast<const U*>(a.in);
  U* out = static_cast<U*>(a.out);
  const bool has_nan = *a.has_nan != 0;
  const long long total = static_cast<long long>(a.ncomp) * a.n;
  const int plane = a.ny * a.nx;
  for (long long i = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * kBlock) {
    const int c = static_cast<int>(i / a.n);
    const int p = static_cast<int>(i - static_cast<long long>(c) * a.n);
    U v = in[i];
    if (has_nan) {
      if (!a.any_valid[a.ncomp == 2 ? p / plane : 0]) {
        if (a.invalid_to_zero) v = 0;
        else if (a.extrapolate) v = Bits<U>::qnan;
      } else if (a.extrapolate) {
        const int s = src[p];
        if (s >= 0) v = in[static_cast<long long>(c) * a.n + s];
      }
    }
    out[i] = v;
  }
}

bool acceptable(const SfmFillMissingDesc* d) {
  if (!d || (d->ncomp != 2 && d->ncomp != 3)) return false;
  long long n = 1;
  for (int i = 0; i < 3; ++i) {
    if (d->shape[i] < 1 || d->shape[i] > SFM_FILL_MISSING_MAX_AXIS) return false;
    n *= d->shape[i];
  }
  return n <= INT_MAX;
}

struct Workspace {
  int* any_valid;
  int* src_a;
  int* src_b;
  size_t bytes;
};

Workspace carve(const SfmFillMissingDesc* d, void* base) {
  const size_t n = static_cast<size_t>(d->shape[0]) * d->shape[1] * d->shape[2];
  sfm::Carver c(base);
  Workspace w;
  w.any_valid = c.take<int>(d->ncomp == 2 ? d->shape[0] : 1);
  w.src_a = c.take<int>(n);
  w.src_b = c.take<int>(n);
  w.bytes = c.total();
  return w;
}

template <typename U>
int run(const SfmFillMissingDesc* d, const FillArgs& a, const Workspace& w, hipStream_t st) {
  const dim3 block(kBlock);
  const long long rows = static_cast<long long>(a.nz) * a.ny;
  const long long gx = (rows + kWaves - 1) / kWaves;
  hipLaunchKernelGGL(fill_x_kernel<U>, dim3(static_cast<unsigned>(gx > kMaxBlocks ? kMaxBlocks : gx)),
                     block, 0, st, a, w.src_a);
  SFM_LAUNCH_CHECK();
  const int* src = w.src_a;
  if (d->extrapolate) {
    const int per_block = kWaves * kRows;
    hipLaunchKernelGGL(fill_line_kernel<false>,
                       dim3((a.nx + 63) / 64, (a.ny + per_block - 1) / per_block, a.nz), block, 0, st,
                       a, w.src_a, w.src_b);
    SFM_LAUNCH_CHECK();
    src = w.src_b;
    if (a.ncomp == 3) {
      hipLaunchKernelGGL(fill_line_kernel<true>,
                         dim3((a.nx + 63) / 64, (a.nz + per_block - 1) / per_block, a.ny), block, 0,
                         st, a, w.src_b, w.src_a);
      SFM_LAUNCH_CHECK();
      src = w.src_a;
    }
  }
  const long long total = static_cast<long long>(a.ncomp) * a.n;
  const long long gg = (total + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(fill_gather_kernel<U>, dim3(static_cast<unsigned>(gg > kMaxBlocks ? kMaxBlocks : gg)),
                     block, 0, st, a, src);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace

extern "C" {

size_t sfm_fill_missing_nearest_workspace_bytes(const SfmFillMissingDesc* d) {
  return acceptable(d) ? carve(d, nullptr).bytes : 0;
}

int sfm_fill_missing_nearest(const SfmFillMissingDesc* d) {
  if (!d || !d->coord_map || !d->out || !d->has_nan)
    return sfm::fail(SFM_ERR_INVALID, "fill missing: NULL argument");
  if (d->ncomp != 2 && d->ncomp != 3)
    return sfm::fail(SFM_ERR_INVALID, "fill missing: ncomp must be 2 or 3");
  if (!acceptable(d))
    return sfm::fail(SFM_ERR_INVALID,
                     "fill missing: every axis holds 1 to %d nodes and a channel fewer than 2^31",
                     SFM_FILL_MISSING_MAX_AXIS);
  const Workspace w = carve(d, d->workspace);
  if (!d->workspace || d->workspace_bytes < w.bytes)
    return sfm::fail(SFM_ERR_WORKSPACE, "fill missing: workspace of %zu bytes needed", w.bytes);
  const size_t elem = d->f64 ? 8 : 4;
  const uintptr_t in = reinterpret_cast<uintptr_t>(d->coord_map);
  const uintptr_t out = reinterpret_cast<uintptr_t>(d->out);
  if (in % elem || out % elem || reinterpret_cast<uintptr_t>(d->has_nan) % 4 ||
      reinterpret_cast<uintptr_t>(d->workspace) % 8)
    return sfm::fail(SFM_ERR_INVALID, "fill missing: misaligned buffer");
  FillArgs a;
  a.ncomp = d->ncomp;
  a.nz = d->shape[0];
  a.ny = d->shape[1];
  a.nx = d->shape[2];
  a.n = a.nz * a.ny * a.nx;
  const size_t bytes = static_cast<size_t>(a.ncomp) * a.n * elem;
  if (in < out + bytes && out < in + bytes)
    return sfm::fail(SFM_ERR_INVALID, "fill missing: out overlaps coord_map");
  a.invalid_to_zero = d->invalid_to_zero != 0;
  a.extrapolate = d->extrapolate != 0;
  a.in = d->coord_map;
  a.out = d->out;
  a.has_nan = d->has_nan;
  a.any_valid = w.any_valid;
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  SFM_HIP_CHECK(hipMemsetAsync(d->has_nan, 0, sizeof(int), st));
  SFM_HIP_CHECK(hipMemsetAsync(w.any_valid, 0, sizeof(int) * (a.ncomp == 2 ? a.nz : 1), st));
  return d->f64 ? run<uint64_t>(d, a, w, st) : run<uint32_t>(d, a, w, st);
}

}  // extern "C"
