// Map geometry helpers for gfx950: the one-pass functions that the reference's
// renderers call around invert_map and the warps.
//
//   shift_kernel        <-> map_utils.to_absolute / to_relative (map_utils.py:150-224)
//   outer_kernel,
//   inner_{x,y,z}_kernel,
//   fold_kernel         <-> map_utils.outer_box / inner_box (:307-389): the reductions
//                           over the absolute map, which is never stored
//   affine_kernel       <-> map_utils.make_affine_map (:789-811)
//   points_kernel       <-> warp.warp_points (warp.py:541-605)
//
// All of them are memory bound (a few flops per element).  The element-wise kernels
// and the outer reduction sweep a channel with 16-byte loads / stores per lane where
// the channel's address allows it, with a scalar head and tail; the inner reductions
// keep lanes along x and read 4 / 8 bytes per lane.  Built with -ffp-contract=off:
// every sum below is NumPy's, operation for operation.
#include "sfm_common.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxBlocks = 1024;   // per pass: SFM_MAP_EXTENTS_WORKSPACE_BYTES
constexpr int kSlot = 4;           // doubles per workgroup partial: a, b, flag, unused

// NumPy's in-place `map += offsets` for a float64 offset array: the element is
// widened, the sum taken in double and narrowed once to the map's type.
template <typename T>
__device__ __forceinline__ T shifted(T m, double off) {
  return static_cast<T>(static_cast<double>(m) + off);
}

template <typename T> struct Vec16;
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<double> { using type = double2; };

// Calls f(value, x, y, z) -> T for every element of one [z, y, x] channel, lanes
// along x, grid-stride.  Elements [head, head + V * nvec) are moved as 16-byte
// vectors (`head` elements bring the address to a 16-byte boundary; in and out must
// share it, else everything is scalar); the rest one by one.
template <typename T, bool LOAD, bool STORE, typename F>
__device__ __forceinline__ void sweep(const T* in, T* out, long long n, int ny, int nx, F f) {
  constexpr int V = 16 / sizeof(T);
  using VT = typename Vec16<T>::type;
  const uintptr_t ai = reinterpret_cast<uintptr_t>(LOAD ? in : out);
  long long head = static_cast<long long>(((16 - (ai & 15)) & 15) / sizeof(T));
  if (LOAD && STORE && ((reinterpret_cast<uintptr_t>(out) & 15) != (ai & 15))) head = n;
  if (head > n) head = n;
  const long long nvec = (n - head) / V;
  const long long tail0 = head + nvec * V;
  const long long items = nvec + head + (n - tail0);
  for (long long item = blockIdx.x * (long long)kBlock + threadIdx.x; item < items;
       item += (long long)gridDim.x * kBlock) {
    if (item < nvec) {
      const long long i = head + item * V;
      int x = static_cast<int>(i % nx);
      const long long r = i / nx;
      int y = static_cast<int>(r % ny);
      int z = static_cast<int>(r / ny);
      T v[V];
      if (LOAD) {
        const VT q = *reinterpret_cast<const VT*>(in + i);
        const T* qs = reinterpret_cast<const T*>(&q);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = qs[k];
      }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        v[k] = f(LOAD ? v[k] : T(0), x, y, z);
        if (++x == nx) {
          x = 0;
          if (++y == ny) {
            y = 0;
            ++z;
          }
        }
      }
      if (STORE) {
        VT q;
        T* qs = reinterpret_cast<T*>(&q);
#pragma unroll
        for (int k = 0; k < V; ++k) qs[k] = v[k];
        *reinterpret_cast<VT*>(out + i) = q;
      }
    } else {
      const long long j = item - nvec;
      const long long i = j < head ? j : tail0 + (j - head);
      const int x = static_cast<int>(i % nx);
      const long long r = i / nx;
      const T v = f(LOAD ? in[i] : T(0), x, static_cast<int>(r % ny), static_cast<int>(r / ny));
      if (STORE) out[i] = v;
    }
  }
}

struct GeomArgs {
  int ncomp, nz, ny, nx;
  long long n;            // nodes per channel
  double stride[3];       // z, y, x
  double start[3];        // z, y, x
  const void* in;
  void* out;
  double* partial;        // [3][kMaxBlocks][kSlot]
};

__device__ __forceinline__ int coord_of(int c, int x, int y, int z) {
  return c == 0 ? x : (c == 1 ? y : z);
}

template <typename T, bool SUB>
__global__ void __launch_bounds__(kBlock) shift_kernel(GeomArgs a) {
  const int c = blockIdx.y;
  const double st = a.stride[2 - c], s0 = a.start[2 - c];
  sweep<T, true, true>(static_cast<const T*>(a.in) + c * a.n, static_cast<T*>(a.out) + c * a.n,
                       a.n, a.ny, a.nx, [&](T m, int x, int y, int z) {
                         const double off = static_cast<double>(coord_of(c, x, y, z)) * st + s0;
                         return static_cast<T>(SUB ? static_cast<double>(m) - off
                                                   : static_cast<double>(m) + off);
                       });
}

struct AffineArgs {
  int nz, ny, nx;
  long long n;
  double stride[3], start[3];   // z, y, x
  double m[12];
  double* out;
};

__global__ void __launch_bounds__(kBlock) affine_kernel(AffineArgs a) {
  const int c = blockIdx.y;
  const double m0 = a.m[4 * c], m1 = a.m[4 * c + 1], m2 = a.m[4 * c + 2], t = a.m[4 * c + 3];
  sweep<double, false, true>(nullptr, a.out + c * a.n, a.n, a.ny, a.nx,
                             [&](double, int x, int y, int z) {
                               const double px = static_cast<double>(x) * a.stride[2] + a.start[2];
                               const double py = static_cast<double>(y) * a.stride[1] + a.start[1];
                               const double pz = static_cast<double>(z) * a.stride[0] + a.start[0];
                               const double pc = c == 0 ? px : (c == 1 ? py : pz);
                               return (((m0 * px + m1 * py) + m2 * pz) + t) - pc;
                             });
}

// ---- reductions ---------------------------------------------------------------
// Accumulators never hold a NaN: they start at +-inf and are updated by compares,
// which a NaN fails.  min / max are order independent, so every fold below gives
// the same bits whatever the launch shape.
__device__ __forceinline__ double pick(double a, double b, bool want_max) {
  return want_max ? (b > a ? b : a) : (b < a ? b : a);
}

// Folds (a, b) over the workgroup -- a by max when a_max, else min; b the other way
// -- ORs `flag`, and writes the workgroup's partial.
__device__ __forceinline__ void block_fold(double a, double b, bool a_max, int flag,
                                           double* __restrict__ dst) {
  __shared__ double s_a[kWaves], s_b[kWaves];
  const int any = __syncthreads_or(flag);
  for (int m = 32; m > 0; m >>= 1) {
    a = pick(a, __shfl_down(a, m, 64), a_max);
    b = pick(b, __shfl_down(b, m, 64), !a_max);
  }
  if ((threadIdx.x & 63) == 0) {
    s_a[threadIdx.x >> 6] = a;
    s_b[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w) {
      a = pick(a, s_a[w], a_max);
      b = pick(b, s_b[w], !a_max);
    }
    dst[0] = a;
    dst[1] = b;
    dst[2] = any ? 1.0 : 0.0;
    dst[3] = 0.0;
  }
}

// nanmin / nanmax of channel blockIdx.y of the absolute map.
template <typename T>
__global__ void __launch_bounds__(kBlock) outer_kernel(GeomArgs a) {
  const int c = blockIdx.y;
  const double st = a.stride[2 - c], s0 = a.start[2 - c];
  double mn = INFINITY, mx = -INFINITY;
  sweep<T, true, false>(static_cast<const T*>(a.in) + c * a.n, nullptr, a.n, a.ny, a.nx,
                        [&](T m, int x, int y, int z) {
                          const double v = static_cast<double>(
                              shifted(m, static_cast<double>(coord_of(c, x, y, z)) * st + s0));
                          if (v < mn) mn = v;
                          if (v > mx) mx = v;
                          return m;
                        });
  block_fold(mn, mx, false, 0, a.partial + ((long long)c * kMaxBlocks + blockIdx.x) * kSlot);
}

// Channel 0, lines along x.  A wave takes 64 / W rows at a time, W the power of two
// that covers a row (at most 64): segments of W lanes run along x and fold with
// xor shuffles that stay inside the segment.
template <typename T>
__global__ void __launch_bounds__(kBlock) inner_x_kernel(GeomArgs a, int w_seg) {
  const T* in = static_cast<const T*>(a.in);
  const double st = a.stride[2], s0 = a.start[2];
  const int lane = threadIdx.x & 63;
  const int seg = lane / w_seg, sx = lane % w_seg, per_wave = 64 / w_seg;
  const long long rows = (long long)a.nz * a.ny;
  const long long wave = blockIdx.x * (long long)kWaves + (threadIdx.x >> 6);
  double lo = -INFINITY, hi = INFINITY;   // max of row mins, min of row maxes
  int nan = 0;
  for (long long r0 = wave * per_wave; r0 < rows; r0 += (long long)gridDim.x * kWaves * per_wave) {
    const long long r = r0 + seg;
    double mn = INFINITY, mx = -INFINITY;
    if (r < rows) {
      const T* row = in + r * a.nx;
      for (int x = sx; x < a.nx; x += w_seg) {
        const T m = row[x];
        nan |= m != m;
        const double v = static_cast<double>(shifted(m, static_cast<double>(x) * st + s0));
        if (v < mn) mn = v;
        if (v > mx) mx = v;
      }
    }
    for (int m = w_seg >> 1; m > 0; m >>= 1) {
      mn = pick(mn, __shfl_xor(mn, m, 64), false);
      mx = pick(mx, __shfl_xor(mx, m, 64), true);
    }
    if (r < rows) {
      lo = pick(lo, mn, true);
      hi = pick(hi, mx, false);
    }
  }
  block_fold(lo, hi, true, nan, a.partial + (long long)blockIdx.x * kSlot);
}

// Channel 1, lines along y.  A workgroup takes one section's strip of 64 columns;
// its waves split the rows and fold per column through LDS.
template <typename T>
__global__ void __launch_bounds__(kBlock) inner_y_kernel(GeomArgs a) {
  __shared__ double s_mn[kWaves][64], s_mx[kWaves][64];
  const T* in = static_cast<const T*>(a.in) + a.n;
  const double st = a.stride[1], s0 = a.start[1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strips = (a.nx + 63) / 64;
  const long long units = (long long)a.nz * strips;
  double lo = -INFINITY, hi = INFINITY;
  int nan = 0;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const int z = static_cast<int>(u / strips);
    const int x = static_cast<int>(u % strips) * 64 + lane;
    double mn = INFINITY, mx = -INFINITY;
    if (x < a.nx) {
      const T* col = in + (long long)z * a.ny * a.nx + x;
#pragma unroll 4
      for (int y = wave; y < a.ny; y += kWaves) {
        const T m = col[(long long)y * a.nx];
        nan |= m != m;
        const double v = static_cast<double>(shifted(m, static_cast<double>(y) * st + s0));
        if (v < mn) mn = v;
        if (v > mx) mx = v;
      }
    }
    s_mn[wave][lane] = mn;
    s_mx[wave][lane] = mx;
    __syncthreads();
    if (wave == 0 && x < a.nx) {
      for (int w = 1; w < kWaves; ++w) {
        mn = pick(mn, s_mn[w][lane], false);
        mx = pick(mx, s_mx[w][lane], true);
      }
      lo = pick(lo, mn, true);
      hi = pick(hi, mx, false);
    }
    __syncthreads();
  }
  block_fold(lo, hi, true, nan, a.partial + ((long long)kMaxBlocks + blockIdx.x) * kSlot);
}

// Channel 2, lines along z: one thread per (y, x) site walks the sections.
template <typename T>
__global__ void __launch_bounds__(kBlock) inner_z_kernel(GeomArgs a) {
  const T* in = static_cast<const T*>(a.in) + 2 * a.n;
  const double st = a.stride[0], s0 = a.start[0];
  const long long plane = (long long)a.ny * a.nx;
  double lo = -INFINITY, hi = INFINITY;
  int nan = 0;
  for (long long s = blockIdx.x * (long long)kBlock + threadIdx.x; s < plane;
       s += (long long)gridDim.x * kBlock) {
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
    for (int z = 0; z < a.nz; ++z) {
      const T m = in[z * plane + s];
      nan |= m != m;
      const double v = static_cast<double>(shifted(m, static_cast<double>(z) * st + s0));
      if (v < mn) mn = v;
      if (v > mx) mx = v;
    }
    lo = pick(lo, mn, true);
    hi = pick(hi, mx, false);
  }
  block_fold(lo, hi, true, nan, a.partial + (2LL * kMaxBlocks + blockIdx.x) * kSlot);
}

struct FoldArgs {
  int passes, inner;
  int blocks[3];
  const double* partial;
  double* result;   // [8]
};

// One workgroup folds the per-workgroup partials of every pass.
__global__ void __launch_bounds__(kBlock) fold_kernel(FoldArgs f) {
  __shared__ double s_a[kBlock], s_b[kBlock];
  __shared__ int s_flag[kBlock];
  const bool a_max = f.inner != 0;
  int flag_all = 0;
  for (int p = 0; p < 3; ++p) {
    double a = a_max ? -INFINITY : INFINITY, b = a_max ? INFINITY : -INFINITY;
    int flag = 0;
    if (p < f.passes)
      for (int i = threadIdx.x; i < f.blocks[p]; i += kBlock) {
        const double* src = f.partial + ((long long)p * kMaxBlocks + i) * kSlot;
        a = pick(a, src[0], a_max);
        b = pick(b, src[1], !a_max);
        flag |= src[2] != 0.0;
      }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    s_flag[threadIdx.x] = flag;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
      if (static_cast<int>(threadIdx.x) < h) {
        s_a[threadIdx.x] = pick(s_a[threadIdx.x], s_a[threadIdx.x + h], a_max);
        s_b[threadIdx.x] = pick(s_b[threadIdx.x], s_b[threadIdx.x + h], !a_max);
        s_flag[threadIdx.x] |= s_flag[threadIdx.x + h];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      f.result[2 * p] = s_a[0];
      f.result[2 * p + 1] = s_b[0];
      flag_all |= s_flag[0];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    f.result[6] = flag_all ? 1.0 : 0.0;
    f.result[7] = 0.0;
  }
}

// ---- warp_points --------------------------------------------------------------
struct PointsArgs {
  int nz, ny, nx;
  long long n;
  double stride;
  double origin[2];          // x, y
  long long grid_start[2];   // x, y
  const void* map;
  const void* points;
  const int* section;
  void* out;
};

// Cell of q on the grid g(j) = (j + start) * stride, j in [0, nodes): the i in
// [0, nodes - 2] with g(i) <= q < g(i + 1), the edge cell outside the grid (and for
// q on the last node), as scipy's find_interval_ascending; t = (q - g(i)) / (g(i + 1)
// - g(i)) is not clipped.  The guess comes from a division and is corrected against
// the grid values themselves; NaN fails every compare and lands in cell 0.
__device__ __forceinline__ int find_cell(double q, int nodes, long long start, double stride,
                                         double* t) {
  auto g = [&](int j) { return static_cast<double>(j + start) * stride; };
  double guess = floor((q - g(0)) / stride);
  if (!(guess >= 0.0)) guess = 0.0;
  if (guess > static_cast<double>(nodes - 2)) guess = static_cast<double>(nodes - 2);
  int i = static_cast<int>(guess);
  while (i > 0 && q < g(i)) --i;
  while (i < nodes - 2 && q >= g(i + 1)) ++i;
  const double gi = g(i);
  *t = (q - gi) / (g(i + 1) - gi);
  return i;
}

template <typename TP> struct PointOut;
template <> struct PointOut<float> { static __device__ float of(float r) { return r; } };
template <> struct PointOut<double> { static __device__ double of(float r) { return r; } };
// np.round on float32 (half to even), then the cast
template <> struct PointOut<int32_t> {
  static __device__ int32_t of(float r) { return static_cast<int32_t>(rintf(r)); }
};
template <> struct PointOut<int64_t> {
  static __device__ int64_t of(float r) { return static_cast<int64_t>(rintf(r)); }
};

template <typename TM, typename TP>
__global__ void __launch_bounds__(kBlock) points_kernel(PointsArgs a) {
  const TM* map = static_cast<const TM*>(a.map);
  const TP* pts = static_cast<const TP*>(a.points);
  TP* out = static_cast<TP*>(a.out);
  const long long plane = (long long)a.ny * a.nx;
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < a.n;
       i += (long long)gridDim.x * kBlock) {
    const int z = a.section[i];
    float rx = NAN, ry = NAN;
    if (z >= 0 && z < a.nz) {
      double tx, ty;
      const int ix = find_cell(static_cast<double>(pts[3 * i]), a.nx, a.grid_start[0], a.stride, &tx);
      const int iy = find_cell(static_cast<double>(pts[3 * i + 1]), a.ny, a.grid_start[1], a.stride, &ty);
      const double wy[2] = {1.0 - ty, ty}, wx[2] = {1.0 - tx, tx};
      double acc[2] = {0.0, 0.0};
      for (int c = 0; c < 2; ++c) {
        const TM* sec = map + ((long long)c * a.nz + z) * plane;
        // corners in scipy's order: (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)
        for (int k = 0; k < 4; ++k) {
          const int y = iy + (k >> 1), x = ix + (k & 1);
          // to_absolute, then `+= origin`: two roundings to the map's type
          const TM node = shifted(shifted(sec[(long long)y * a.nx + x],
                                          static_cast<double>(c == 0 ? x : y) * a.stride),
                                  a.origin[c]);
          const double v = static_cast<double>(node);
          // float64 nodes: scipy's compiled 2-D path, (v * wy) * wx summed left to
          // right; float32 nodes: its generic path, v * ((1 * wy) * wx) added to 0
          const double term = sizeof(TM) == 8 ? (v * wy[k >> 1]) * wx[k & 1]
                                              : v * ((1.0 * wy[k >> 1]) * wx[k & 1]);
          acc[c] = (k == 0 && sizeof(TM) == 8) ? term : acc[c] + term;
        }
      }
      rx = static_cast<float>(acc[0]);
      ry = static_cast<float>(acc[1]);
    }
    out[3 * i] = PointOut<TP>::of(rx);
    out[3 * i + 1] = PointOut<TP>::of(ry);
  }
}

int grid_for(long long items, int cap) {
  long long g = (items + kBlock - 1) / kBlock;
  return static_cast<int>(g < 1 ? 1 : (g > cap ? cap : g));
}

bool bad_shape(const int32_t* s) {
  return s[0] < 1 || s[1] < 1 || s[2] < 1 ||
         (long long)s[0] * s[1] * s[2] > (1LL << 40);
}

template <typename D>
GeomArgs geom_args(const D* d, const void* in) {
  GeomArgs a;
  a.ncomp = d->ncomp;
  a.nz = d->shape[0];
  a.ny = d->shape[1];
  a.nx = d->shape[2];
  a.n = (long long)a.nz * a.ny * a.nx;
  for (int i = 0; i < 3; ++i) {
    a.stride[i] = d->stride[i];
    a.start[i] = d->start[i];
  }
  a.in = in;
  a.out = nullptr;
  a.partial = nullptr;
  return a;
}

template <typename TM>
int launch_points(const SfmWarpPointsDesc* d, const PointsArgs& a, hipStream_t st) {
  const dim3 grid(grid_for(d->n, 8192)), block(kBlock);
  switch (d->point_dtype) {
    case SFM_POINT_F32:
      hipLaunchKernelGGL((points_kernel<TM, float>), grid, block, 0, st, a);
      break;
    case SFM_POINT_F64:
      hipLaunchKernelGGL((points_kernel<TM, double>), grid, block, 0, st, a);
      break;
    case SFM_POINT_I32:
      hipLaunchKernelGGL((points_kernel<TM, int32_t>), grid, block, 0, st, a);
      break;
    case SFM_POINT_I64:
      hipLaunchKernelGGL((points_kernel<TM, int64_t>), grid, block, 0, st, a);
      break;
    default:
      return sfm::fail(SFM_ERR_INVALID, "warp points: unknown point dtype");
  }
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace

extern "C" {

int sfm_map_shift(const SfmMapShiftDesc* d) {
  if (!d || !d->coord_map || !d->out) return sfm::fail(SFM_ERR_INVALID, "map shift: NULL argument");
  if (d->ncomp != 2 && d->ncomp != 3)
    return sfm::fail(SFM_ERR_INVALID, "map shift: ncomp must be 2 or 3");
  if (bad_shape(d->shape)) return sfm::fail(SFM_ERR_INVALID, "map shift: bad shape");
  if (d->direction != SFM_SHIFT_TO_ABSOLUTE && d->direction != SFM_SHIFT_TO_RELATIVE)
    return sfm::fail(SFM_ERR_INVALID, "map shift: unknown direction");
  const size_t elem = d->f64 ? 8 : 4;
  if (reinterpret_cast<uintptr_t>(d->coord_map) % elem || reinterpret_cast<uintptr_t>(d->out) % elem)
    return sfm::fail(SFM_ERR_INVALID, "map shift: misaligned map");
  GeomArgs a = geom_args(d, d->coord_map);
  a.out = d->out;
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  const dim3 grid(grid_for((a.n + 16 / elem - 1) / (16 / elem) + 16, 4096), d->ncomp), block(kBlock);
  const bool sub = d->direction == SFM_SHIFT_TO_RELATIVE;
  if (d->f64) {
    if (sub) hipLaunchKernelGGL((shift_kernel<double, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((shift_kernel<double, false>), grid, block, 0, st, a);
  } else {
    if (sub) hipLaunchKernelGGL((shift_kernel<float, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((shift_kernel<float, false>), grid, block, 0, st, a);
  }
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int sfm_map_extents(const SfmMapExtentsDesc* d) {
  if (!d || !d->coord_map || !d->result)
    return sfm::fail(SFM_ERR_INVALID, "map extents: NULL argument");
  if (d->ncomp != 2 && d->ncomp != 3)
    return sfm::fail(SFM_ERR_INVALID, "map extents: ncomp must be 2 or 3");
  if (bad_shape(d->shape)) return sfm::fail(SFM_ERR_INVALID, "map extents: bad shape");
  if (d->mode != SFM_EXTENTS_OUTER && d->mode != SFM_EXTENTS_INNER)
    return sfm::fail(SFM_ERR_INVALID, "map extents: unknown mode");
  if (!d->workspace || d->workspace_bytes < SFM_MAP_EXTENTS_WORKSPACE_BYTES)
    return sfm::fail(SFM_ERR_WORKSPACE, "map extents: workspace of %d bytes needed",
                     SFM_MAP_EXTENTS_WORKSPACE_BYTES);
  const size_t elem = d->f64 ? 8 : 4;
  if (reinterpret_cast<uintptr_t>(d->coord_map) % elem ||
      reinterpret_cast<uintptr_t>(d->workspace) % 8 || reinterpret_cast<uintptr_t>(d->result) % 8)
    return sfm::fail(SFM_ERR_INVALID, "map extents: misaligned buffer");
  GeomArgs a = geom_args(d, d->coord_map);
  a.partial = static_cast<double*>(d->workspace);
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  FoldArgs f;
  f.passes = d->ncomp;
  f.inner = d->mode == SFM_EXTENTS_INNER;
  f.blocks[0] = f.blocks[1] = f.blocks[2] = 0;
  f.partial = a.partial;
  f.result = d->result;
  const dim3 block(kBlock);
  if (d->mode == SFM_EXTENTS_OUTER) {
    const int g = grid_for((a.n + 16 / elem - 1) / (16 / elem) + 16, kMaxBlocks);
    for (int c = 0; c < d->ncomp; ++c) f.blocks[c] = g;
    if (d->f64) hipLaunchKernelGGL(outer_kernel<double>, dim3(g, d->ncomp), block, 0, st, a);
    else hipLaunchKernelGGL(outer_kernel<float>, dim3(g, d->ncomp), block, 0, st, a);
    SFM_LAUNCH_CHECK();
  } else {
    int w_seg = 1;
    while (w_seg < 64 && w_seg < a.nx) w_seg <<= 1;
    const long long rows = (long long)a.nz * a.ny;
    const long long per_block = (long long)kWaves * (64 / w_seg);
    long long gx = (rows + per_block - 1) / per_block;
    f.blocks[0] = static_cast<int>(gx > kMaxBlocks ? kMaxBlocks : gx);
    const long long units = (long long)a.nz * ((a.nx + 63) / 64);
    f.blocks[1] = static_cast<int>(units > kMaxBlocks ? kMaxBlocks : units);
    f.blocks[2] = d->ncomp == 3 ? grid_for((long long)a.ny * a.nx, kMaxBlocks) : 0;
    if (d->f64) {
      hipLaunchKernelGGL(inner_x_kernel<double>, dim3(f.blocks[0]), block, 0, st, a, w_seg);
      hipLaunchKernelGGL(inner_y_kernel<double>, dim3(f.blocks[1]), block, 0, st, a);
      if (d->ncomp == 3)
        hipLaunchKernelGGL(inner_z_kernel<double>, dim3(f.blocks[2]), block, 0, st, a);
    } else {
      hipLaunchKernelGGL(inner_x_kernel<float>, dim3(f.blocks[0]), block, 0, st, a, w_seg);
      hipLaunchKernelGGL(inner_y_kernel<float>, dim3(f.blocks[1]), block, 0, st, a);
      if (d->ncomp == 3)
        hipLaunchKernelGGL(inner_z_kernel<float>, dim3(f.blocks[2]), block, 0, st, a);
    }
    SFM_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fold_kernel, dim3(1), block, 0, st, f);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int sfm_affine_map(const SfmAffineMapDesc* d) {
  if (!d || !d->out) return sfm::fail(SFM_ERR_INVALID, "affine map: NULL argument");
  if (bad_shape(d->shape)) return sfm::fail(SFM_ERR_INVALID, "affine map: bad shape");
  if (reinterpret_cast<uintptr_t>(d->out) % 8)
    return sfm::fail(SFM_ERR_INVALID, "affine map: misaligned output");
  AffineArgs a;
  a.nz = d->shape[0];
  a.ny = d->shape[1];
  a.nx = d->shape[2];
  a.n = (long long)a.nz * a.ny * a.nx;
  for (int i = 0; i < 3; ++i) {
    a.stride[i] = d->stride[i];
    a.start[i] = d->start[i];
  }
  for (int i = 0; i < 12; ++i) a.m[i] = d->matrix[i];
  a.out = d->out;
  hipLaunchKernelGGL(affine_kernel, dim3(grid_for(a.n / 2 + 16, 4096), 3), dim3(kBlock), 0,
                     static_cast<hipStream_t>(d->stream), a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

int sfm_warp_points(const SfmWarpPointsDesc* d) {
  if (!d) return sfm::fail(SFM_ERR_INVALID, "warp points: NULL argument");
  if (d->n < 0) return sfm::fail(SFM_ERR_INVALID, "warp points: negative point count");
  if (d->n == 0) return SFM_OK;
  if (!d->coord_map || !d->points || !d->section || !d->out)
    return sfm::fail(SFM_ERR_INVALID, "warp points: NULL argument");
  if (bad_shape(d->shape) || d->shape[1] < 2 || d->shape[2] < 2)
    return sfm::fail(SFM_ERR_INVALID, "warp points: the map needs at least 2 x 2 nodes");
  if (!(d->stride > 0.0) || !std::isfinite(d->stride))
    return sfm::fail(SFM_ERR_INVALID, "warp points: stride must be finite and positive");
  if (d->n > (1LL << 40)) return sfm::fail(SFM_ERR_INVALID, "warp points: too many points");
  PointsArgs a;
  a.nz = d->shape[0];
  a.ny = d->shape[1];
  a.nx = d->shape[2];
  a.n = d->n;
  a.stride = d->stride;
  for (int i = 0; i < 2; ++i) {
    a.origin[i] = d->origin[i];
    a.grid_start[i] = d->grid_start[i];
  }
  a.map = d->coord_map;
  a.points = d->points;
  a.section = d->section;
  a.out = d->out;
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  return d->f64 ? launch_points<double>(d, a, st) : launch_points<float>(d, a, st);
}

}  // extern "C"
