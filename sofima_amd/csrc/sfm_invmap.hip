// Inversion of in-plane coordinate maps on the device:
//
//   sfm_invert_map    <->  map_utils.invert_map, 2-D branch (map_utils.py:392-463)
//   sfm_resample_map  <->  map_utils.resample_map, linear (map_utils.py:490-546)
//   sfm_compose_maps_tri  <->  map_utils.compose_maps (map_utils.py:549-611)
//
// The reference triangulates the absolute positions of the valid nodes of a z
// slice with Qhull and interpolates the source lattice coordinates linearly
// over the Delaunay triangles (scipy LinearNDInterpolator).  Here the Delaunay
// triangulation is built from the lattice and then verified:
//
//   1. im_prep_kernel      absolute positions (to_absolute's float64 order),
//                          the per-slice exponent that fixes the predicate grid
//   2. im_quad_kernel      every quad with four valid corners (the lattice part
//                          R) is split by the in-circle test; a non-positive
//                          triangle is a fold and refuses the slice
//   3. im_complete_kernel  one workgroup per slice: the valid nodes that are not
//                          interior vertices of R (the set B, in LDS) are joined
//                          by gift wrapping from R's outline (or from a hull
//                          edge when R is empty) into the pocket, hole and hull
//                          triangles
//   4. im_verify_*         every edge of every triangle is locally Delaunay,
//                          has a twin or lies on the convex hull, the cover has
//                          degree one at a probe point and every valid node is
//                          a vertex.  By Lawson's theorem a set that passes is
//                          the Delaunay triangulation; a failure sets the
//                          slice's status and nothing of it is trusted
//   5. im_scatter_*        triangle-major scatter over the query lattice: the
//                          lowest triangle key wins a query (atomicMin), so
//                          shared edges and vertices are deterministic
//   6. im_gather_kernel    barycentric value in float64, made relative
//
// Predicates.  Positions are rounded to a per-slice power-of-two grid with
// |X| <= 2^50 (a step of 2^-37 px for coordinates below 8192), so orient2d is
// exact in 128-bit and incircle exact in 256-bit integers after a float64
// filter.  Exact ties of incircle (co-circular lattices: identity, translation)
// are broken by a symbolic perturbation of the lifting in node-index order, so
// every decision is consistent and the result is a Delaunay triangulation of
// the (rounded) points.
//
// Modes.  The engine triangulates points that carry values and interpolates
// them at a query lattice; what the points, the queries and the values are is
// a compile-time mode (Mode) of steps 1, 5 and 6 and of nothing else:
//
//   kInvert    points: the deformed positions of the nodes; queries: the dst
//              lattice trunc(u * stride); values: the source lattice
//              coordinates, made relative
//   kResample  points: the src lattice ((j + start) * src_stride) at the nodes
//              whose channel 0 is finite; queries: the dst lattice
//              ((u + start) * dst_stride); values: the two channels of the map
//              itself, stored in the map's type
//
//   kCompose   points: the lattice of map2 ((j + start) * stride2) at the nodes
//              where both channels of abs_map2 are finite; queries: the
//              absolute positions of map1's nodes, arbitrary points, so steps
//              5 and 6 are kernels of their own (cp_*): a query-major point
//              location in the lattice part R (the cell guessed from the
//              query and its eight neighbours, exact closed tests, lowest key
//              first), a triangle-major pass over the queries that R left
//              over, and a gather of abs_map2 that is made relative in map1's
//              type.  The winner of a query is the one the scatter would
//              pick: the lowest-keyed triangle whose closed exact test
//              contains it.
//
// In kResample and kCompose every full quad is an exact square: the in-circle
// test ties and the perturbation (lowest node id first: corner a of the quad) gives
// orient(b, c, d) > 0, so the diagonal is always b-d, from (i, j + 1) to
// (i + 1, j).  No quad can fold there.
#include "sfm_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace {

constexpr int kBlock = 256;
constexpr int kCompleteBlock = 1024;
// |B| cap: 20 bytes per node of B (two int64 coordinates, an int32 node id)
// in the 160 KB of LDS of one workgroup.
constexpr int kMaxB = 7936;
constexpr int kBBits = 13;  // kMaxB < 2^13: B-local ids in edge keys
constexpr int kNodeBits = 21;  // node ids in triangle keys: H * W <= 2^21
constexpr unsigned long long kEmptyKey = ~0ull;

enum : int {
  kStFold = 1,
  kStNotDelaunay = 2,
  kStBoundaryCap = 4,
  kStCapacity = 8,
  kStOverlap = 16,
  kStHull = 32,
  kStCover = 64,
  kStUnused = 128,
};

typedef long long ll;
typedef __int128 i128;
typedef unsigned __int128 u128;

struct SliceInfo {
  int exp;         // max binary exponent of |position| over the valid nodes
  int nvalid;
  int first_quad;  // lowest full quad (probe triangle), INT_MAX: R empty
  int nB;
  int ntri;        // triangles outside R
  int qcount;      // triangles that contain the probe point
};

enum Mode : int { kInvert = 0, kResample = 1, kCompose = 2 };

struct Args {
  const void* map;    // [2, Z, H, W]: double (kInvert), float or double (kResample)
  int Z, H, W, Hd, Wd;
  int sy0, sx0;       // kInvert: src start - dst start (y, x); kResample: src start
  double sy, sx;      // stride of the node lattice
  int qy0, qx0;       // kResample: dst start (y, x)
  double qs;          // kResample: stride of the query lattice
  int* status;
  double2* pos;       // [Z, H, W] absolute, NaN when invalid
  longlong2* qpos;    // [Z, H, W] on the predicate grid
  unsigned char* split;  // [Z, H-1, W-1]: 0 not full, 1 diagonal a-c, 2 b-d
  int* bid;           // [Z, H, W] index in B, -1
  unsigned char* used;  // [Z, H, W] vertex of a triangle outside R
  SliceInfo* info;    // [Z]
  int* blist;         // [Z, capB] node ids of B
  int4* tris;         // [Z, capT] node ids (x, y, z), w unused
  unsigned* ekeys;    // [Z, capE] directed edge (bu << 13 | bv) + 1, 0 empty
  int* evals;         // [Z, capE] owner triangle, -1 none, -2 R
  unsigned long long* tkeys;  // [Z, capTH] triangle hash, 0 empty
  unsigned* queue;    // [Z, capQ] edge keys
  unsigned long long* qkeys;  // [Z, Hd, Wd] winning triangle
  void* out;          // [2, Z, Hd, Wd], of the map's type
  int capB, capT, capQ;
  unsigned capE, capTH;
  // kCompose only
  const void* map1;     // [2, Zq, Hd, Wd]: the queries; Z is 1 or Zq
  int Zq;
  const double* scale2;  // [Zq] or NULL: factor of map2's relative values
  longlong2* cq;        // [Zq, Hd, Wd] queries on the predicate grid
  int* lcount;          // [Zq] queries that no triangle of R contains
  int* llist;           // [Zq, Hd * Wd] their indices in the slice
  int4* ibox;           // [Z] (-min j, max j, -min i, max i) of the valid nodes
};

// ---------------------------------------------------------------- predicates

__device__ __forceinline__ ll quant(double v, int g) { return llrint(ldexp(v, g)); }

// Sign of (b - a) x (c - a); inputs below 2^62 in magnitude.
__device__ __forceinline__ int orient(ll ax, ll ay, ll bx, ll by, ll cx, ll cy) {
  const i128 l = (i128)(bx - ax) * (cy - ay);
  const i128 r = (i128)(by - ay) * (cx - ax);
  return l > r ? 1 : (l < r ? -1 : 0);
}

struct S256 {
  unsigned long long w[4];
};

__device__ __forceinline__ S256 mul_signed(i128 a, i128 b) {
  const bool neg = (a < 0) != (b < 0);
  const u128 ua = a < 0 ? (u128)(-a) : (u128)a;
  const u128 ub = b < 0 ? (u128)(-b) : (u128)b;
  const unsigned long long a0 = (unsigned long long)ua, a1 = (unsigned long long)(ua >> 64);
  const unsigned long long b0 = (unsigned long long)ub, b1 = (unsigned long long)(ub >> 64);
  const u128 p00 = (u128)a0 * b0, p01 = (u128)a0 * b1, p10 = (u128)a1 * b0,
             p11 = (u128)a1 * b1;
  S256 r;
  r.w[0] = (unsigned long long)p00;
  const u128 mid = (p00 >> 64) + (unsigned long long)p01 + (unsigned long long)p10;
  r.w[1] = (unsigned long long)mid;
  const u128 hi = (mid >> 64) + (p01 >> 64) + (p10 >> 64) + (unsigned long long)p11;
  r.w[2] = (unsigned long long)hi;
  r.w[3] = (unsigned long long)(hi >> 64) + (unsigned long long)(p11 >> 64);
  if (neg) {
    unsigned long long c = 1;
    for (int i = 0; i < 4; ++i) {
      const unsigned long long v = ~r.w[i] + c;
      c = (c && v == 0) ? 1 : 0;
      r.w[i] = v;
    }
  }
  return r;
}

__device__ __forceinline__ S256 add256(const S256& a, const S256& b) {
  S256 r;
  unsigned long long c = 0;
  for (int i = 0; i < 4; ++i) {
    const unsigned long long s = a.w[i] + b.w[i];
    const unsigned long long c1 = s < a.w[i];
    const unsigned long long t = s + c;
    const unsigned long long c2 = t < s;
    r.w[i] = t;
    c = c1 | c2;
  }
  return r;
}

__device__ __forceinline__ int sign256(const S256& a) {
  if (a.w[3] >> 63) return -1;
  return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) ? 1 : 0;
}

// Sign of the in-circle determinant: > 0 when d lies inside the circle through
// a, b, c (a, b, c positively oriented).  Inputs below 2^51 in magnitude.
__device__ int incircle_exact(ll ax, ll ay, ll bx, ll by, ll cx, ll cy, ll dx, ll dy) {
  const ll adx = ax - dx, ady = ay - dy, bdx = bx - dx, bdy = by - dy, cdx = cx - dx,
           cdy = cy - dy;
  {  // float64 filter: differences are exact (below 2^52)
    const double fadx = (double)adx, fady = (double)ady, fbdx = (double)bdx,
                 fbdy = (double)bdy, fcdx = (double)cdx, fcdy = (double)cdy;
    const double bdxcdy = fbdx * fcdy, cdxbdy = fcdx * fbdy;
    const double cdxady = fcdx * fady, adxcdy = fadx * fcdy;
    const double adxbdy = fadx * fbdy, bdxady = fbdx * fady;
    const double alift = fadx * fadx + fady * fady;
    const double blift = fbdx * fbdx + fbdy * fbdy;
    const double clift = fcdx * fcdx + fcdy * fcdy;
    const double det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) +
                       clift * (adxbdy - bdxady);
    const double perm = (fabs(bdxcdy) + fabs(cdxbdy)) * alift +
                        (fabs(cdxady) + fabs(adxcdy)) * blift +
                        (fabs(adxbdy) + fabs(bdxady)) * clift;
    const double eps = 1.1102230246251565e-16;
    const double bound = (10.0 + 96.0 * eps) * eps * perm;
    if (det > bound) return 1;
    if (-det > bound) return -1;
  }
  const i128 alift = (i128)adx * adx + (i128)ady * ady;
  const i128 blift = (i128)bdx * bdx + (i128)bdy * bdy;
  const i128 clift = (i128)cdx * cdx + (i128)cdy * cdy;
  const i128 bc = (i128)bdx * cdy - (i128)cdx * bdy;
  const i128 ca = (i128)cdx * ady - (i128)adx * cdy;
  const i128 ab = (i128)adx * bdy - (i128)bdx * ady;
  return sign256(add256(add256(mul_signed(alift, bc), mul_signed(blift, ca)),
                        mul_signed(clift, ab)));
}

// incircle with exact ties broken by perturbing the lifting of the node with
// the lowest id first (ids distinct): the sign of d(det)/d(lift_p).
__device__ int incircle_sos(const ll* a, int ia, const ll* b, int ib, const ll* c, int ic,
                            const ll* d, int id) {
  const int s = incircle_exact(a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]);
  if (s != 0) return s;
  int m = ia;
  if (ib < m) m = ib;
  if (ic < m) m = ic;
  if (id < m) m = id;
  if (m == ia) return orient(b[0], b[1], c[0], c[1], d[0], d[1]);
  if (m == ib) return -orient(a[0], a[1], c[0], c[1], d[0], d[1]);
  if (m == ic) return orient(a[0], a[1], b[0], b[1], d[0], d[1]);
  return -orient(a[0], a[1], b[0], b[1], c[0], c[1]);
}

// ------------------------------------------------------------ lattice helpers

__device__ __forceinline__ int slice_g(const SliceInfo& s) { return 50 - s.exp; }

// Corner k (0 a, 1 b, 2 c, 3 d) of quad (i, j) as a node index.
__device__ __forceinline__ int corner(int W, int i, int j, int k) {
  return k == 0 ? i * W + j : k == 1 ? i * W + j + 1 : k == 2 ? (i + 1) * W + j + 1
                                                              : (i + 1) * W + j;
}

// Triangle `half` of a split quad as corners (positively oriented).
__device__ __forceinline__ void quad_tri(int s, int half, int* k) {
  if (s == 1) {
    if (half == 0) { k[0] = 0; k[1] = 1; k[2] = 2; } else { k[0] = 0; k[1] = 2; k[2] = 3; }
  } else {
    if (half == 0) { k[0] = 0; k[1] = 1; k[2] = 3; } else { k[0] = 1; k[1] = 2; k[2] = 3; }
  }
}

// The apex of the R triangle that has the directed edge u -> v, or -1.
__device__ int r_apex(const Args& a, const unsigned char* split, int u, int v) {
  const int W = a.W, H = a.H;
  const int ui = u / W, uj = u % W, vi = v / W, vj = v % W;
  const int di = vi - ui, dj = vj - uj;
  int qi, qj, k1, k2;  // quad, apex corner for split 1 / 2 (-1: not an edge)
  if (di == 0 && dj == 1) { qi = ui; qj = uj; k1 = 2; k2 = 3; }
  else if (di == 0 && dj == -1) { qi = ui - 1; qj = uj - 1; k1 = 0; k2 = 1; }
  else if (di == 1 && dj == 0) { qi = ui; qj = uj - 1; k1 = 0; k2 = 3; }
  else if (di == -1 && dj == 0) { qi = ui - 1; qj = uj; k1 = 2; k2 = 1; }
  else if (di == 1 && dj == 1) { qi = ui; qj = uj; k1 = 3; k2 = -1; }
  else if (di == -1 && dj == -1) { qi = ui - 1; qj = uj - 1; k1 = 1; k2 = -1; }
  else if (di == 1 && dj == -1) { qi = ui; qj = uj - 1; k1 = -1; k2 = 0; }
  else if (di == -1 && dj == 1) { qi = ui - 1; qj = uj; k1 = -1; k2 = 2; }
  else return -1;
  if (qi < 0 || qj < 0 || qi >= H - 1 || qj >= W - 1) return -1;
  const int s = split[qi * (W - 1) + qj];
  const int k = s == 1 ? k1 : s == 2 ? k2 : -1;
  return k < 0 ? -1 : corner(W, qi, qj, k);
}

__device__ __forceinline__ unsigned ekey(int bu, int bv) {
  return ((unsigned)bu << kBBits | (unsigned)bv) + 1u;
}

__device__ __forceinline__ unsigned ehash(unsigned key, unsigned cap) {
  return (key * 2654435761u) & (cap - 1);
}

// Inserts a directed edge; returns its slot (or -1 when the table is full) and
// whether this call inserted it.
__device__ int edge_insert(unsigned* keys, unsigned cap, unsigned key, bool* inserted) {
  unsigned h = ehash(key, cap);
  for (unsigned n = 0; n < cap; ++n, h = (h + 1) & (cap - 1)) {
    const unsigned old = atomicCAS(&keys[h], 0u, key);
    if (old == 0u) { *inserted = true; return (int)h; }
    if (old == key) { *inserted = false; return (int)h; }
  }
  *inserted = false;
  return -1;
}

__device__ int edge_find(const unsigned* keys, unsigned cap, unsigned key) {
  unsigned h = ehash(key, cap);
  for (unsigned n = 0; n < cap; ++n, h = (h + 1) & (cap - 1)) {
    const unsigned k = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
    if (k == key) return (int)h;
    if (k == 0u) return -1;
  }
  return -1;
}

// --------------------------------------------------------------------- kernels

__global__ void __launch_bounds__(kBlock) im_init_kernel(Args a) {
  const int z = blockIdx.x * kBlock + threadIdx.x;
  if (z >= a.Z) return;
  SliceInfo s;
  s.exp = -4096;
  s.nvalid = 0;
  s.first_quad = 0x7fffffff;
  s.nB = 0;
  s.ntri = 0;
  s.qcount = 0;
  a.info[z] = s;
}

// Wave reduction of per-slice values before one atomic: every thread of a
// slice would otherwise hit the same address.  Used when the whole wave maps to
// one slice (z < 0: lane out of range).
__device__ __forceinline__ bool wave_one_slice(int z) {
  const int z0 = __shfl(z, 0);
  return __all(z == z0 || z < 0) && z0 >= 0;
}

// Query (u, w) of the output lattice, one axis at a time.
template <int MODE>
__device__ __forceinline__ double query_x(const Args& a, int u) {
  if constexpr (MODE == kInvert) return trunc((double)u * a.sx);
  return (double)((long long)u + a.qx0) * a.qs;
}

template <int MODE>
__device__ __forceinline__ double query_y(const Args& a, int w) {
  if constexpr (MODE == kInvert) return trunc((double)w * a.sy);
  return (double)((long long)w + a.qy0) * a.qs;
}

template <int MODE, typename T>
__global__ void __launch_bounds__(kBlock) im_prep_kernel(Args a) {
  const long long hw = (long long)a.H * a.W;
  const long long n = (long long)a.Z * hw;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  const bool live = t < n;
  const int z = live ? (int)(t / hw) : -1;
  int emax = -4096, cnt = 0;
  if (live) {
    const int r = (int)(t % hw);
    const int i = r / a.W, j = r % a.W;
    const T* map = static_cast<const T*>(a.map);
    bool valid;
    double2 p;
    if constexpr (MODE == kInvert) {
      const double rx = map[t], ry = map[n + t];
      valid = isfinite(rx) && isfinite(ry);
      if (valid) {
        // to_absolute: rel + (j * sx + start_x * sx), same for y
        p.x = rx + ((double)j * a.sx + (double)a.sx0 * a.sx);
        p.y = ry + ((double)i * a.sy + (double)a.sy0 * a.sy);
      }
    } else {
      if constexpr (MODE == kResample) {
        // the reference looks at channel 0 only
        valid = isfinite(map[t]);
      } else {
        // both channels of abs_map2, rounded to the map's type
        const T ax = (T)((double)map[t] + ((double)j * a.sx + (double)a.sx0 * a.sx));
        const T ay = (T)((double)map[n + t] + ((double)i * a.sy + (double)a.sy0 * a.sy));
        valid = isfinite(ax) && isfinite(ay);
      }
      // the integer sum, then one product
      p.x = (double)((long long)j + a.sx0) * a.sx;
      p.y = (double)((long long)i + a.sy0) * a.sy;
    }
    if (valid && isfinite(p.x) && isfinite(p.y)) {
      int ex, ey;
      frexp(fabs(p.x), &ex);
      frexp(fabs(p.y), &ey);
      emax = ex > ey ? ex : ey;
      cnt = 1;
    } else {
      p.x = p.y = __builtin_nan("");
    }
    a.pos[t] = p;
    a.bid[t] = -1;
    if constexpr (MODE == kCompose) {
      if (cnt) {
        // the box only grows: a stale read costs an atomic, never a node
        int* b = &a.ibox[z].x;
        const int c[4] = {-j, j, -i, i};
        for (int m = 0; m < 4; ++m)
          if (__atomic_load_n(&b[m], __ATOMIC_RELAXED) < c[m]) atomicMax(&b[m], c[m]);
      }
    }
  }
  if (wave_one_slice(z)) {
    for (int off = 32; off > 0; off >>= 1) {
      const int e2 = __shfl_xor(emax, off);
      emax = e2 > emax ? e2 : emax;
      cnt += __shfl_xor(cnt, off);
    }
    if ((threadIdx.x & 63) == 0 && cnt > 0) {
      atomicMax(&a.info[z].exp, emax);
      atomicAdd(&a.info[z].nvalid, cnt);
    }
  } else if (cnt > 0) {
    atomicMax(&a.info[z].exp, emax);
    atomicAdd(&a.info[z].nvalid, cnt);
  }
}

__global__ void __launch_bounds__(kBlock) im_quant_kernel(Args a) {
  const long long hw = (long long)a.H * a.W;
  const long long n = (long long)a.Z * hw;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (t >= n) return;
  const int g = slice_g(a.info[t / hw]);
  const double2 p = a.pos[t];
  longlong2 q;
  q.x = isnan(p.x) ? 0 : quant(p.x, g);
  q.y = isnan(p.x) ? 0 : quant(p.y, g);
  a.qpos[t] = q;
}

// Splits quad t of slice z; returns its index in the slice when it is full.
__device__ int quad_split(const Args& a, long long t, int z) {
  const int qw = a.W - 1, qh = a.H - 1;
  const long long per = (long long)qh * qw;
  const int q = (int)(t % per);
  const int i = q / qw, j = q % qw;
  const long long base = (long long)z * a.H * a.W;
  int id[4];
  ll P[4][2];
  bool full = true;
  for (int k = 0; k < 4; ++k) {
    id[k] = corner(a.W, i, j, k);
    full = full && !isnan(a.pos[base + id[k]].x);
    const longlong2 v = a.qpos[base + id[k]];
    P[k][0] = v.x;
    P[k][1] = v.y;
  }
  unsigned char s = 0;
  if (full) {
    // d inside the circle through a, b, c: the Delaunay diagonal is b-d
    s = incircle_sos(P[0], id[0], P[1], id[1], P[2], id[2], P[3], id[3]) > 0 ? 2 : 1;
    for (int h = 0; h < 2; ++h) {
      int k[3];
      quad_tri(s, h, k);
      if (orient(P[k[0]][0], P[k[0]][1], P[k[1]][0], P[k[1]][1], P[k[2]][0], P[k[2]][1]) <= 0)
        atomicOr(&a.status[z], kStFold);
    }
  }
  a.split[t] = s;
  return s ? q : 0x7fffffff;
}

__global__ void __launch_bounds__(kBlock) im_quad_kernel(Args a) {
  const int qw = a.W - 1, qh = a.H - 1;
  const long long per = (long long)qh * qw;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  const bool live = t < (long long)a.Z * per;
  const int z = live ? (int)(t / per) : -1;
  int fq = 0x7fffffff;
  if (live) fq = quad_split(a, t, z);
  if (wave_one_slice(z)) {
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(fq, off);
      fq = o < fq ? o : fq;
    }
    if ((threadIdx.x & 63) == 0 && fq != 0x7fffffff) atomicMin(&a.info[z].first_quad, fq);
  } else if (fq != 0x7fffffff) {
    atomicMin(&a.info[z].first_quad, fq);
  }
}


// One workgroup per slice: B into LDS, then gift wrapping in rounds (one wave
// per front edge, the candidates of B across the lanes).
__global__ void __launch_bounds__(kCompleteBlock) im_complete_kernel(Args a) {
  __shared__ ll bx[kMaxB], by[kMaxB];
  __shared__ int bnode[kMaxB];
  __shared__ int s_nB, s_head, s_tail, s_ntri, s_err;
  const int z = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nwaves = kCompleteBlock / 64;
  const int H = a.H, W = a.W, hw = H * W;
  const long long base = (long long)z * hw;
  const unsigned char* split = a.split + (long long)z * (H - 1) * (W - 1);
  const SliceInfo info = a.info[z];
  if (info.nvalid < 3) return;
  unsigned* ekeys = a.ekeys + (long long)z * a.capE;
  int* evals = a.evals + (long long)z * a.capE;
  unsigned long long* tkeys = a.tkeys + (long long)z * a.capTH;
  unsigned* queue = a.queue + (long long)z * a.capQ;
  int4* tris = a.tris + (long long)z * a.capT;
  if (tid == 0) {
    s_nB = 0;
    s_head = 0;
    s_tail = 0;
    s_ntri = 0;
    s_err = 0;
  }
  __syncthreads();
  auto full = [&](int qi, int qj) {
    return qi >= 0 && qj >= 0 && qi < H - 1 && qj < W - 1 && split[qi * (W - 1) + qj] != 0;
  };
  // B: valid nodes that are not interior vertices of R
  for (int r = tid; r < hw; r += kCompleteBlock) {
    if (isnan(a.pos[base + r].x)) continue;
    const int i = r / W, j = r % W;
    if (full(i - 1, j - 1) && full(i - 1, j) && full(i, j - 1) && full(i, j)) continue;
    const int k = atomicAdd(&s_nB, 1);
    if (k < kMaxB) {
      const longlong2 q = a.qpos[base + r];
      bx[k] = q.x;
      by[k] = q.y;
      bnode[k] = r;
      a.bid[base + r] = k;
      a.blist[(long long)z * a.capB + k] = r;
    }
  }
  __syncthreads();
  const int nB = s_nB;
  if (nB > kMaxB || nB > a.capB) {
    if (tid == 0) {
      atomicOr(&a.status[z], kStBoundaryCap);
      a.info[z].nB = nB;
    }
    return;
  }
  auto push = [&](int bu, int bv) {
    bool ins;
    const int slot = edge_insert(ekeys, a.capE, ekey(bu, bv), &ins);
    if (slot < 0) { atomicOr(&s_err, kStCapacity); return; }
    if (!ins) return;
    const int k = atomicAdd(&s_tail, 1);
    if (k >= a.capQ) { atomicOr(&s_err, kStCapacity); return; }
    queue[k] = ekey(bu, bv);
  };
  auto mark_r = [&](int bu, int bv) {  // directed edge with R on its left
    bool ins;
    const int slot = edge_insert(ekeys, a.capE, ekey(bu, bv), &ins);
    if (slot < 0) { atomicOr(&s_err, kStCapacity); return; }
    evals[slot] = -2;
  };
  if (info.first_quad != 0x7fffffff) {
    // seeds: R's outline edges, directed with the outside on their left
    for (int k = tid; k < nB; k += kCompleteBlock) {
      const int r = bnode[k];
      const int i = r / W, j = r % W;
      if (j + 1 < W && !isnan(a.pos[base + r + 1].x)) {
        const bool up = full(i - 1, j), down = full(i, j);
        const int o = a.bid[base + r + 1];
        if (down && !up) { mark_r(k, o); push(o, k); }
        if (up && !down) { mark_r(o, k); push(k, o); }
      }
      if (i + 1 < H && !isnan(a.pos[base + r + W].x)) {
        const bool left = full(i, j - 1), right = full(i, j);
        const int o = a.bid[base + r + W];
        if (right && !left) { mark_r(o, k); push(k, o); }
        if (left && !right) { mark_r(k, o); push(o, k); }
      }
    }
  } else if (wave == 0) {
    // no lattice part: start from the hull edge at the lowest node
    int lo = -1;
    for (int k = lane; k < nB; k += 64)
      if (lo < 0 || by[k] < by[lo] || (by[k] == by[lo] && bx[k] < bx[lo])) lo = k;
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(lo, off);
      if (o >= 0 && (lo < 0 || by[o] < by[lo] || (by[o] == by[lo] && bx[o] < bx[lo]))) lo = o;
    }
    // the next hull node: no node strictly right of lo -> nx, the nearest on ties
    auto better = [&](int p, int c) {
      if (c < 0) return true;
      const int o = orient(bx[lo], by[lo], bx[c], by[c], bx[p], by[p]);
      if (o != 0) return o < 0;
      const i128 dp = (i128)(bx[p] - bx[lo]) * (bx[p] - bx[lo]) +
                      (i128)(by[p] - by[lo]) * (by[p] - by[lo]);
      const i128 dc = (i128)(bx[c] - bx[lo]) * (bx[c] - bx[lo]) +
                      (i128)(by[c] - by[lo]) * (by[c] - by[lo]);
      return dp < dc;
    };
    int nx = -1;
    for (int k = lane; k < nB; k += 64)
      if (k != lo && (bx[k] != bx[lo] || by[k] != by[lo]) && better(k, nx)) nx = k;
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(nx, off);
      if (o >= 0 && better(o, nx)) nx = o;
    }
    if (lane == 0 && nx >= 0) push(lo, nx);
  }
  __syncthreads();
  while (true) {
    // every wave reads the round's bounds before any wave pushes
    const int head = s_head, tail = s_tail, err = s_err;
    __syncthreads();
    if (head >= tail || err) break;
    for (int e = head + wave; e < tail; e += nwaves) {
      const unsigned key = queue[e] - 1u;
      const int ea = (int)(key >> kBBits), eb = (int)(key & ((1u << kBBits) - 1));
      const ll ax = bx[ea], ay = by[ea], bbx = bx[eb], bby = by[eb];
      const int ia = bnode[ea], ib = bnode[eb];
      const ll A[2] = {ax, ay}, B[2] = {bbx, bby};
      int best = -1;
      for (int k = lane; k < nB; k += 64) {
        if (k == ea || k == eb) continue;
        if (orient(ax, ay, bbx, bby, bx[k], by[k]) <= 0) continue;
        if (best >= 0) {
          const ll C[2] = {bx[best], by[best]}, P[2] = {bx[k], by[k]};
          if (incircle_sos(A, ia, B, ib, C, bnode[best], P, bnode[k]) <= 0) continue;
        }
        best = k;
      }
      for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(best, off);
        if (o < 0) continue;
        if (best >= 0) {
          const ll C[2] = {bx[best], by[best]}, P[2] = {bx[o], by[o]};
          if (incircle_sos(A, ia, B, ib, C, bnode[best], P, bnode[o]) <= 0) continue;
        }
        best = o;
      }
      if (lane != 0 || best < 0) continue;
      // triangle (ea, eb, best), positively oriented; canonical rotation
      int t3[3] = {ea, eb, best};
      int r0 = 0;
      if (t3[1] < t3[r0]) r0 = 1;
      if (t3[2] < t3[r0]) r0 = 2;
      const int c0 = t3[r0], c1 = t3[(r0 + 1) % 3], c2 = t3[(r0 + 2) % 3];
      const unsigned long long tk =
          ((unsigned long long)c0 << (2 * kBBits) | (unsigned long long)c1 << kBBits | c2) + 1;
      unsigned h = (unsigned)((tk * 0x9E3779B97F4A7C15ull) >> 32) & (a.capTH - 1);
      bool fresh = false, placed = false;
      for (unsigned n = 0; n < a.capTH; ++n, h = (h + 1) & (a.capTH - 1)) {
        const unsigned long long old = atomicCAS(&tkeys[h], 0ull, tk);
        if (old == 0ull) { fresh = true; placed = true; break; }
        if (old == tk) { placed = true; break; }
      }
      if (!placed) { atomicOr(&s_err, kStCapacity); continue; }
      if (!fresh) continue;
      const int t = atomicAdd(&s_ntri, 1);
      if (t >= a.capT) { atomicOr(&s_err, kStCapacity); continue; }
      // stored rotated to the lowest node id: the scatter keys are deterministic
      int n3[3] = {bnode[c0], bnode[c1], bnode[c2]};
      int n0 = 0;
      if (n3[1] < n3[n0]) n0 = 1;
      if (n3[2] < n3[n0]) n0 = 2;
      tris[t] = make_int4(n3[n0], n3[(n0 + 1) % 3], n3[(n0 + 2) % 3], 0);
      a.used[base + bnode[c0]] = 1;
      a.used[base + bnode[c1]] = 1;
      a.used[base + bnode[c2]] = 1;
      const int cs[3] = {c0, c1, c2};
      for (int m = 0; m < 3; ++m) {
        bool ins;
        const int slot = edge_insert(ekeys, a.capE, ekey(cs[m], cs[(m + 1) % 3]), &ins);
        if (slot < 0) { atomicOr(&s_err, kStCapacity); continue; }
        const int old = atomicCAS(&evals[slot], -1, t);
        if (old != -1 && old != t) atomicOr(&s_err, kStOverlap);
      }
      for (int m = 0; m < 3; ++m) push(cs[(m + 1) % 3], cs[m]);
    }
    __syncthreads();
    if (tid == 0) s_head = tail;
    __syncthreads();
  }
  if (tid == 0) {
    if (s_err) atomicOr(&a.status[z], s_err);
    a.info[z].nB = nB;
    a.info[z].ntri = s_ntri < a.capT ? s_ntri : a.capT;
  }
}

// The probe point of the cover test, scaled by 3 (the centroid of the first
// triangle: the first half of the lowest full quad, else triangle 0 outside R).
__device__ bool probe3(const Args& a, int z, ll* q3) {
  const SliceInfo s = a.info[z];
  const long long base = (long long)z * a.H * a.W;
  int v[3];
  if (s.first_quad != 0x7fffffff) {
    const int i = s.first_quad / (a.W - 1), j = s.first_quad % (a.W - 1);
    int k[3];
    quad_tri(a.split[(long long)z * (a.H - 1) * (a.W - 1) + s.first_quad], 0, k);
    for (int m = 0; m < 3; ++m) v[m] = corner(a.W, i, j, k[m]);
  } else if (s.ntri > 0) {
    const int4 t = a.tris[(long long)z * a.capT];
    v[0] = t.x;
    v[1] = t.y;
    v[2] = t.z;
  } else {
    return false;
  }
  q3[0] = q3[1] = 0;
  for (int m = 0; m < 3; ++m) {
    const longlong2 p = a.qpos[base + v[m]];
    q3[0] += p.x;
    q3[1] += p.y;
  }
  return true;
}

// Checks the triangle (v0, v1, v2) of slice z: positive orientation, every edge
// has a twin (R or outside) across which it is locally Delaunay or lies on the
// hull; counts whether it contains the probe point.  `outside`: a triangle of
// the completion (its edges must not belong to R).
__device__ void verify_triangle(const Args& a, int z, const int* v, bool outside) {
  const long long base = (long long)z * a.H * a.W;
  const unsigned char* split = a.split + (long long)z * (a.H - 1) * (a.W - 1);
  const unsigned* ekeys = a.ekeys + (long long)z * a.capE;
  const int* evals = a.evals + (long long)z * a.capE;
  ll P[3][2];
  for (int m = 0; m < 3; ++m) {
    const longlong2 p = a.qpos[base + v[m]];
    P[m][0] = p.x;
    P[m][1] = p.y;
  }
  int st = 0;
  if (orient(P[0][0], P[0][1], P[1][0], P[1][1], P[2][0], P[2][1]) <= 0) st |= kStFold;
  for (int m = 0; m < 3; ++m) {
    const int u = v[m], w = v[(m + 1) % 3], own = v[(m + 2) % 3];
    const int bu = a.bid[base + u], bw = a.bid[base + w];
    if (outside && r_apex(a, split, u, w) >= 0) st |= kStOverlap;
    if (!outside && bu >= 0 && bw >= 0) {
      const int slot = edge_find(ekeys, a.capE, ekey(bu, bw));
      if (slot >= 0 && evals[slot] >= 0) st |= kStOverlap;
    }
    // the neighbour across u -> w owns w -> u
    int nb = r_apex(a, split, w, u);
    if (bu >= 0 && bw >= 0) {
      const int slot = edge_find(ekeys, a.capE, ekey(bw, bu));
      const int t = slot >= 0 ? evals[slot] : -1;
      if (t >= 0) {
        if (nb >= 0) st |= kStOverlap;
        const int4 tr = a.tris[(long long)z * a.capT + t];
        nb = (tr.x != u && tr.x != w) ? tr.x : (tr.y != u && tr.y != w) ? tr.y : tr.z;
      }
    }
    if (nb >= 0) {
      const longlong2 p = a.qpos[base + nb];
      const ll N[2] = {p.x, p.y};
      if (incircle_sos(P[m], u, P[(m + 1) % 3], w, P[(m + 2) % 3], own, N, nb) > 0)
        st |= kStNotDelaunay;
    } else {
      // no twin: a hull edge, no node of B strictly on its right
      const SliceInfo s = a.info[z];
      const int* bl = a.blist + (long long)z * a.capB;
      for (int k = 0; k < s.nB; ++k) {
        const longlong2 p = a.qpos[base + bl[k]];
        if (orient(P[m][0], P[m][1], P[(m + 1) % 3][0], P[(m + 1) % 3][1], p.x, p.y) < 0) {
          st |= kStHull;
          break;
        }
      }
    }
  }
  ll q3[2];
  if (probe3(a, z, q3)) {
    bool in = true;
    for (int m = 0; m < 3 && in; ++m)
      in = orient(3 * P[m][0], 3 * P[m][1], 3 * P[(m + 1) % 3][0], 3 * P[(m + 1) % 3][1],
                  q3[0], q3[1]) >= 0;
    if (in) atomicAdd(&a.info[z].qcount, 1);
  }
  if (st) atomicOr(&a.status[z], st);
}

__global__ void __launch_bounds__(kBlock) im_verify_r_kernel(Args a) {
  const int qw = a.W - 1, qh = a.H - 1;
  const long long per = (long long)qh * qw;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (t >= (long long)a.Z * per) return;
  const int s = a.split[t];
  if (s == 0) return;
  const int z = (int)(t / per), q = (int)(t % per);
  if (a.info[z].nB > a.capB) return;
  const int i = q / qw, j = q % qw;
  for (int h = 0; h < 2; ++h) {
    int k[3], v[3];
    quad_tri(s, h, k);
    for (int m = 0; m < 3; ++m) v[m] = corner(a.W, i, j, k[m]);
    verify_triangle(a, z, v, false);
  }
}

__global__ void __launch_bounds__(kBlock) im_verify_o_kernel(Args a) {
  const int z = blockIdx.y;
  const int n = a.info[z].ntri;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    const int4 tr = a.tris[(long long)z * a.capT + t];
    const int v[3] = {tr.x, tr.y, tr.z};
    verify_triangle(a, z, v, true);
  }
}

// Every valid node is a vertex; the probe point is covered exactly once.
__global__ void __launch_bounds__(kBlock) im_verify_nodes_kernel(Args a) {
  const long long hw = (long long)a.H * a.W;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (t >= (long long)a.Z * hw) return;
  const int z = (int)(t / hw), r = (int)(t % hw);
  const SliceInfo s = a.info[z];
  const bool any = s.first_quad != 0x7fffffff || s.ntri > 0;
  if (!any || s.nB > a.capB) return;
  if (r == 0 && s.qcount != 1) atomicOr(&a.status[z], kStCover);
  if (isnan(a.pos[t].x) || a.used[t]) return;
  const int i = r / a.W, j = r % a.W, H = a.H, W = a.W;
  const unsigned char* split = a.split + (long long)z * (H - 1) * (W - 1);
  bool in_r = false;
  for (int di = -1; di <= 0; ++di)
    for (int dj = -1; dj <= 0; ++dj) {
      const int qi = i + di, qj = j + dj;
      if (qi >= 0 && qj >= 0 && qi < H - 1 && qj < W - 1 && split[qi * (W - 1) + qj])
        in_r = true;
    }
  if (!in_r) atomicOr(&a.status[z], kStUnused);
}

// Query lattice range [lo, hi] that can hold a triangle spanning [mn, mx]:
// queries at trunc(u * s) (kInvert) or (u + q0) * s (kResample).
template <int MODE>
__device__ __forceinline__ void query_range(double mn, double mx, double s, int q0, int n,
                                            int* lo, int* hi) {
  const double margin = MODE == kInvert ? 1.0 + ceil(1.0 / s) : 2.0;
  double l = floor(mn / s) - margin, h = ceil(mx / s) + margin;
  if constexpr (MODE == kResample) {
    l -= (double)q0;
    h -= (double)q0;
  }
  // clamp both ends before the conversion (an empty range stays empty)
  l = l < 0 ? 0 : (l > n ? n : l);
  h = h > n - 1 ? n - 1 : (h < -1 ? -1 : h);
  *lo = (int)l;
  *hi = (int)h;
}

// Scatters triangle v (keyed `key`) over the query lattice of slice z; lanes
// [lane0, lane0 + nlanes) share the work.
template <int MODE>
__device__ void scatter(const Args& a, int z, const int* v, unsigned long long key, int lane0,
                        int nlanes) {
  const long long base = (long long)z * a.H * a.W;
  const int g = slice_g(a.info[z]);
  ll P[3][2];
  double mnx = 1e308, mxx = -1e308, mny = 1e308, mxy = -1e308;
  for (int m = 0; m < 3; ++m) {
    const longlong2 q = a.qpos[base + v[m]];
    P[m][0] = q.x;
    P[m][1] = q.y;
    const double2 p = a.pos[base + v[m]];
    mnx = fmin(mnx, p.x);
    mxx = fmax(mxx, p.x);
    mny = fmin(mny, p.y);
    mxy = fmax(mxy, p.y);
  }
  int u0, u1, w0, w1;
  if constexpr (MODE == kInvert) {
    query_range<MODE>(mnx, mxx, a.sx, 0, a.Wd, &u0, &u1);
    query_range<MODE>(mny, mxy, a.sy, 0, a.Hd, &w0, &w1);
  } else {
    query_range<MODE>(mnx, mxx, a.qs, a.qx0, a.Wd, &u0, &u1);
    query_range<MODE>(mny, mxy, a.qs, a.qy0, a.Hd, &w0, &w1);
  }
  if (u0 > u1 || w0 > w1) return;
  const int nu = u1 - u0 + 1;
  const long long cnt = (long long)nu * (w1 - w0 + 1);
  unsigned long long* keys = a.qkeys + (long long)z * a.Hd * a.Wd;
  const double lim = 2305843009213693952.0;  // 2^61
  for (long long c = lane0; c < cnt; c += nlanes) {
    const int u = u0 + (int)(c % nu), w = w0 + (int)(c / nu);
    const double qx = ldexp(query_x<MODE>(a, u), g), qy = ldexp(query_y<MODE>(a, w), g);
    if (!(fabs(qx) < lim && fabs(qy) < lim)) continue;
    const ll X = llrint(qx), Y = llrint(qy);
    bool in = true;
    for (int m = 0; m < 3 && in; ++m)
      in = orient(P[m][0], P[m][1], P[(m + 1) % 3][0], P[(m + 1) % 3][1], X, Y) >= 0;
    if (in) atomicMin(&keys[(long long)w * a.Wd + u], key);
  }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) im_scatter_r_kernel(Args a) {
  const int qw = a.W - 1, qh = a.H - 1;
  const long long per = (long long)qh * qw;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (t >= (long long)a.Z * per) return;
  const int s = a.split[t];
  if (s == 0) return;
  const int z = (int)(t / per), q = (int)(t % per);
  const int i = q / qw, j = q % qw;
  for (int h = 0; h < 2; ++h) {
    int k[3], v[3];
    quad_tri(s, h, k);
    for (int m = 0; m < 3; ++m) v[m] = corner(a.W, i, j, k[m]);
    scatter<MODE>(a, z, v, (unsigned long long)q << 1 | h, 0, 1);
  }
}

// One wave per triangle outside R (its bounding box can span the lattice).
template <int MODE>
__global__ void __launch_bounds__(kBlock) im_scatter_o_kernel(Args a) {
  const int z = blockIdx.y;
  const int n = a.info[z].ntri;
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (kBlock / 64);
  for (int t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < n; t += nw) {
    const int4 tr = a.tris[(long long)z * a.capT + t];
    const int v[3] = {tr.x, tr.y, tr.z};
    const unsigned long long key = 1ull << 63 | (unsigned long long)tr.x << (2 * kNodeBits) |
                                   (unsigned long long)tr.y << kNodeBits |
                                   (unsigned long long)tr.z;
    scatter<MODE>(a, z, v, key, lane, 64);
  }
}

template <int MODE, typename T>
__global__ void __launch_bounds__(kBlock) im_gather_kernel(Args a) {
  const long long per = (long long)a.Hd * a.Wd;
  const long long n = (long long)a.Z * per;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (t >= n) return;
  const int z = (int)(t / per), r = (int)(t % per);
  const int w = r / a.Wd, u = r % a.Wd;
  const unsigned long long key = a.qkeys[t];
  double ox = __builtin_nan(""), oy = __builtin_nan("");
  if (key != kEmptyKey) {
    int v[3];
    if (key >> 63) {
      const unsigned long long m = (1ull << kNodeBits) - 1;
      v[0] = (int)(key >> (2 * kNodeBits) & m);
      v[1] = (int)(key >> kNodeBits & m);
      v[2] = (int)(key & m);
    } else {
      const int q = (int)(key >> 1), h = (int)(key & 1);
      const int i = q / (a.W - 1), j = q % (a.W - 1);
      int k[3];
      quad_tri(a.split[(long long)z * (a.H - 1) * (a.W - 1) + q], h, k);
      for (int m = 0; m < 3; ++m) v[m] = corner(a.W, i, j, k[m]);
    }
    const long long base = (long long)z * a.H * a.W;
    double2 p[3];
    double vx[3], vy[3];
    for (int m = 0; m < 3; ++m) {
      p[m] = a.pos[base + v[m]];
      if constexpr (MODE == kInvert) {
        const int i = v[m] / a.W, j = v[m] % a.W;
        // the reference's source coordinates live in an integer array
        vx[m] = trunc((double)(j + a.sx0) * a.sx);
        vy[m] = trunc((double)(i + a.sy0) * a.sy);
      } else {
        // the map's own channels; a NaN in channel 1 propagates
        const T* map = static_cast<const T*>(a.map);
        vx[m] = (double)map[base + v[m]];
        vy[m] = (double)map[(long long)a.Z * a.H * a.W + base + v[m]];
      }
    }
    const double qx = query_x<MODE>(a, u), qy = query_y<MODE>(a, w);
    const double e1x = p[1].x - p[0].x, e1y = p[1].y - p[0].y;
    const double e2x = p[2].x - p[0].x, e2y = p[2].y - p[0].y;
    const double dx = qx - p[0].x, dy = qy - p[0].y;
    const double det = e1x * e2y - e1y * e2x;
    const double l1 = (dx * e2y - dy * e2x) / det;
    const double l2 = (e1x * dy - e1y * dx) / det;
    const double l0 = 1.0 - l1 - l2;
    ox = l0 * vx[0] + l1 * vx[1] + l2 * vx[2];
    oy = l0 * vy[0] + l1 * vy[1] + l2 * vy[2];
    if constexpr (MODE == kInvert) {
      // to_relative
      ox = ox - (double)u * a.sx;
      oy = oy - (double)w * a.sy;
    }
  }
  T* out = static_cast<T*>(a.out);
  out[(long long)z * per + r] = (T)ox;
  out[n + (long long)z * per + r] = (T)oy;
}

// ------------------------------------------------ kCompose: arbitrary queries

// The slice of map2 that answers slice z of map1 (one slice serves them all).
__device__ __forceinline__ int compose_z2(const Args& a, int z) { return a.Z == 1 ? 0 : z; }

// Node (w, u) of map1 (element t of a channel) in absolute format, rounded to
// map1's type as to_absolute stores it; false when a channel is not finite.
template <typename T1>
__device__ __forceinline__ bool compose_query(const Args& a, long long t, int w, int u,
                                              double* qx, double* qy) {
  const T1* m1 = static_cast<const T1*>(a.map1);
  const long long n1 = (long long)a.Zq * a.Hd * a.Wd;
  const T1 ax = (T1)((double)m1[t] + ((double)u * a.qs + (double)a.qx0 * a.qs));
  const T1 ay = (T1)((double)m1[n1 + t] + ((double)w * a.qs + (double)a.qy0 * a.qs));
  *qx = (double)ax;
  *qy = (double)ay;
  return isfinite(ax) && isfinite(ay);
}

__device__ __forceinline__ void tri_points(const Args& a, long long base, const int* v,
                                           ll P[3][2]) {
  for (int m = 0; m < 3; ++m) {
    const longlong2 q = a.qpos[base + v[m]];
    P[m][0] = q.x;
    P[m][1] = q.y;
  }
}

__device__ __forceinline__ bool tri_contains(const ll P[3][2], ll X, ll Y) {
  bool in = true;
  for (int m = 0; m < 3 && in; ++m)
    in = orient(P[m][0], P[m][1], P[(m + 1) % 3][0], P[(m + 1) % 3][1], X, Y) >= 0;
  return in;
}

// One thread per node of map1: the query on the predicate grid, then the
// triangles of R in the guessed cell of map2 and its eight neighbours in key
// order (the guess may be off by one, and a query on a lattice vertex lies in
// four cells: the exact tests decide).  A query that R does not contain and
// that lies in the bounding box of the valid nodes goes on the slice's
// leftover list for cp_scatter_o_kernel.
template <typename T1>
__global__ void __launch_bounds__(kBlock) cp_locate_kernel(Args a) {
  const long long per = (long long)a.Hd * a.Wd;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (t >= (long long)a.Zq * per) return;
  const int z = (int)(t / per), r = (int)(t % per);
  const int w = r / a.Wd, u = r % a.Wd;
  const int z2 = compose_z2(a, z);
  const SliceInfo s = a.info[z2];
  double qx, qy;
  if (s.nvalid < 3 || !compose_query<T1>(a, t, w, u, &qx, &qy)) return;
  const int g = slice_g(s);
  const double lim = 2305843009213693952.0;  // 2^61
  const double fx = ldexp(qx, g), fy = ldexp(qy, g);
  if (!(fabs(fx) < lim && fabs(fy) < lim)) return;
  const ll X = llrint(fx), Y = llrint(fy);
  const int4 b = a.ibox[z2];
  if (X < quant((double)((ll)-b.x + a.sx0) * a.sx, g) ||
      X > quant((double)((ll)b.y + a.sx0) * a.sx, g) ||
      Y < quant((double)((ll)-b.z + a.sy0) * a.sy, g) ||
      Y > quant((double)((ll)b.w + a.sy0) * a.sy, g))
    return;
  longlong2 c;
  c.x = X;
  c.y = Y;
  a.cq[t] = c;
  const int H = a.H, W = a.W;
  // inside the box: the quotients are within the lattice's index range
  const int cj = (int)(floor(qx / a.sx) - (double)a.sx0);
  const int ci = (int)(floor(qy / a.sy) - (double)a.sy0);
  const unsigned char* split = a.split + (long long)z2 * (H - 1) * (W - 1);
  const long long base = (long long)z2 * H * W;
  for (int di = -1; di <= 1; ++di)
    for (int dj = -1; dj <= 1; ++dj) {
      const int qi = ci + di, qj = cj + dj;
      if (qi < 0 || qj < 0 || qi >= H - 1 || qj >= W - 1) continue;
      const int q = qi * (W - 1) + qj;
      const int sp = split[q];
      if (sp == 0) continue;
      for (int h = 0; h < 2; ++h) {
        int k[3], v[3];
        quad_tri(sp, h, k);
        for (int m = 0; m < 3; ++m) v[m] = corner(W, qi, qj, k[m]);
        ll P[3][2];
        tri_points(a, base, v, P);
        if (tri_contains(P, X, Y)) {
          a.qkeys[t] = (unsigned long long)q << 1 | h;
          return;
        }
      }
    }
  const int k = atomicAdd(&a.lcount[z], 1);
  a.llist[(long long)z * per + k] = r;
}

// One wave per triangle outside R; the lanes stride over the leftover list of
// the slice.  The bounding-box reject is taken on the predicate grid, where it
// is exact; the lowest key wins a query, as in the scatter.
__global__ void __launch_bounds__(kBlock) cp_scatter_o_kernel(Args a) {
  const long long per = (long long)a.Hd * a.Wd;
  const int lane = threadIdx.x & 63;
  const int nw = gridDim.x * (kBlock / 64);
  for (int z = blockIdx.y; z < a.Zq; z += gridDim.y) {
    const int z2 = compose_z2(a, z);
    const int n = a.info[z2].ntri;
    const int nl = a.lcount[z];
    if (nl == 0) continue;
    const long long base = (long long)z2 * a.H * a.W;
    const int* list = a.llist + (long long)z * per;
    const longlong2* cq = a.cq + (long long)z * per;
    unsigned long long* keys = a.qkeys + (long long)z * per;
    for (int t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < n; t += nw) {
      const int4 tr = a.tris[(long long)z2 * a.capT + t];
      const int v[3] = {tr.x, tr.y, tr.z};
      const unsigned long long key = 1ull << 63 | (unsigned long long)tr.x << (2 * kNodeBits) |
                                     (unsigned long long)tr.y << kNodeBits |
                                     (unsigned long long)tr.z;
      ll P[3][2];
      tri_points(a, base, v, P);
      ll mnx = P[0][0], mxx = P[0][0], mny = P[0][1], mxy = P[0][1];
      for (int m = 1; m < 3; ++m) {
        mnx = P[m][0] < mnx ? P[m][0] : mnx;
        mxx = P[m][0] > mxx ? P[m][0] : mxx;
        mny = P[m][1] < mny ? P[m][1] : mny;
        mxy = P[m][1] > mxy ? P[m][1] : mxy;
      }
      for (int c = lane; c < nl; c += 64) {
        const int r = list[c];
        const longlong2 q = cq[r];
        if (q.x < mnx || q.x > mxx || q.y < mny || q.y > mxy) continue;
        if (tri_contains(P, q.x, q.y)) atomicMin(&keys[r], key);
      }
    }
  }
}

// The barycentric value of abs_map2 (rel * scale in map2's type, made absolute
// and rounded to map2's type) over the winning triangle, stored as the
// reference stores it: rounded to map1's type, then made relative in it.
template <typename T1, typename T2>
__global__ void __launch_bounds__(kBlock) cp_gather_kernel(Args a) {
  const long long per = (long long)a.Hd * a.Wd;
  const long long n = (long long)a.Zq * per;
  const long long t = blockIdx.x * (long long)kBlock + threadIdx.x;
  if (t >= n) return;
  const int z = (int)(t / per), r = (int)(t % per);
  const int w = r / a.Wd, u = r % a.Wd;
  const int z2 = compose_z2(a, z);
  const unsigned long long key = a.qkeys[t];
  double ox = __builtin_nan(""), oy = __builtin_nan("");
  if (key != kEmptyKey) {
    int v[3];
    if (key >> 63) {
      const unsigned long long m = (1ull << kNodeBits) - 1;
      v[0] = (int)(key >> (2 * kNodeBits) & m);
      v[1] = (int)(key >> kNodeBits & m);
      v[2] = (int)(key & m);
    } else {
      const int q = (int)(key >> 1), h = (int)(key & 1);
      const int i = q / (a.W - 1), j = q % (a.W - 1);
      int k[3];
      quad_tri(a.split[(long long)z2 * (a.H - 1) * (a.W - 1) + q], h, k);
      for (int m = 0; m < 3; ++m) v[m] = corner(a.W, i, j, k[m]);
    }
    const long long base = (long long)z2 * a.H * a.W;
    const long long n2 = (long long)a.Z * a.H * a.W;
    const T2* map2 = static_cast<const T2*>(a.map);
    double2 p[3];
    double vx[3], vy[3];
    for (int m = 0; m < 3; ++m) {
      p[m] = a.pos[base + v[m]];
      const int i = v[m] / a.W, j = v[m] % a.W;
      T2 rx = map2[base + v[m]], ry = map2[n2 + base + v[m]];
      if (a.scale2) {
        const T2 sc = (T2)a.scale2[z];
        rx = rx * sc;
        ry = ry * sc;
      }
      vx[m] = (double)(T2)((double)rx + ((double)j * a.sx + (double)a.sx0 * a.sx));
      vy[m] = (double)(T2)((double)ry + ((double)i * a.sy + (double)a.sy0 * a.sy));
    }
    double qx, qy;
    compose_query<T1>(a, t, w, u, &qx, &qy);
    const double e1x = p[1].x - p[0].x, e1y = p[1].y - p[0].y;
    const double e2x = p[2].x - p[0].x, e2y = p[2].y - p[0].y;
    const double dx = qx - p[0].x, dy = qy - p[0].y;
    const double det = e1x * e2y - e1y * e2x;
    const double l1 = (dx * e2y - dy * e2x) / det;
    const double l2 = (e1x * dy - e1y * dx) / det;
    const double l0 = 1.0 - l1 - l2;
    ox = l0 * vx[0] + l1 * vx[1] + l2 * vx[2];
    oy = l0 * vy[0] + l1 * vy[1] + l2 * vy[2];
  }
  // ret[valid] = u (rounds to map1's type), then to_relative in that type
  const T1 rx = (T1)ox, ry = (T1)oy;
  T1* out = static_cast<T1*>(a.out);
  out[t] = (T1)((double)rx - ((double)u * a.qs + (double)a.qx0 * a.qs));
  out[n + t] = (T1)((double)ry - ((double)w * a.qs + (double)a.qy0 * a.qs));
}

unsigned pow2_at_least(unsigned long long v) {
  unsigned long long p = 1;
  while (p < v) p <<= 1;
  return (unsigned)p;
}

struct InvLayout {
  size_t pos, qpos, split, bid, used, info, blist, tris, ekeys, evals, tkeys, queue, qkeys,
      bytes;
  int capB, capT, capQ;
  unsigned capE, capTH;
};

InvLayout invmap_layout(const int32_t* shape, const int32_t* dst_shape) {
  InvLayout w{};
  const size_t Z = shape[0], H = shape[1], W = shape[2];
  const size_t nodes = Z * H * W, hw = H * W;
  const size_t quads = Z * (H > 1 ? H - 1 : 0) * (W > 1 ? W - 1 : 0);
  const size_t queries = Z * (size_t)dst_shape[0] * dst_shape[1];
  w.capB = (int)(hw < (size_t)kMaxB ? hw : (size_t)kMaxB);
  w.capT = 2 * w.capB + 8;
  w.capQ = 3 * w.capT + 2 * w.capB + 8;
  w.capE = pow2_at_least(2ull * (6ull * w.capT + 4ull * w.capB));
  w.capTH = pow2_at_least(2ull * w.capT);
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += up(bytes);
    return o;
  };
  w.pos = take(nodes * sizeof(double2));
  w.qpos = take(nodes * sizeof(longlong2));
  w.split = take(quads);
  w.bid = take(nodes * sizeof(int));
  w.used = take(nodes);
  w.info = take(Z * sizeof(SliceInfo));
  w.blist = take(Z * w.capB * sizeof(int));
  w.tris = take(Z * w.capT * sizeof(int4));
  w.ekeys = take(Z * w.capE * sizeof(unsigned));
  w.evals = take(Z * w.capE * sizeof(int));
  w.tkeys = take(Z * w.capTH * sizeof(unsigned long long));
  w.queue = take(Z * w.capQ * sizeof(unsigned));
  w.qkeys = take(queries * sizeof(unsigned long long));
  w.bytes = off > 256 ? off : 256;
  return w;
}

unsigned blocks(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// The shape and stride checks of both entry points; 0 when they pass.
int check_shapes(const char* name, const int32_t* shape, const int32_t* dst_shape, double s0,
                 double s1) {
  for (int i = 0; i < 3; ++i)
    if (shape[i] < 1) return sfm::fail(SFM_ERR_INVALID, "%s: bad shape", name);
  if (dst_shape[0] < 0 || dst_shape[1] < 0)
    return sfm::fail(SFM_ERR_INVALID, "%s: bad output shape", name);
  if (!(s0 > 0.0) || !(s1 > 0.0) || !std::isfinite(s0) || !std::isfinite(s1))
    return sfm::fail(SFM_ERR_INVALID, "%s: strides must be finite and positive", name);
  const long long hw = (long long)shape[1] * shape[2];
  if (hw > (1LL << kNodeBits))
    return sfm::fail(SFM_ERR_INVALID, "%s: %lld nodes per slice exceed 2^21", name, hw);
  if (hw * shape[0] > 0x7fffffffLL ||
      (long long)dst_shape[0] * dst_shape[1] * shape[0] > 0x7fffffffLL)
    return sfm::fail(SFM_ERR_INVALID, "%s: more than 2^31 - 1 nodes", name);
  return SFM_OK;
}

// Binds the workspace and runs steps 1 to 4 (the verified triangulation) in one
// mode on a map of type T; `queries` keys are cleared for step 5.
template <int MODE, typename T>
int triangulate(Args& a, const int32_t* shape, const int32_t* dst_shape, long long queries,
                const InvLayout& w, void* workspace, hipStream_t st) {
  char* ws = static_cast<char*>(workspace);
  a.Z = shape[0];
  a.H = shape[1];
  a.W = shape[2];
  a.Hd = dst_shape[0];
  a.Wd = dst_shape[1];
  const long long hw = (long long)a.H * a.W;
  a.pos = reinterpret_cast<double2*>(ws + w.pos);
  a.qpos = reinterpret_cast<longlong2*>(ws + w.qpos);
  a.split = reinterpret_cast<unsigned char*>(ws + w.split);
  a.bid = reinterpret_cast<int*>(ws + w.bid);
  a.used = reinterpret_cast<unsigned char*>(ws + w.used);
  a.info = reinterpret_cast<SliceInfo*>(ws + w.info);
  a.blist = reinterpret_cast<int*>(ws + w.blist);
  a.tris = reinterpret_cast<int4*>(ws + w.tris);
  a.ekeys = reinterpret_cast<unsigned*>(ws + w.ekeys);
  a.evals = reinterpret_cast<int*>(ws + w.evals);
  a.tkeys = reinterpret_cast<unsigned long long*>(ws + w.tkeys);
  a.queue = reinterpret_cast<unsigned*>(ws + w.queue);
  if constexpr (MODE != kCompose) a.qkeys = reinterpret_cast<unsigned long long*>(ws + w.qkeys);
  a.capB = w.capB;
  a.capT = w.capT;
  a.capQ = w.capQ;
  a.capE = w.capE;
  a.capTH = w.capTH;
  const long long Z = a.Z;
  const long long nodes = Z * hw;
  const long long quads = Z * (a.H - 1) * (long long)(a.W - 1);
  SFM_HIP_CHECK(hipMemsetAsync(a.status, 0, Z * sizeof(int), st));
  SFM_HIP_CHECK(hipMemsetAsync(a.used, 0, nodes, st));
  SFM_HIP_CHECK(hipMemsetAsync(a.ekeys, 0, Z * w.capE * sizeof(unsigned), st));
  SFM_HIP_CHECK(hipMemsetAsync(a.evals, 0xff, Z * w.capE * sizeof(int), st));
  SFM_HIP_CHECK(hipMemsetAsync(a.tkeys, 0, Z * w.capTH * sizeof(unsigned long long), st));
  if (queries > 0)
    SFM_HIP_CHECK(hipMemsetAsync(a.qkeys, 0xff, queries * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(im_init_kernel, dim3(blocks(Z)), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL((im_prep_kernel<MODE, T>), dim3(blocks(nodes)), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(im_quant_kernel, dim3(blocks(nodes)), dim3(kBlock), 0, st, a);
  if (quads > 0)
    hipLaunchKernelGGL(im_quad_kernel, dim3(blocks(quads)), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(im_complete_kernel, dim3((unsigned)Z), dim3(kCompleteBlock), 0, st, a);
  SFM_LAUNCH_CHECK();
  if (quads > 0)
    hipLaunchKernelGGL(im_verify_r_kernel, dim3(blocks(quads)), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(im_verify_o_kernel, dim3(16, (unsigned)Z), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(im_verify_nodes_kernel, dim3(blocks(nodes)), dim3(kBlock), 0, st, a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

// Runs the engine over a query lattice (kInvert, kResample).  `a` carries the
// map, the lattices, the status and the output.
template <int MODE, typename T>
int run(Args a, const int32_t* shape, const int32_t* dst_shape, const InvLayout& w,
        void* workspace, hipStream_t st) {
  const long long queries = (long long)shape[0] * dst_shape[0] * dst_shape[1];
  if (const int err = triangulate<MODE, T>(a, shape, dst_shape, queries, w, workspace, st))
    return err;
  const long long quads = (long long)a.Z * (a.H - 1) * (long long)(a.W - 1);
  if (queries > 0) {
    if (quads > 0)
      hipLaunchKernelGGL(im_scatter_r_kernel<MODE>, dim3(blocks(quads)), dim3(kBlock), 0, st,
                         a);
    hipLaunchKernelGGL(im_scatter_o_kernel<MODE>, dim3(64, (unsigned)a.Z), dim3(kBlock), 0, st,
                       a);
    hipLaunchKernelGGL((im_gather_kernel<MODE, T>), dim3(blocks(queries)), dim3(kBlock), 0, st,
                       a);
    SFM_LAUNCH_CHECK();
  }
  return SFM_OK;
}

// kCompose: the triangulation's workspace (no query lattice), then the keys,
// the quantized queries, the leftover lists and the boxes of the valid nodes.
struct ComposeLayout {
  InvLayout tri;
  size_t qkeys, cq, lcount, llist, ibox, bytes;
};

ComposeLayout compose_layout(const int32_t* shape1, const int32_t* shape2) {
  ComposeLayout c{};
  const int32_t none[2] = {0, 0};
  c.tri = invmap_layout(shape2, none);
  const size_t Z1 = shape1[0], queries = Z1 * (size_t)shape1[1] * shape1[2];
  size_t off = c.tri.bytes;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  c.qkeys = take(queries * sizeof(unsigned long long));
  c.cq = take(queries * sizeof(longlong2));
  c.lcount = take(Z1 * sizeof(int));
  c.llist = take(queries * sizeof(int));
  c.ibox = take((size_t)shape2[0] * sizeof(int4));
  c.bytes = off;
  return c;
}

// 0 when the shapes of a composition pass (both maps checked, z of map2 is 1 or
// map1's).
int check_compose(const SfmComposeTriDesc* d) {
  const int32_t dst[2] = {d->shape1[1], d->shape1[2]};
  for (int i = 0; i < 3; ++i)
    if (d->shape1[i] < 1) return sfm::fail(SFM_ERR_INVALID, "compose_maps_tri: bad shape");
  if (const int err = check_shapes("compose_maps_tri", d->shape2, dst, d->stride1, d->stride2))
    return err;
  if (d->shape2[0] != 1 && d->shape2[0] != d->shape1[0])
    return sfm::fail(SFM_ERR_INVALID, "compose_maps_tri: map2 has %d z slices, map1 %d",
                     d->shape2[0], d->shape1[0]);
  if ((long long)d->shape1[0] * d->shape1[1] * d->shape1[2] > 0x7fffffffLL)
    return sfm::fail(SFM_ERR_INVALID, "compose_maps_tri: more than 2^31 - 1 nodes");
  return SFM_OK;
}

template <typename T1, typename T2>
int run_compose(Args a, const SfmComposeTriDesc* d, const ComposeLayout& c, hipStream_t st) {
  char* ws = static_cast<char*>(d->workspace);
  const int32_t dst[2] = {d->shape1[1], d->shape1[2]};
  const long long Z1 = d->shape1[0], queries = Z1 * dst[0] * dst[1];
  a.Zq = (int)Z1;
  a.qkeys = reinterpret_cast<unsigned long long*>(ws + c.qkeys);
  a.cq = reinterpret_cast<longlong2*>(ws + c.cq);
  a.lcount = reinterpret_cast<int*>(ws + c.lcount);
  a.llist = reinterpret_cast<int*>(ws + c.llist);
  a.ibox = reinterpret_cast<int4*>(ws + c.ibox);
  SFM_HIP_CHECK(hipMemsetAsync(a.lcount, 0, Z1 * sizeof(int), st));
  // 0x80808080 is below every -index and index
  SFM_HIP_CHECK(hipMemsetAsync(a.ibox, 0x80, d->shape2[0] * sizeof(int4), st));
  if (const int err =
          triangulate<kCompose, T2>(a, d->shape2, dst, queries, c.tri, d->workspace, st))
    return err;
  hipLaunchKernelGGL(cp_locate_kernel<T1>, dim3(blocks(queries)), dim3(kBlock), 0, st, a);
  const unsigned gy = (unsigned)(Z1 < 65535 ? Z1 : 65535);
  hipLaunchKernelGGL(cp_scatter_o_kernel, dim3(64, gy), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL((cp_gather_kernel<T1, T2>), dim3(blocks(queries)), dim3(kBlock), 0, st, a);
  SFM_LAUNCH_CHECK();
  return SFM_OK;
}

}  // namespace

extern "C" size_t sfm_invert_map_workspace_bytes(const SfmInvertMapDesc* d) {
  if (!d) return 0;
  for (int i = 0; i < 3; ++i)
    if (d->shape[i] < 1) return 0;
  if (d->dst_shape[0] < 0 || d->dst_shape[1] < 0) return 0;
  return invmap_layout(d->shape, d->dst_shape).bytes;
}

extern "C" int sfm_invert_map(const SfmInvertMapDesc* d, double* out) {
  // an empty dst box has no output to point at
  if (!d || !d->coord_map || !d->status ||
      (!out && d->dst_shape[0] > 0 && d->dst_shape[1] > 0))
    return sfm::fail(SFM_ERR_INVALID, "invert_map: NULL argument");
  if (const int err = check_shapes("invert_map", d->shape, d->dst_shape, d->stride[0],
                                   d->stride[1]))
    return err;
  const InvLayout w = invmap_layout(d->shape, d->dst_shape);
  if (!d->workspace || d->workspace_bytes < w.bytes)
    return sfm::fail(SFM_ERR_WORKSPACE, "invert_map workspace needs %zu bytes, got %zu",
                     w.bytes, d->workspace_bytes);
  Args a{};
  a.map = d->coord_map;
  a.sy0 = d->src_start[0];
  a.sx0 = d->src_start[1];
  a.sy = d->stride[0];
  a.sx = d->stride[1];
  a.status = d->status;
  a.out = out;
  return run<kInvert, double>(a, d->shape, d->dst_shape, w, d->workspace,
                              static_cast<hipStream_t>(d->stream));
}

extern "C" size_t sfm_resample_map_workspace_bytes(const SfmResampleMapDesc* d) {
  if (!d) return 0;
  for (int i = 0; i < 3; ++i)
    if (d->shape[i] < 1) return 0;
  if (d->dst_shape[0] < 0 || d->dst_shape[1] < 0) return 0;
  return invmap_layout(d->shape, d->dst_shape).bytes;
}

extern "C" int sfm_resample_map(const SfmResampleMapDesc* d, void* out) {
  if (!d || !d->coord_map || !d->status ||
      (!out && d->dst_shape[0] > 0 && d->dst_shape[1] > 0))
    return sfm::fail(SFM_ERR_INVALID, "resample_map: NULL argument");
  if (const int err = check_shapes("resample_map", d->shape, d->dst_shape, d->src_stride,
                                   d->dst_stride))
    return err;
  const InvLayout w = invmap_layout(d->shape, d->dst_shape);
  if (!d->workspace || d->workspace_bytes < w.bytes)
    return sfm::fail(SFM_ERR_WORKSPACE, "resample_map workspace needs %zu bytes, got %zu",
                     w.bytes, d->workspace_bytes);
  Args a{};
  a.map = d->coord_map;
  a.sy0 = d->src_start[0];
  a.sx0 = d->src_start[1];
  a.sy = a.sx = d->src_stride;
  a.qy0 = d->dst_start[0];
  a.qx0 = d->dst_start[1];
  a.qs = d->dst_stride;
  a.status = d->status;
  a.out = out;
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  if (d->f64)
    return run<kResample, double>(a, d->shape, d->dst_shape, w, d->workspace, st);
  return run<kResample, float>(a, d->shape, d->dst_shape, w, d->workspace, st);
}

extern "C" size_t sfm_compose_maps_tri_workspace_bytes(const SfmComposeTriDesc* d) {
  if (!d) return 0;
  for (int i = 0; i < 3; ++i)
    if (d->shape1[i] < 1 || d->shape2[i] < 1) return 0;
  return compose_layout(d->shape1, d->shape2).bytes;
}

extern "C" int sfm_compose_maps_tri(const SfmComposeTriDesc* d, void* out) {
  if (!d || !d->map1 || !d->map2 || !d->status || !out)
    return sfm::fail(SFM_ERR_INVALID, "compose_maps_tri: NULL argument");
  if (const int err = check_compose(d)) return err;
  const ComposeLayout c = compose_layout(d->shape1, d->shape2);
  if (!d->workspace || d->workspace_bytes < c.bytes)
    return sfm::fail(SFM_ERR_WORKSPACE, "compose_maps_tri workspace needs %zu bytes, got %zu",
                     c.bytes, d->workspace_bytes);
  Args a{};
  a.map = d->map2;
  a.sy0 = d->start2[0];
  a.sx0 = d->start2[1];
  a.sy = a.sx = d->stride2;
  a.map1 = d->map1;
  a.qy0 = d->start1[0];
  a.qx0 = d->start1[1];
  a.qs = d->stride1;
  a.scale2 = d->scale2;
  a.status = d->status;
  a.out = out;
  hipStream_t st = static_cast<hipStream_t>(d->stream);
  if (d->f64_1)
    return d->f64_2 ? run_compose<double, double>(a, d, c, st)
                    : run_compose<double, float>(a, d, c, st);
  return d->f64_2 ? run_compose<float, double>(a, d, c, st)
                  : run_compose<float, float>(a, d, c, st);
}
