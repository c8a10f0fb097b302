// Device code shared by the flow filters: sfm_flowutils.hip (clean_flow,
// reconcile_flows, one launch set per flow) and sfm_tileflows.hip (the same
// filters for a ragged batch of tile-pair flows, one workgroup per pair).
// The window, border and comparison rules are stated once, here.
#ifndef SFM_FLOWFILTER_H_
#define SFM_FLOWFILTER_H_

#include <hip/hip_runtime.h>

namespace sfm {
namespace flowfilter {

// np.nan_to_num for float32: NaN -> 0, +-inf -> +-FLT_MAX.
__device__ __forceinline__ float nan_to_num(float v) {
  if (isnan(v)) return 0.f;
  if (isinf(v)) return v > 0.f ? 3.4028234663852886e38f : -3.4028234663852886e38f;
  return v;
}

// scipy.ndimage "reflect" boundary (d c b a | a b c d | d c b a) for a
// one-element overhang.
__device__ __forceinline__ int reflect(int i, int n) {
  if (i < 0) return -i - 1 < n ? -i - 1 : n - 1;
  if (i >= n) return 2 * n - 1 - i >= 0 ? 2 * n - 1 - i : 0;
  return i;
}

// Insertion of v into the sorted window w[0 .. n).
__device__ __forceinline__ void insert_sorted(float* w, int& n, float v) {
  int k = n++;
  while (k > 0 && w[k - 1] > v) {
    w[k] = w[k - 1];
    --k;
  }
  w[k] = v;
}

// Median of the 3 x 3 window of nan_to_num(at(yy, xx)) around (y, x) of a
// [Y, X] plane, mode "reflect".
template <typename At>
__device__ __forceinline__ float median3x3(At at, int y, int x, int Y, int X) {
  float w[9];
  int n = 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx)
      insert_sorted(w, n, nan_to_num(at(reflect(y + dy, Y), reflect(x + dx, X))));
  return w[4];
}

// A float32 quantity against a threshold held as a double (the Python layer
// rounds the threshold to float32 where NumPy would compare in float32).
// Comparisons with NaN are false, as in NumPy.
__device__ __forceinline__ bool below(float v, double t) { return static_cast<double>(v) < t; }
__device__ __forceinline__ bool above(float v, double t) { return static_cast<double>(v) > t; }

// clean_flow's peak tests (flow_utils.py:62-64).
__device__ __forceinline__ bool peak_bad(float sharpness, float ratio, double min_sharp,
                                         double min_ratio) {
  const float pr = fabsf(ratio);
  return below(fabsf(sharpness), min_sharp) || (pr > 0.f && below(pr, min_ratio));
}

// reconcile_flows' gradient test (flow_utils.py:112-115) at one vector: c0 / c1
// are its channels, l / r the x neighbours' channel 0, u / d the y neighbours'
// channel 1, 0 beyond the border.  np.diff with prepend=0 / append=0: the int64
// zero promotes the field to float64, so the differences are taken in double;
// |a - b| > t is false for a NaN difference.
__device__ __forceinline__ bool gradient_bad(float c0, float c1, float l, float r, float u,
                                             float d, double max_grad) {
  const double e0 = c0, e1 = c1;
  return fabs(e0 - static_cast<double>(l)) > max_grad ||
         fabs(static_cast<double>(r) - e0) > max_grad ||
         fabs(e1 - static_cast<double>(u)) > max_grad ||
         fabs(static_cast<double>(d) - e1) > max_grad;
}

// The median-deviation test on the two deviations |median - value|: np.max over
// the channels propagates NaN, and NaN > t is false.
__device__ __forceinline__ bool deviation_bad(float d0, float d1, double max_dev) {
  return !isnan(d0) && !isnan(d1) && above(fmaxf(d0, d1), max_dev);
}

// Union-find on int32 vector indices (Playne & Hawick 2018); -1 marks an
// invalid vector.  Parents only ever point to smaller indices (hooks and path
// halving are atomicMin), so find and union terminate by construction.
// kScope: the memory scope of the parent array -- agent for global memory
// shared by all workgroups, workgroup for LDS.
template <int kScope>
__device__ __forceinline__ int load_parent(const int* p, int i) {
  return __hip_atomic_load(p + i, __ATOMIC_RELAXED, kScope);
}

template <int kScope>
__device__ __forceinline__ int lower_parent(int* p, int i, int v) {
  return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, kScope);
}

// Root of i, halving the path on the way (p[i] <- p[p[i]], never upwards).
template <int kScope>
__device__ int find_root(int* p, int i) {
  while (true) {
    const int q = load_parent<kScope>(p, i);
    if (q == i) return i;
    const int g = load_parent<kScope>(p, q);
    if (g == q) return q;
    lower_parent<kScope>(p, i, g);
    i = g;
  }
}

// Hooks the larger root under the smaller; when the hook loses a race (the
// larger root got a parent meanwhile) it retries from that parent.
template <int kScope>
__device__ void unite(int* p, int a, int b) {
  while (true) {
    a = find_root<kScope>(p, a);
    b = find_root<kScope>(p, b);
    if (a == b) return;
    if (a > b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = lower_parent<kScope>(p, b, a);
    if (old == b) return;
    b = old;
  }
}

}  // namespace flowfilter
}  // namespace sfm

#endif  // SFM_FLOWFILTER_H_
