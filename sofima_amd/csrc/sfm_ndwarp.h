// The map_coordinates family on the device: ndimage_warp (orders 0 .. 5, with and
// without SciPy's boundary modes, absolute and relative maps), the fused affine warp
// and the 3-D tile render.
//
// The translation units of the family and what they share:
//   sfm_ndwarp_kernel.h   the kernels and their launch templates;
//                         sfm_ndwarp_o<order>[d<dim>[_<map>]].hip instantiates the kernels
//                         of one (spline order, dimension) each, or of one map of it
//   sfm_warp.hip          the host side: every entry point of the family, the checks,
//                         the choice of the unit
// Here: what both sides see -- the kernel arguments, the map accessors, the list of the
// units and the launch functions that sfm_warp.hip calls.
#ifndef SFM_NDWARP_H_
#define SFM_NDWARP_H_

#include "sfm_common.h"
#include "sfm_ndsample.h"

namespace sfm {

constexpr int kNdBlock = 256;            // nd-warp and affine: one thread per output voxel
constexpr int kBrickX = 64, kBrickY = 4; // render: the brick of a workgroup

// The map of a launch, as the kernels read it: channel<DIM>(d, nodes, stride) is
// the accessor of the channel that gives the dense coordinate of axis d (channel
// DIM - 1 - d: channels are x, y[, z]) for sfm::linear_sample.
//
// AbsoluteMap: the float64 absolute source map that the caller prepared.
struct AbsoluteMap {
  const double* m;
  template <int DIM>
  __device__ __forceinline__ const double* channel(int d, long long nodes, const double*) const {
    return m + (long long)(DIM - 1 - d) * nodes;
  }
};
// RelativeMapArgs: the relative map in its own type; the absolute value of a node
// is formed on every read (sfm::RelativeMap).  shift and scale are per channel.
template <typename M>
struct RelativeMapArgs {
  const M* m;
  int has_shift;
  double shift[3], scale[3];
  template <int DIM>
  __device__ __forceinline__ sfm::RelativeMap<M, DIM> channel(int d, long long nodes,
                                                              const double* stride) const {
    const int c = DIM - 1 - d;
    return {m + (long long)c * nodes, d, has_shift != 0, stride[3 - DIM + d], shift[c], scale[c]};
  }
};

template <typename MAP>
struct NdWarpArgs {
  const void* image;
  MAP map;
  void* out;
  int order;
  int ishape[3], mshape[3], oshape[3];
  double stride[3], offset[3];
};

struct AffineArgs {
  const void* image;
  void* out;
  int order;
  int shape[3];     // of out
  int ishape[3];    // of what is sampled: shape, or with b.pad the padded coefficients
  double m[3][3], off[3];
  sfm::Boundary b;
};

struct RenderArgs {
  const SfmRenderTile* tiles;
  const double* coeffs;   // spline orders: the crops' coefficients, back to back
  void* out;
  int n_tiles, order;
  int oshape[3];
  double stride[3];
};

// The units that hold the kernels, as X(ORDER, DIM): ORDER 0 stands for the kernels
// of orders 0 and 1, which read the image and take the order at run time.
// (tests/test_build.py holds the files of the family against this list.)
#define SFM_NDWARP_UNITS(X) \
  X(0, 2) X(0, 3) X(2, 2) X(2, 3) X(3, 2) X(3, 3) X(4, 2) X(4, 3) X(5, 2) X(5, 3)

// A launch as the host side decided it; dtype is a checked SFM_DTYPE_U8 / U16 / F32.
struct NdLaunch {
  dim3 grid, block;
  hipStream_t stream;
  int dtype;
};

// --- the units: the launches ---------------------------------------------------
// Each picks the kernel of l.dtype among those of its (ORDER, DIM).  bnd: SciPy's
// boundary mode on both steps (the mode kernels), else nullptr; taps: orders 2 .. 5
// under a mode whose taps do not mirror (the TAPS kernels).
template <int ORDER, int DIM, typename MAP>
int launch_ndwarp(const NdWarpArgs<MAP>& a, const Boundary* bnd, bool taps, const NdLaunch& l);
template <int ORDER, int DIM>
int launch_affine(const AffineArgs& a, bool taps, const NdLaunch& l);
// (3-D only) out_f32: float32 output from integer tiles
template <int ORDER>
int launch_render(const RenderArgs& a, bool out_f32, const NdLaunch& l);

}  // namespace sfm

#endif  // SFM_NDWARP_H_
