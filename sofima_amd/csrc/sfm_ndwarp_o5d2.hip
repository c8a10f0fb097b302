// The nd-warp and affine kernels of spline order 5, 2-D.
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_UNIT(5, 2)
