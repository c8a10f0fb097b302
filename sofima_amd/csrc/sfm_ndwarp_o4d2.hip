// The nd-warp and affine kernels of spline order 4, 2-D.
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_UNIT(4, 2)
