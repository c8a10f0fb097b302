// The nd-warp, affine and render kernels of spline order 2, 3-D.
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_UNIT(2, 3)
