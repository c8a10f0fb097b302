// The nd-warp, affine and render kernels of orders 0 and 1 (ORDER = 0), 2-D and 3-D.
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_UNIT(0, 2)
SFM_NDWARP_UNIT(0, 3)
