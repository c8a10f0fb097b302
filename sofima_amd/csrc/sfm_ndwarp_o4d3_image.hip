// The affine and render kernels of spline order 4, 3-D (no map accessor).
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_IMAGE_UNIT(4, 3)
