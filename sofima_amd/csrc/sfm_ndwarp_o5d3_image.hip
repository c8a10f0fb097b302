// The affine and render kernels of spline order 5, 3-D (no map accessor).
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_IMAGE_UNIT(5, 3)
