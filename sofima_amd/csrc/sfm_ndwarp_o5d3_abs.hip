// The nd-warp kernels of spline order 5, 3-D, that read the float64 absolute map.
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_MAP_UNIT(5, 3, AbsoluteMap)
