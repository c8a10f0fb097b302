// The nd-warp kernels of spline order 5, 3-D, that read a relative float64 map.
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_MAP_UNIT(5, 3, RelativeMapArgs<double>)
