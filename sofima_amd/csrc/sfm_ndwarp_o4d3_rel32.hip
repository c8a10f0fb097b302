// The nd-warp kernels of spline order 4, 3-D, that read a relative float32 map.
#include "sfm_ndwarp_kernel.h"

SFM_NDWARP_MAP_UNIT(4, 3, RelativeMapArgs<float>)
