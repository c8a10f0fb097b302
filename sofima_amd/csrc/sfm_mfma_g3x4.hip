// xcorr_mfma_kernel<3, 4, *>: one chunk geometry of the correlation kernel.
#include "sfm_mfma_kernel.h"

SFM_MFMA_GEOMETRY_UNIT(3, 4)
