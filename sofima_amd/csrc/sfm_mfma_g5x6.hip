// xcorr_mfma_kernel<5, 6, *>: one chunk geometry of the correlation kernel.
#include "sfm_mfma_kernel.h"

SFM_MFMA_GEOMETRY_UNIT(5, 6)
