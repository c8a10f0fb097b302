// xcorr_mfma_kernel<20, 11, *>: one chunk geometry of the correlation kernel.
#include "sfm_mfma_kernel.h"

SFM_MFMA_GEOMETRY_UNIT(20, 11)
