// xcorr_mfma_kernel<15, 11, *>: one chunk geometry of the correlation kernel.
#include "sfm_mfma_kernel.h"

SFM_MFMA_GEOMETRY_UNIT(15, 11)
