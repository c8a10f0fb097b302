// What the translation units of the correlation family call on each other:
// sfm_xcorr.hip (batch driver, peak kernels), sfm_xcorr_fft.hip (FFT form),
// sfm_fft_own.hip (the transforms) and the matrix-core files (sfm_mfma_host.hip
// and the units behind it, see sfm_mfma.h).  Every function here is
// declared once, and this header is included by its definer and by its callers.
#ifndef SFM_XCORR_UNITS_H_
#define SFM_XCORR_UNITS_H_

#include "sfm_common.h"

namespace sfm {

// --- sfm_mfma_host.hip: the int8 matrix-core path ----------------------------
bool mfma_i8_eligible(const SfmXcorrDesc* d);
size_t mfma_i8_workspace_bytes(const SfmXcorrDesc* d);
// Writes a surface padded to whole 16 x 16 tiles: [B, rows, pitch].
int mfma_i8_surface(const SfmXcorrDesc* d, void* ws, float* surface,
                    const FusedPeaks* fused);
void mfma_i8_padded_dims(const SfmXcorrDesc* d, int* rows, int* pitch);
// Masked correlation: the normalised surface, padded to whole tiles; `smax`
// (optional, zeroed by the caller) receives the ordered bits of every surface
// maximum for the peak search.
int mfma_i8_masked(const SfmXcorrDesc* d, void* ws, float* surface,
                   unsigned int* maxima, unsigned int* smax, float* blkmax);
// rows per block of `blkmax` (the assembly workgroups take 4 waves x 8 rows:
// sfm_mfma.h pins kWaves * kAsmRowsPerWave to it)
constexpr int kMaskedBlkRows = 32;

// --- sfm_xcorr_fft.hip -------------------------------------------------------
bool fft_preferred(const SfmXcorrDesc* d);
int fft_check(const SfmXcorrDesc* d);
size_t fft_workspace_bytes(const SfmXcorrDesc* d);
int fft_correlate(const SfmXcorrDesc* d, const float* a0, const float* b0,
                  const float* va, const float* vb, float* surface, float* den,
                  float* ov, unsigned int* maxima, void* ws, unsigned int* smax);

// --- sfm_fft_own.hip: the hand-written transforms ----------------------------
bool own_fft_supported(int rank, const int* F);
bool own_fft_fits_tile(int n);
// in-plane patches beyond one tile along both axes (full-complex path)
bool own_fft_big_supported(int rank, const int* F);
int own_fft_big_correlate(const int* P, const int* Q, const int* S, const int* F, int nb,
                          const float* a0, const float* b0, float2* sa, float2* sb, float2* tmp,
                          float* surface, unsigned int* smax, hipStream_t st);
int own_fft_big_forward(const int* R, const int* F, int nb, const float* src, int square,
                        float2* spec, float2* tmp, hipStream_t st);
int own_fft_big_inverse_product(const int* F, int nb, const float2* lhs, const float2* rhs,
                                float2* work, float2* tmp, float* real_out, hipStream_t st);
int own_fft_correlate(const int* P, const int* Q, const int* S, const int* F, int nb,
                      const float* a0, const float* b0, float2* sa, float2* sb, float* surface,
                      unsigned int* smax, hipStream_t st);
int own_fft_forward(const int* R, const int* F, int nb, const float* src, int square,
                    float2* spec, hipStream_t st);
int own_fft_inverse_product(const int* F, int nb, const float2* lhs, const float2* rhs,
                            float2* work, float* real_out, hipStream_t st);

}  // namespace sfm

#endif  // SFM_XCORR_UNITS_H_
