/* sofima_amd.h -- C ABI of libsofima_amd.so (MI355X / gfx950).
 *
 * The library is the drop-in device back end for the two compute cores of
 * SOFIMA.  The reference has no FFI: its "operator API" is the Python
 * signatures of flow_field.py / mesh.py.  Each entry point below names the
 * reference function (file:line under /root/reference) whose device work it
 * replaces; sofima_amd/flow_field.py and sofima_amd/mesh.py bind them through
 * ctypes with exactly the reference's Python signatures.
 *
 * Conventions
 *   - plain C types only; every buffer is CALLER-OWNED device memory (HIP
 *     pointers, e.g. torch.Tensor.data_ptr()); the library never frees or
 *     keeps caller memory, and scratch space is passed in as `workspace`.  The
 *     only device memory it owns: the twiddle tables of the hand-written FFT
 *     (8 bytes per sample of a transform length, per device), cached for the
 *     process;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream).  Entry points do not synchronise unless stated;
 *   - return 0 on success, a negative SFM_ERR_* otherwise; the message is in
 *     sfm_last_error() (thread-local).  No C++ exception crosses the boundary;
 *   - image / mask / surface arrays are row-major [z,]y,x; mesh arrays are
 *     [C, batch, z, y, x] with C = 2|3 vector components in x,y[,z] order;
 *   - shapes, sizes and starts are given in [z]yx order padded to 3 entries:
 *     for 2-D data entry 0 is 1 (sizes) or 0 (starts).
 */
#ifndef SOFIMA_AMD_H_
#define SOFIMA_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_ABI_VERSION 9   /* 4: SfmProfile.mfma_issued; sfm_mesh_relax_banded; 5: SfmWarpDesc.coord_map_f64;
                                6: SfmBandedDesc.host_halo / host_allgather / host_user;
                                7: sfm_ndimage_warp; 8: SfmProfile.tiles_abandoned;
                                9: SfmMaskIrregularDesc and SfmCleanFlowDesc carry
                                   double thresholds; sfm_map_shift, sfm_map_extents,
                                   sfm_affine_map and sfm_warp_points were added
                                   without a bump: new entry points only, no
                                   existing struct or call changed; likewise
                                   sfm_prev_state, sfm_mask_irregular_f64,
                                   sfm_render_tiles3d, and sfm_spline_prefilter,
                                   sfm_ndimage_warp_spline and
                                   sfm_render_tiles3d_spline, and
                                   sfm_ndimage_warp_mode and sfm_affine_warp, and
                                   sfm_ndimage_warp_rel, and
                                   sfm_spline_prefilter_mode and sfm_spline_mode_pad
                                   (with them the switch SFM_SPLINE_MODES, under
                                   which the mode entry points read padded
                                   coefficients for two modes; off: unchanged),
                                   and sfm_fill_missing_nearest with
                                   sfm_fill_missing_nearest_workspace_bytes, and
                                   sfm_resample_map with
                                   sfm_resample_map_workspace_bytes, and
                                   sfm_compose_maps_tri with
                                   sfm_compose_maps_tri_workspace_bytes */

#define SFM_OK 0
#define SFM_ERR_INVALID (-1)     /* bad argument / unsupported combination */
#define SFM_ERR_HIP (-2)         /* a HIP runtime call failed              */
#define SFM_ERR_WORKSPACE (-3)   /* workspace missing or too small         */
#define SFM_ERR_NO_DEVICE (-4)   /* no gfx950 device visible               */

#define SFM_DTYPE_U8 0
#define SFM_DTYPE_F32 1
#define SFM_DTYPE_U16 2          /* warping only                               */
#define SFM_DTYPE_I32 3          /* warping only: contiguous segment ids       */

/* Which correlation kernel family to use. AUTO picks MFMA_I8 whenever the
 * inputs qualify (uint8 images, 2-D, no masks in the correlation) and DIRECT
 * otherwise. */
#define SFM_XCORR_AUTO 0
#define SFM_XCORR_DIRECT 1    /* f32 shift-by-shift kernel, any dtype/dim/mask */
#define SFM_XCORR_MFMA_I8 2   /* int8 MFMA Toeplitz kernel                   */
#define SFM_XCORR_FFT 3       /* zero-padded rFFT form (3-D / large patches)  */

int sfm_version(void);
const char* sfm_last_error(void);
/* Number of visible HIP devices (0 and SFM_OK when none). */
int sfm_device_count(int* count);

/* Behaviour switches.  Every switch selects between kernels / schedules that
 * return the SAME results (the tests pin the variants against each other);
 * they exist for A/B measurements and for the tests themselves.  A switch set
 * here wins over the environment variable of the same name, which is only the
 * default; value NULL removes the explicit setting again.
 * sfm_get_option copies the value in effect (returns 1 and "" when unset).
 *   SFM_MFMA_PRUNE=0      correlation kernel computes every surface tile
 *   SFM_MFMA_LAZY=0       flow path stores every computed surface tile (default:
 *                         only the tiles the peak kernels can read)
 *   SFM_MFMA_EARLY=n      lazy path: least number of row groups between two tests that
 *                         abandon a provably cold tile inside its row loop, or narrow
 *                         it (default 1; each test schedules the next; 0: no tests)
 *   SFM_MFMA_NARROW=n     lazy path: widest in-flight narrowing of a row loop (outer column
 *                         tiles dropped once proved cold; default: down to the four
 *                         central tiles; 0: never)
 *   SFM_MFMA_RUN=n        same-size correlation launches: consecutive patches a workgroup takes
 *                         per ticket of the patch queue (default 8; the end of a batch always
 *                         goes out one patch at a time; 1: one patch per ticket throughout)
 *   SFM_MFMA_LAZYG=0      the prep kernel writes the whole correction table (default, pruned
 *                         flow launches: the finishing tiles build their 16 rows; the prep pass
 *                         then keeps no patch in LDS)
 *   (measurement-only, honoured by a library built with -DSFM_MEASUREMENT_SWITCHES only --
 *   sfm_get_option("SFM_BUILD_MEASUREMENT_SWITCHES") = "1"; the production build ignores them:)
 *   SFM_MFMA_PROBE=0      no seed probe in front of the pruning
 *   SFM_MFMA_TOUCH_ALL=1  lazy path: pull a patch's whole correction table into L2
 *   SFM_MFMA_EXACT=0      run-time instead of compile-time column geometry
 *   SFM_MFMA_QUEUE=0      static instead of dynamic patch queue
 *   SFM_MFMA_RUN_TAIL=n   patch queue: n x grid patches at the end of a batch go out one at a
 *                         time (default 8)
 *   SFM_MFMA_PRIO=n       wave priority experiment (0..3)
 *   SFM_MFMA_MAX_WG_PER_CU=n   occupancy cap of the correlation kernel
 *   SFM_MFMA_GUARD_2R=1   lazy / pruned path: the row band around hot rows and pruned tiles
 *                         is 2 x peak_radius rows everywhere (default: the rows the peak
 *                         kernels can read -- the clamped window and min_distance)
 *   SFM_SPLINE_MODES=1    (not a same-result switch: it adds a capability) spline orders
 *                         2 .. 5 take the boundary modes nearest, reflect, grid-constant and
 *                         grid-wrap (sfm_spline_prefilter_mode; default: rejected)
 *   SFM_MASKED_FAST=0     masked patches always take all eight passes
 *   SFM_MASKED_DEADROWS=0 no overlap-rule skips in the masked assembly
 *   SFM_MASKED_GROUPS=n   masked matrix-core path: reference batches (`group` patches each)
 *                         processed per round of a call (default 8).  The workspace of a masked
 *                         call -- sfm_xcorr_workspace_bytes -- is sized for n groups (about 4 GB
 *                         per 1024 patches of 160^2): a caller with a tight memory budget and a
 *                         small `group` sets a smaller n BEFORE asking for the size
 *   SFM_PHASE_XCD=0       masked assembly without the XCD-aware tile order
 *   SFM_MESH_PERSISTENT=0 / SFM_MESH_SPECULATE=0 / SFM_MESH_TILED=0 /
 *   SFM_MESH_SMALL=0 / SFM_MESH_FUSE_TARGET=0
 *                         fall back to the simpler integrator
 *   SFM_MESH_MARCH3D=0|1  default-link volumes (elastic_mesh_3d): the z-march integrator that
 *                         evaluates every spring once -- never / for every volume (default:
 *                         from 1.5 * 10^6 nodes on).  Forces bit-identical to the per-node kernel.
 *   SFM_MESH_MARCH3D_T=256|512|1024 / SFM_MESH_MARCH3D_ZC=n
 *                         its workgroup size / planes per workgroup (default: planned per mesh)
 *   SFM_MESH_PACK=0       tiled in-plane step: a workgroup per tile also in a narrow last
 *                         tile column (default: its tile rows share workgroups)
 *   SFM_MESH_TILE=16|32   tile edge of the persistent integrator
 *   SFM_MESH_XCD=0|1      tiled in-plane step: one contiguous run of tiles per
 *                         XCD never / always (default: from 2048 tiles on)   */
int sfm_set_option(const char* name, const char* value);
int sfm_get_option(const char* name, char* value, size_t capacity);

/* Kernel timing hooks (used by bench.py for the roofline figures; no
 * reference counterpart).  While enabled, hipEvents on the launch stream
 * bracket every launch of the dominant kernels: the patch-correlation kernel
 * (kind 0) and the mesh integrate kernel (kind 1).  sfm_profile_read waits for
 * the recorded events, returns the accumulated kernel time and launch count
 * per kind since the last read, and resets the counters. */
typedef struct SfmProfile {
  double kernel_ms[2];
  int64_t launches[2];
  double clock_mhz[2];          /* sustained shader clock inside the kernels of
                                   that kind (s_memtime / s_memrealtime of one
                                   workgroup); 0 when not sampled             */
  int64_t tiles_skipped[2];     /* kind 0: surface row tiles the exact pruning of
                                   the fused-peaks kernel skipped / looked at   */
  int64_t tiles_drawn[2];
  int64_t col_tiles_skipped[2]; /* column tiles left out of the computed row tiles */
  int64_t mfma_issued[2];       /* kind 0: matrix instructions (16 x 16 x 64 int8 =
                                   32768 operations each) the kernel issued      */
  int64_t tiles_abandoned[2];   /* kind 0: row tiles given up inside their row loop
                                   (proved cold by the rows still to come)       */
} SfmProfile;
int sfm_profile_enable(int on);
int sfm_profile_read(SfmProfile* out);

/* ------------------------------------------------------------------------
 * Patch cross-correlation + peak statistics for ONE batch.
 * Replaces flow_field.batched_xcorr_peaks (flow_field.py:374-441) =
 * _batched_xcorr (:278-371) + masked_xcorr(use_jax=True) (:36-156) +
 * _batched_peaks (:205-275) + _peak_stats (:178-202).
 * ---------------------------------------------------------------------- */
typedef struct SfmXcorrDesc {
  int32_t ndim;                 /* 2 or 3                                    */
  int32_t dtype;                /* SFM_DTYPE_* of pre/post image             */
  const void* pre_image;        /* device, [z,]y,x                           */
  const void* post_image;
  const uint8_t* pre_mask;      /* device bool bytes (1 = invalid) or NULL   */
  const uint8_t* post_mask;
  int32_t pre_shape[3];         /* [z]yx, entry 0 = 1 for 2-D                */
  int32_t post_shape[3];
  int32_t pre_mask_shape[3];    /* masks may differ in shape from the images */
  int32_t post_mask_shape[3];
  int32_t patch[3];             /* pre patch size  P                         */
  int32_t post_patch[3];        /* post patch size Q (<= P)                  */
  const int32_t* pre_starts;    /* device [batch, ndim] [z]yx, row-major     */
  const int32_t* post_starts;   /* device [batch, ndim]                      */
  int32_t batch;                /* rows in the starts arrays (incl. padding) */
  int32_t group;                /* rows per reference batch, see below; 0 = batch */
  int32_t use_mean;             /* 0: subtract per-patch mean; 1: use `mean` */
  float mean;
  int32_t min_distance;         /* max-filter half width (reference: 2)      */
  float threshold_rel;          /* reference: 0.5                            */
  int32_t peak_radius[3];       /* [z]yx sharpness window radius             */
  int32_t method;               /* SFM_XCORR_*                               */
  void* workspace;              /* device scratch                            */
  size_t workspace_bytes;
  void* stream;
} SfmXcorrDesc;

/* Scratch bytes sfm_xcorr_peaks / sfm_xcorr_surface need for this desc. */
size_t sfm_xcorr_workspace_bytes(const SfmXcorrDesc* desc);

/* peaks: device float [batch, ndim + 2] = x, y[, z], sharpness, ratio.
 * The batch-coupled behaviours of the reference (second-peak suppression set,
 * batch-global masked-NCC tolerances) are computed over every run of `group`
 * consecutive rows separately (the last run may be shorter): one call can
 * carry many reference batches (flow_field.py:610-699) in one launch and
 * still returns what the reference returns batch by batch. */
int sfm_xcorr_peaks(const SfmXcorrDesc* desc, float* peaks);

/* surface: device float [batch, *(P + Q - 1)]; the array masked_xcorr returns
 * for the mean-subtracted patches (flow_field.py:361-371). */
int sfm_xcorr_surface(const SfmXcorrDesc* desc, float* surface);

/* Masked-pixel count of every patch of the sampling grid.  Replaces
 * flow_field._integral_image (flow_field.py:159-175) + the box query of the
 * summed-area table (flow_field.py:575-589) used for patch selection:
 * counts[o] = number of non-zero mask bytes in the patch of size `patch` at
 * o * step, for o in [0, (shape - patch) / step] per axis. */
typedef struct SfmMaskCountDesc {
  int32_t ndim;
  int32_t shape[3];             /* mask [z]yx                                */
  int32_t patch[3];
  int32_t step[3];
  const uint8_t* mask;          /* device bool bytes                         */
  void* stream;
} SfmMaskCountDesc;

/* counts: device int32 [prod((shape - patch) / step + 1)], row-major. */
int sfm_mask_patch_counts(const SfmMaskCountDesc* desc, int32_t* counts);

/* ------------------------------------------------------------------------
 * The host loop of flow_field() on the device.
 * sfm_flow_starts replaces the per-batch start arithmetic (flow_field.py:
 * 620-680): post start = grid position * step; pre start = post start -
 * (patch - post_patch) / 2 clipped at 0; optional integer shifts looked up in
 * the targeting fields (nearest cell, nan_to_num, truncation) and kept inside
 * the images; final clip at 0.  sfm_flow_scatter replaces the per-patch result
 * scatter (:701-709), undoing the targeting shifts.
 * All shapes / steps are [z]yx padded to 3 entries in front.
 * ---------------------------------------------------------------------- */
typedef struct SfmFlowStartsDesc {
  int32_t ndim;
  int32_t n;                    /* patches (rows of `positions`)             */
  int32_t step[3];
  int32_t patch[3];
  int32_t post_patch[3];
  int32_t pre_shape[3];         /* image shapes                              */
  int32_t post_shape[3];
  const int32_t* positions;     /* device [n, ndim] grid positions, [z]yx    */
  const float* pre_targeting_field;   /* device [ndim, *shape] (x, y[, z]) or NULL */
  const float* post_targeting_field;
  int32_t pre_targeting_shape[3];
  int32_t post_targeting_shape[3];
  int32_t pre_targeting_step[3];
  int32_t post_targeting_step[3];
  int32_t* pre_starts;          /* out, device [n, ndim]                     */
  int32_t* post_starts;
  int32_t* pre_offsets;         /* out, device [n, ndim]; required with the  */
  int32_t* post_offsets;        /* corresponding targeting field             */
  void* stream;
} SfmFlowStartsDesc;

int sfm_flow_starts(const SfmFlowStartsDesc* desc);

typedef struct SfmFlowScatterDesc {
  int32_t ndim;
  int32_t n;
  int32_t grid[3];              /* output grid, [z]yx                        */
  const float* peaks;           /* device [n, ndim + 2]                      */
  const int32_t* positions;     /* device [n, ndim]                          */
  const int32_t* pre_offsets;   /* device [n, ndim] or NULL                  */
  const int32_t* post_offsets;
  float* out;                   /* device [ndim + 2, *grid], pre-filled (NaN) */
  void* stream;
} SfmFlowScatterDesc;

int sfm_flow_scatter(const SfmFlowScatterDesc* desc);

/* Patch selection and ordered compaction of a 2-D flow_field() call in one
 * launch (flow_field.py:570-589, :607, :614-618): a node of the [ny, nx] grid is
 * selected where its selection byte is not 0 and, for each count plane given,
 * !(double(count) / double(area) >= max_masked).  `positions` receives the
 * (y, x) of the selected nodes in row-major order (np.where's); rows n ..
 * total - 1 repeat row n - 1, total = ceil(n / batch_size) * batch_size;
 * counts[0] = n, counts[1] = total (0 and 0 when nothing is selected).  The
 * count planes are those of sfm_mask_patch_counts; their grids may be larger
 * than [ny, nx] (the [out_sel] crop), never smaller (SFM_ERR_INVALID). */
typedef struct SfmFlowSelectDesc {
  int32_t grid[2];              /* ny, nx                                    */
  int32_t batch_size;
  int32_t capacity;             /* rows of `positions`, >= ceil(ny * nx / batch_size) * batch_size */
  const uint8_t* selection;     /* device [ny, selection_pitch]              */
  int32_t selection_pitch;      /* elements per row, >= nx                   */
  int32_t pre_grid[2];          /* rows, columns of pre_counts               */
  const int32_t* pre_counts;    /* device [pre_grid[0], pre_pitch] or NULL   */
  int32_t pre_pitch;
  int32_t pre_area;             /* pixels of a pre patch                     */
  double pre_max_masked;
  int32_t post_grid[2];
  int32_t post_pitch;
  int32_t post_area;
  const int32_t* post_counts;   /* device [post_grid[0], post_pitch] or NULL */
  double post_max_masked;
  int32_t* positions;           /* out, device [capacity, 2]                 */
  int32_t* counts;              /* out, device [2]: n, total                 */
  void* stream;
} SfmFlowSelectDesc;

int sfm_flow_select(const SfmFlowSelectDesc* desc);

/* The accept / update step of one look-back round of EstimateMissingFlow
 * (processor/flow.py:806-828) and the attempts cap of the next round (:785).
 * Per node of the [sy, sx] field (the top-left part of the [ny, nx] section):
 * a finite field[0] counts an attempt; the node is updated where its mask byte
 * is set, field[0] is finite and clean_flow(max_deviation = 0) would keep the
 * vector; an update writes field[0], field[1] and delta_z into the three
 * planes, clears the mask byte and is counted in *filled.  Then, for every
 * node of the section, mask &= attempts <= max_attempts.  The thresholds are
 * compared in double, as in SfmCleanFlowDesc; max_magnitude 0 disables that
 * test.  *filled is added to, never cleared. */
typedef struct SfmMissingFlowDesc {
  int32_t shape[2];             /* ny, nx of the section                     */
  int32_t field_shape[2];       /* sy <= ny, sx <= nx                        */
  const float* field;           /* device [4, sy, sx]                        */
  float* out[3];                /* device [ny, nx] planes: x, y, look-back   */
  uint8_t* mask;                /* device [ny, nx], nodes still to estimate  */
  int32_t* attempts;            /* device [ny, nx]                           */
  double min_peak_ratio;
  double min_peak_sharpness;
  double max_magnitude;
  int32_t delta_z;
  int32_t max_attempts;
  int64_t* filled;              /* device, this round's counter              */
  void* stream;
} SfmMissingFlowDesc;

int sfm_missing_flow_update(const SfmMissingFlowDesc* desc);

/* Stand-alone peak statistics, replaces _batched_peaks (flow_field.py:205-275)
 * for a caller-provided batch of surfaces.  A surface that holds a NaN or a
 * +inf has no peak (a NaN row; its first-peak index counts as 0 in the batch's
 * suppression set); the sharpness window is clipped to a surface smaller than
 * 2 * peak_radius + 1.  SFM_ERR_INVALID for a negative min_distance or a
 * negative peak_radius on a used axis. */
typedef struct SfmPeaksDesc {
  int32_t ndim;
  int32_t batch;
  int32_t shape[3];             /* surface [z]yx                             */
  float center_offset[3];       /* [z]yx                                     */
  int32_t min_distance;
  float threshold_rel;
  int32_t peak_radius[3];
  const float* surface;         /* device [batch, *shape]                    */
  void* workspace;
  size_t workspace_bytes;
  void* stream;
} SfmPeaksDesc;

size_t sfm_peaks_workspace_bytes(const SfmPeaksDesc* desc);
int sfm_peaks(const SfmPeaksDesc* desc, float* peaks);

/* ------------------------------------------------------------------------
 * Coordinate-map composition.
 * Replaces map_utils.compose_maps_fast (map_utils.py:616-734): bilinear /
 * trilinear resampling of map2 (absolute) at the targets of map1, result in
 * map1's relative format.  Maps are float [C, z, y, x], C = 2 (every z
 * section independently in-plane) or 3 (volumetric).
 * ---------------------------------------------------------------------- */
#define SFM_INTERP_NEAREST 0   /* out-of-range corner indices are clamped      */
#define SFM_INTERP_CONSTANT 1  /* out-of-range corners read as NaN             */

typedef struct SfmComposeDesc {
  int32_t ncomp;                /* 2 or 3                                    */
  int32_t mode;                 /* SFM_INTERP_*                              */
  int32_t shape1[3];            /* z, y, x of map1 (and of the output)       */
  int32_t shape2[3];            /* z, y, x of map2                           */
  float start1[3];              /* zyx origin of map1 (z ignored for C = 2)  */
  float start2[3];
  float stride1[3];             /* zyx node spacing of map1                  */
  float stride2[3];
  const float* map1;            /* device [C, *shape1]                       */
  const float* map2;            /* device [C, *shape2]                       */
  void* stream;
} SfmComposeDesc;

int sfm_compose_maps(const SfmComposeDesc* desc, float* out);

/* ------------------------------------------------------------------------
 * Flow-field clean-up, the step between flow estimation and mesh relaxation.
 * Replaces flow_utils.clean_flow (flow_utils.py:37-78): invalidates (NaN)
 * vectors with low peak sharpness / peak ratio, too large components, or a
 * too large deviation from the 3 x 3 (x 3) median of the nan_to_num'ed field
 * (scipy.ndimage.median_filter, mode "reflect").  The float32 quantities are
 * compared with the thresholds in double: to compare in float32, as NumPy does
 * with a Python number, pass the threshold rounded to float32.
 * ---------------------------------------------------------------------- */
typedef struct SfmCleanFlowDesc {
  int32_t dim;                  /* 2 or 3 spatial dimensions                 */
  int32_t channels;             /* dim .. dim + 2 input channels             */
  int32_t shape[3];             /* z, y, x                                   */
  double min_peak_ratio;
  double min_peak_sharpness;
  double max_magnitude;         /* <= 0: not applied                         */
  double max_deviation;         /* <= 0: not applied                         */
  const float* flow;            /* device [channels, z, y, x]                */
  void* stream;
} SfmCleanFlowDesc;

/* out: device float [dim, z, y, x]. */
int sfm_clean_flow(const SfmCleanFlowDesc* desc, float* out);

/* ------------------------------------------------------------------------
 * Flow reconciliation, the step between clean-up and mesh relaxation.
 * Replaces flow_utils.reconcile_flows (flow_utils.py:81-135): flows 1..K-1
 * fill (all channels) where the merged channel 0 is NaN (3 channels: and
 * |dz| >= min_delta_z); then, each only when its threshold is > 0, vectors are
 * invalidated (all channels NaN) where the zero-padded x / y differences of
 * channel 0 / 1 exceed max_gradient, where channel 0 or 1 deviates from the
 * 3 x 3 median of the nan_to_num'ed field (per z slice, mode "reflect") by
 * more than max_deviation, and where the 4-connected component of valid
 * (NaN-free) vectors in its z slice has fewer than min_patch_size vectors.
 * As in the reference, the invalid vectors of a slice count as one more
 * component: when there are fewer than min_patch_size of them they become
 * all-NaN too.  Bit-exact: values are only copied, subtracted or compared.
 * The gradient differences are taken in double (np.diff's zero padding
 * promotes the field to float64) and compared with max_gradient in double.
 * The float32 deviations and |dz| are compared with max_deviation /
 * min_delta_z in double: to compare in float32, as NumPy does with a Python
 * number, pass the threshold rounded to float32.  At most 2^31 - 1 vectors
 * (int32 indices); out must not overlap flows.
 * ---------------------------------------------------------------------- */
typedef struct SfmReconcileDesc {
  int32_t channels;             /* 2 or 3                                    */
  int32_t shape[3];             /* z, y, x                                   */
  int32_t num_flows;            /* K >= 1                                    */
  double max_gradient;          /* <= 0: not applied                         */
  double max_deviation;         /* <= 0: not applied                         */
  double min_delta_z;           /* 3 channels only                           */
  int64_t min_patch_size;       /* <= 0: not applied                         */
  const float* flows;           /* device [K, channels, z, y, x], packed, in
                                   order of decreasing preference            */
  void* workspace;              /* sfm_reconcile_flows_workspace_bytes()     */
  size_t workspace_bytes;
  void* stream;
} SfmReconcileDesc;

/* Host arithmetic only (callable without a GPU); 0 for a NULL descriptor or
 * an empty shape. */
size_t sfm_reconcile_flows_workspace_bytes(const SfmReconcileDesc* desc);
/* out: device float [channels, z, y, x].  SFM_ERR_WORKSPACE when the
 * workspace is missing or too small. */
int sfm_reconcile_flows(const SfmReconcileDesc* desc, float* out);

/* ------------------------------------------------------------------------
 * The fine flows of a tile montage: clean_flow, then reconcile_flows of that
 * one flow, for a ragged batch of n in-plane tile-pair flows in ONE launch
 * (one workgroup per pair, the pair stays in LDS).  Pair p occupies
 * flows[:, p, :h, :w] of the packed [channels, n, Y, X] input, (h, w) =
 * extents[p]; what lies outside is never read.  Every pair is filtered on its
 * own extent -- borders, the 3 x 3 "reflect" windows and the invalid count of
 * the small-component test are those of [h, w], not of [Y, X] -- and gives,
 * bit for bit, what sfm_clean_flow (z = 1, dim = 2) followed by
 * sfm_reconcile_flows (K = 1, 2 channels) give for that pair alone, with the
 * comparison rules of SfmCleanFlowDesc / SfmReconcileDesc.  4 channels:
 * channel 2 is the peak sharpness, channel 3 the peak ratio.  do_clean = 0
 * takes channels 0 / 1 as they are; do_reconcile = 0 stops after the clean-up.
 * A pair holds at most sfm_filter_tile_flows_max_nodes() vectors (what 160 KB
 * of LDS hold at 12 bytes per vector).
 * ---------------------------------------------------------------------- */
typedef struct SfmTileFlowsDesc {
  int32_t channels;             /* 2 or 4                                    */
  int32_t n;                    /* tile pairs                                */
  int32_t padded_shape[2];      /* Y, X of the packed arrays                 */
  const int32_t* extents;       /* HOST [n, 2]: h, w of every pair           */
  const int32_t* extents_device;/* the same table in device memory           */
  double min_peak_ratio;        /* clean-up, 4 channels only                 */
  double min_peak_sharpness;
  double max_magnitude;         /* <= 0: not applied                         */
  double clean_max_deviation;   /* <= 0: not applied                         */
  double max_gradient;          /* reconciliation; <= 0: not applied         */
  double max_deviation;         /* <= 0: not applied                         */
  double min_delta_z;           /* 3-channel flows only: not read            */
  int64_t min_patch_size;       /* <= 0: not applied                         */
  int32_t do_clean;
  int32_t do_reconcile;
  const float* flows;           /* device [channels, n, Y, X]                */
  void* stream;
} SfmTileFlowsDesc;

/* out: device float [2, n, Y, X], NaN outside a pair's extent; must not
 * overlap flows. */
int sfm_filter_tile_flows(const SfmTileFlowsDesc* desc, float* out);
/* Host arithmetic only (callable without a GPU). */
int sfm_filter_tile_flows_max_nodes(void);

/* ------------------------------------------------------------------------
 * Inversion of an in-plane coordinate map, the step between mesh relaxation
 * and warping.  Replaces the 2-D branch of map_utils.invert_map
 * (map_utils.py:392-463): per z slice, the valid nodes (both channels finite)
 * at their absolute positions rel + (j * stride_x + src_start_x * stride_x)
 * (same for y) are triangulated (Delaunay) and the source coordinates
 * trunc((j + src_start_x) * stride_x), trunc((i + src_start_y) * stride_y)
 * are interpolated linearly at the queries (trunc(u * stride_x),
 * trunc(v * stride_y)) of the output lattice; the result is made relative by
 * subtracting (u * stride_x, v * stride_y).  Queries outside the convex hull,
 * slices with fewer than 3 valid or only collinear nodes: NaN.  All arithmetic
 * in double; combinatorial decisions use exact predicates.  The triangulation
 * is verified on the device; status[z] is 0 for an answered slice, otherwise
 * an OR of SFM_INVMAP_* reasons and the slice's output must not be used.
 * At most 2^21 nodes per slice and 7936 nodes of the boundary set (valid
 * nodes that are not interior vertices of the full-quad lattice part).
 * ---------------------------------------------------------------------- */
#define SFM_INVMAP_FOLD 1           /* a full quad is folded or degenerate     */
#define SFM_INVMAP_NOT_DELAUNAY 2   /* an edge is not locally Delaunay         */
#define SFM_INVMAP_BOUNDARY_CAP 4   /* more than 7936 boundary nodes           */
#define SFM_INVMAP_CAPACITY 8       /* completion tables overflowed            */
#define SFM_INVMAP_OVERLAP 16       /* an edge has two triangles on one side   */
#define SFM_INVMAP_HULL 32          /* a border edge is not on the convex hull */
#define SFM_INVMAP_COVER 64         /* the triangles do not tile the hull once */
#define SFM_INVMAP_UNUSED 128       /* a valid node is not a vertex            */

typedef struct SfmInvertMapDesc {
  int32_t shape[3];             /* z, y, x of coord_map                      */
  int32_t dst_shape[2];         /* y, x of the output lattice                */
  int32_t src_start[2];         /* y, x: src_box.start - dst_box.start       */
  double stride[2];             /* y, x, finite and > 0                      */
  const double* coord_map;      /* device [2, z, y, x], relative format      */
  int32_t* status;              /* device [z], caller-owned, written         */
  void* workspace;              /* sfm_invert_map_workspace_bytes()          */
  size_t workspace_bytes;
  void* stream;
} SfmInvertMapDesc;

/* Host arithmetic only (callable without a GPU); 0 for a NULL descriptor or
 * an empty shape. */
size_t sfm_invert_map_workspace_bytes(const SfmInvertMapDesc* desc);
/* out: device double [2, z, dst y, dst x]; must not overlap coord_map; may
 * be NULL when the output lattice is empty (status is still written).
 * Asynchronous: read status after the stream has finished. */
int sfm_invert_map(const SfmInvertMapDesc* desc, double* out);

/* ------------------------------------------------------------------------
 * Resampling of an in-plane coordinate map (or a flow) onto another lattice,
 * the upsampling between two flow resolutions.  Replaces the linear branch of
 * map_utils.resample_map (map_utils.py:490-546) on the engine of
 * sfm_invert_map: per z slice, the nodes whose channel 0 is finite, at
 * ((j + src_start_x) * src_stride, (i + src_start_y) * src_stride), are
 * triangulated (Delaunay, exact predicates, ties broken in node-index order:
 * a full lattice quad is split from (i, j + 1) to (i + 1, j)) and both
 * channels are interpolated linearly, l0 * v0 + l1 * v1 + l2 * v2 in double,
 * at the queries ((u + dst_start_x) * dst_stride, (w + dst_start_y) *
 * dst_stride).  The result is the interpolant of ONE Delaunay triangulation
 * of the valid nodes: equal to any other's wherever all Delaunay
 * triangulations agree, one of their values elsewhere.  Queries outside the
 * convex hull, slices with fewer than 3 valid or only collinear nodes: NaN.  A
 * NaN in channel 1 of a valid node propagates.  status[z] and the limits are
 * those of sfm_invert_map (SFM_INVMAP_*); a lattice cannot fold.
 * ---------------------------------------------------------------------- */
typedef struct SfmResampleMapDesc {
  int32_t shape[3];             /* z, y, x of coord_map                      */
  int32_t dst_shape[2];         /* y, x of the output lattice                */
  int32_t src_start[2];         /* y, x of src_box.start                     */
  int32_t dst_start[2];         /* y, x of dst_box.start                     */
  double src_stride;            /* finite and > 0                            */
  double dst_stride;            /* finite and > 0                            */
  int32_t f64;                  /* coord_map and out are double, else float  */
  const void* coord_map;        /* device [2, z, y, x]                       */
  int32_t* status;              /* device [z], caller-owned, written         */
  void* workspace;              /* sfm_resample_map_workspace_bytes()        */
  size_t workspace_bytes;
  void* stream;
} SfmResampleMapDesc;

/* Host arithmetic only (callable without a GPU); 0 for a NULL descriptor or
 * an empty shape. */
size_t sfm_resample_map_workspace_bytes(const SfmResampleMapDesc* desc);
/* out: device [2, z, dst y, dst x] of coord_map's type; must not overlap
 * coord_map; may be NULL when the output lattice is empty (status is still
 * written).  Asynchronous: read status after the stream has finished. */
int sfm_resample_map(const SfmResampleMapDesc* desc, void* out);

/* ------------------------------------------------------------------------
 * Composition of two in-plane coordinate maps through a triangulation, the
 * step of the cross-block reconcile.  Replaces map_utils.compose_maps
 * (map_utils.py:549-611) on the engine of sfm_invert_map (sfm_compose_maps is
 * the lattice sampler of compose_maps_fast).  Per z slice the nodes of map2
 * where both channels of its absolute form are finite, at
 * ((j + start2_x) * stride2, (i + start2_y) * stride2), are triangulated as in
 * sfm_resample_map.  Node (w, u) of map1 asks at its absolute position
 * T1(rel + (u * stride1 + start1_x * stride1)) (same for y); a node with a
 * channel that is not finite gives NaN in both outputs.  A query is answered
 * by the lowest-keyed triangle whose closed exact test contains it (lattice
 * triangles first), so shared edges and vertices are deterministic.  The
 * values are map2's absolute form T2(rel [* T2(scale2[z])] + (j * stride2 +
 * start2_x * stride2)), interpolated in double; the result is rounded to T1
 * and then made relative in T1: T1(double(r) - (u * stride1 + start1_x *
 * stride1)).  T1 / T2 are float or double (f64_1 / f64_2).  map2 may have one
 * z slice that serves every slice of map1: it is triangulated once, and
 * scale2 (validity does not look at it) gives each slice of map1 its own
 * factor.  Queries outside the convex hull, slices with fewer than 3 valid or
 * only collinear nodes: NaN.  status[z2] and the limits are those of
 * sfm_invert_map (SFM_INVMAP_*), per slice of map2.
 * ---------------------------------------------------------------------- */
typedef struct SfmComposeTriDesc {
  int32_t shape1[3];            /* z, y, x of map1 and of out                */
  int32_t shape2[3];            /* z, y, x of map2; z is 1 or shape1[0]      */
  int32_t start1[2];            /* y, x of box1.start                        */
  int32_t start2[2];            /* y, x of box2.start                        */
  double stride1;               /* finite and > 0                            */
  double stride2;               /* finite and > 0                            */
  int32_t f64_1;                /* map1 and out are double, else float       */
  int32_t f64_2;                /* map2 is double, else float                */
  const void* map1;             /* device [2, z, y, x], relative format      */
  const void* map2;             /* device [2, z or 1, y2, x2], relative      */
  const double* scale2;         /* device [shape1[0]] or NULL                */
  int32_t* status;              /* device [shape2[0]], caller-owned, written */
  void* workspace;              /* sfm_compose_maps_tri_workspace_bytes()    */
  size_t workspace_bytes;
  void* stream;
} SfmComposeTriDesc;

/* Host arithmetic only (callable without a GPU); 0 for a NULL descriptor or
 * an empty shape. */
size_t sfm_compose_maps_tri_workspace_bytes(const SfmComposeTriDesc* desc);
/* out: device [2, z, y, x] of map1's shape and type; must not overlap the
 * maps.  Asynchronous: read status after the stream has finished. */
int sfm_compose_maps_tri(const SfmComposeTriDesc* desc, void* out);

/* ------------------------------------------------------------------------
 * Fold / stretch detection on a relaxed mesh, the step after relaxation.
 * Replaces map_utils.mask_irregular (map_utils.py:737-786): a node is bad when
 * the distance to its +x (+y) neighbour leaves [min_dist, max_dist]; the bad
 * set is dilated `dilation_iters` times with the full 3 x 3 structure and the
 * map is NaN'ed there in place.  The neighbour difference is taken in float32
 * (np.diff of a float32 map); the stride is added and the sum compared with
 * the limits in double, as NumPy >= 2 does with a float64 stride scalar.  The
 * caller forms the limits (frac * stride, max_frac * stride) in double.
 * ---------------------------------------------------------------------- */
typedef struct SfmMaskIrregularDesc {
  int32_t shape[2];             /* y, x                                      */
  int32_t dilation_iters;
  double stride[2];             /* x, y (the reference's order)              */
  double min_dist[2];           /* x, y: frac * stride                       */
  double max_dist[2];           /* x, y: max_frac * stride                   */
  void* stream;
} SfmMaskIrregularDesc;

/* coord_map: device float [2, y, x], modified in place; bad: device uint8
 * [y, x] (1 = masked). */
int sfm_mask_irregular(const SfmMaskIrregularDesc* desc, float* coord_map,
                       uint8_t* bad);
/* The same test on a float64 map, not narrowed: the neighbour difference is
 * taken in double, as np.diff does for a float64 map.  coord_map: device double
 * [2, y, x], modified in place.  n_valid: device int32, written: the number of
 * nodes that keep a component that is not NaN (0 <=> np.all(np.isnan(map))). */
int sfm_mask_irregular_f64(const SfmMaskIrregularDesc* desc, double* coord_map,
                           uint8_t* bad, int32_t* n_valid);

/* ------------------------------------------------------------------------
 * Reference positions of one section from several flows at once.
 * Replaces the compute part of RelaxMesh.get_prev_state with compute_ref_mesh
 * and compute_ref_mesh_multiz (processor/mesh.py:170-371): every flow is
 * composed with the solved mesh of the section it was measured against
 * (map_utils.compose_maps_fast, mode nearest, both maps at the same box start)
 * and the composed vectors are averaged per node over the flows that gave a
 * finite x component.  A 2-channel flow has one reference section.  A
 * 3-channel flow picks its reference per node: channel 2 is compared for exact
 * equality with delta_z[k]; a node that matches no entry (NaN, 0, a fraction,
 * a section of another block) contributes NaN.  Sums are kept in double:
 * NaN adds 0, +-inf adds +-FLT_MAX (2 channels: np.nan_to_num of the float32
 * composed map) or +-DBL_MAX (3 channels: of the float64 array the reference
 * collects the vectors in); a node without a finite vector is NaN.
 * Which flows and sections take part is host logic
 * (sofima_amd.processor_mesh.refs_for_section).
 * ---------------------------------------------------------------------- */
#define SFM_PREV_MAX_FLOWS 8
#define SFM_PREV_MAX_REFS 16

typedef struct SfmPrevFlow {
  int32_t channels;             /* 2 or 3                                    */
  int32_t n_refs;               /* 2 channels: 1; 3 channels: 0 to 16        */
  const float* flow;            /* device, channel c at flow + c * flow_channel_stride, each [y, x] */
  int64_t flow_channel_stride;  /* elements, >= y * x                        */
  int64_t mesh_channel_stride;  /* elements between the x and y plane of a mesh[k] */
  int32_t delta_z[SFM_PREV_MAX_REFS];   /* 3 channels: look-back offsets, none 0 */
  const float* mesh[SFM_PREV_MAX_REFS]; /* device: x plane [y, x] of section z - delta_z[k] */
} SfmPrevFlow;

typedef struct SfmPrevStateDesc {
  int32_t shape[2];             /* y, x                                      */
  int32_t n_flows;              /* 1 to 8, averaged in this order            */
  float stride[2];              /* y, x: compose_maps_fast's stride          */
  SfmPrevFlow flows[SFM_PREV_MAX_FLOWS];
  void* stream;
} SfmPrevStateDesc;

/* out: device double [2, y, x]; must not overlap any input. */
int sfm_prev_state(const SfmPrevStateDesc* desc, double* out);

/* ------------------------------------------------------------------------
 * Warping one image section by an inverse coordinate map.
 * Replaces the per-section body of warp.warp_subvolume (warp.py:145-167):
 * linear (extrapolating) interpolation of the map nodes to every output
 * pixel, cv2.convertMaps to 1/32-pixel fixed point, cv2.remap with a zero
 * border -- fused, one pass over the output.
 * ---------------------------------------------------------------------- */
#define SFM_WARP_NEAREST 0
#define SFM_WARP_TABLE 1         /* taps weighted by `weights` (linear, cubic,
                                    lanczos4 differ only in the table)        */
typedef struct SfmWarpDesc {
  int32_t dtype;                /* SFM_DTYPE_* of image and out              */
  int32_t interpolation;        /* SFM_WARP_*                                */
  int32_t ksize;                /* taps per axis: 2, 4 or 8                  */
  int32_t image_shape[2];       /* y, x                                      */
  int32_t map_shape[2];         /* y, x nodes (>= 2 x 2)                     */
  int32_t out_shape[2];         /* y, x                                      */
  double map_origin[2];         /* y, x of map node (0, 0) in output pixels  */
  double stride;                /* output pixels per map node                */
  const void* image;            /* device [y, x]                             */
  const void* coord_map;        /* device [2, y, x]: ABSOLUTE source (x, y)
                                   coordinates in image pixels, float32 (or
                                   float64 when coord_map_f64 is set: the
                                   reference interpolates in the map's dtype,
                                   warp.py:125-150)                          */
  const void* weights;          /* device [32 * 32, ksize * ksize]: int16 with
                                   15 fractional bits for u8 images, float
                                   otherwise; phase = 32 * fy + fx            */
  void* out;                    /* device [y, x]                             */
  void* stream;
  int32_t coord_map_f64;        /* 1: coord_map holds doubles                */
} SfmWarpDesc;

int sfm_warp_section(const SfmWarpDesc* desc);

/* ------------------------------------------------------------------------
 * warp.ndimage_warp (warp.py:189-335), the SciPy rendering path, 2-D and 3-D,
 * as ONE kernel: per output voxel the node-space position (c - offset) / stride,
 * the order-1 interpolation of the absolute source map (scipy.ndimage.
 * map_coordinates, mode "constant", cval 0: a position outside the node grid
 * gives the dense coordinate 0, like the reference), and the order-0 / order-1
 * sampling of the image at the dense coordinates, all in double like SciPy and
 * in SciPy's operation order (weights 1 - t and 1 - (1 - t), value x weights in
 * axis order, taps added in row-major order), so integer images come out bit
 * for bit and float images to the last bit.  The work-box decomposition of the
 * reference (work_size / overlap) does not change the result for these orders
 * and has no counterpart here.  Axes are z, y, x; 2-D inputs use y, x of the
 * last two entries with shape[0] = 1.
 * ---------------------------------------------------------------------- */
typedef struct SfmNdWarpDesc {
  int32_t ndim;                 /* 2 or 3                                      */
  int32_t dtype;                /* SFM_DTYPE_U8 | U16 | F32 of image and out   */
  int32_t order;                /* 0 nearest, 1 linear                         */
  int32_t image_shape[3];       /* z, y, x                                     */
  int32_t map_shape[3];         /* z, y, x nodes                               */
  int32_t out_shape[3];         /* z, y, x                                     */
  double stride[3];             /* z, y, x output voxels per map node          */
  double offset[3];             /* z, y, x of map node 0 relative to out voxel 0 */
  const void* image;            /* device [z, y, x]                            */
  const double* src_map;        /* device [ndim, z, y, x] float64, channels x,
                                   y[, z]: absolute source coordinates in image
                                   voxels (warp.py:250-265)                    */
  void* out;                    /* device [z, y, x]                            */
  void* stream;
} SfmNdWarpDesc;

int sfm_ndimage_warp(const SfmNdWarpDesc* desc);

/* ------------------------------------------------------------------------
 * processor/warp.py: StitchAndRender3dTiles.process (:292-343), the warp-and-
 * blend loop of a 3-D tile montage, as ONE kernel per output box.  Every output
 * voxel walks the request's tile table in ascending order; for a tile whose
 * sub_box holds it the voxel computes, as warp.ndimage_warp does (see above),
 * the node-space position and the three dense source coordinates ONCE, samples
 * the image region data_box (order 0 / 1, converted to the tile dtype as SciPy
 * does) and the tile's 2-D blend weights repeated along z (order 1, narrowed to
 * float32), and accumulates img += float32(image) * w, norm += w in float32.
 * Where norm > 0 the voxel is the IEEE float32 quotient img / norm, elsewhere
 * img (0 where no tile reaches); the result is cast by truncation and stored
 * once.  The absolute source map of a (tile, request) pair is read as
 * abs_map + shift: abs_map is the tile's float64 inverse map plus node index x
 * stride (sfm_map_shift, SFM_SHIFT_TO_ABSOLUTE, no box) and shift the scalar
 * tg_box.start * stride - data_box.start per channel, the two sums of
 * warp.py:249-258 in their order.
 * ---------------------------------------------------------------------- */
typedef struct SfmRenderTile {
  const void* image;            /* device [z, y, x]: the WHOLE tile            */
  const double* abs_map;        /* device [3, z, y, x] float64, channels x, y, z */
  const float* weights;         /* device [y, x] float32 of the whole tile     */
  int32_t tile_shape[3];        /* z, y, x of image (y, x of weights)          */
  int32_t map_shape[3];         /* z, y, x nodes                               */
  int32_t data_start[3];        /* z, y, x of data_box within the tile         */
  int32_t data_size[3];         /* z, y, x of data_box                         */
  int32_t sub_start[3];         /* z, y, x of sub_box within the output box    */
  int32_t sub_size[3];          /* z, y, x of sub_box                          */
  double shift[3];              /* per channel x, y, z: added to abs_map       */
  double offset[3];             /* z, y, x of map node 0 relative to voxel 0 of
                                   sub_box (warp.py:288)                       */
} SfmRenderTile;

typedef struct SfmRenderTilesDesc {
  int32_t dtype;                /* SFM_DTYPE_U8 | U16 | F32 of the tiles       */
  int32_t out_dtype;            /* dtype, or SFM_DTYPE_F32                     */
  int32_t order;                /* image sampling: 0 nearest, 1 linear         */
  int32_t n_tiles;              /* entries of the table, >= 0                  */
  int32_t out_shape[3];         /* z, y, x of the output box                   */
  double stride[3];             /* z, y, x output voxels per map node          */
  const SfmRenderTile* tiles_host;  /* host copy of the table: every box is
                                   checked against its array before the launch */
  const SfmRenderTile* tiles;   /* device copy of the same table, read by the
                                   kernel (NULL allowed when n_tiles is 0)     */
  void* out;                    /* device [z, y, x] of out_dtype, all written  */
  void* stream;
} SfmRenderTilesDesc;

int sfm_render_tiles3d(const SfmRenderTilesDesc* desc);

/* ------------------------------------------------------------------------
 * Spline orders 2 .. 5 of the two calls above (sfm_spline.hip, sfm_ndwarp_kernel.h).
 * SciPy samples orders above 1 from B-spline coefficients, not from the image:
 * scipy.ndimage.spline_filter(image, order, output=float64, mode="constant"),
 * a recursive filter along axis 0, then 1, then 2, each pass on the previous
 * pass's output, mirror boundaries, axes of length 1 skipped.
 * sfm_spline_prefilter computes these coefficients for a table of arrays (or
 * regions of arrays) in one batch of launches: plain double arithmetic in
 * SciPy's operation order, one thread per line (a line's recursion is not
 * split: that would change the rounding), the x pass staged through LDS.  The
 * poles are SciPy's literals and live in the library; pow(pole, len - 1) of
 * the mirror initialisation is NOT computed on the device, whose pow is not
 * libm's: the caller fills `zn` with the host's libm.
 * ---------------------------------------------------------------------- */
typedef struct SfmSplineItem {
  const void* image;            /* device: first element of the region         */
  int64_t pitch[3];             /* z, y, x element distance within image       */
  int64_t coeff_offset;         /* element offset within coeffs of this item's
                                   dense [shape] float64 coefficients          */
  int32_t shape[3];             /* z, y, x of the region; 2-D: shape[0] = 1    */
  int32_t reserved;             /* 0                                           */
  double zn[3][2];              /* pow(pole p, shape[k] - 1) per axis k and
                                   pole p (order 2, 3: p = 0 only), host libm  */
} SfmSplineItem;

typedef struct SfmSplinePrefilterDesc {
  int32_t dtype;                /* SFM_DTYPE_U8 | U16 | F32 of every image     */
  int32_t order;                /* 2 .. 5                                      */
  int32_t n_items;              /* entries of the table, >= 0                  */
  int32_t reserved;             /* 0                                           */
  const SfmSplineItem* items_host;  /* host copy of the table, checked here    */
  const SfmSplineItem* items;   /* device copy of the same table               */
  double* coeffs;               /* device, caller-owned: coeffs_len doubles    */
  int64_t coeffs_len;           /* every item lies inside [0, coeffs_len)      */
  void* stream;
} SfmSplinePrefilterDesc;

int sfm_spline_prefilter(const SfmSplinePrefilterDesc* desc);

/* sfm_ndimage_warp with order 2 .. 5: desc->image holds the float64 B-spline
 * coefficients of the image (dense, image_shape), desc->dtype is the type of
 * `out` alone.  The dense coordinates stay order 1. */
int sfm_ndimage_warp_spline(const SfmNdWarpDesc* desc);

/* sfm_render_tiles3d with order 2 .. 5 for the image (the weights stay order
 * 1).  The reference warps each tile's data_box CROP, so the spline is that of
 * the crop, mirrored at the crop's edges: `coeffs` holds the float64
 * coefficients of the data_box regions of all table entries, each dense in its
 * data_size, back to back in table order (sfm_spline_prefilter with one item
 * per entry); `image` of an entry is not read. */
int sfm_render_tiles3d_spline(const SfmRenderTilesDesc* desc, const double* coeffs);

/* ------------------------------------------------------------------------
 * SciPy's boundary modes and fill value for the samplers (sfm_ndsample.h), as
 * scipy.ndimage.map_coordinates(mode=, cval=) applies them: restated from
 * SciPy's behaviour in tests/ndwarp_modes_ref.py, which a CPU test pins to SciPy
 * bit for bit.  Orders 0 and 1 take every mode; orders 2 .. 5 take CONSTANT,
 * MIRROR and WRAP, whose B-spline coefficients are those of
 * sfm_spline_prefilter; the others need another prefilter and are rejected,
 * unless the switch SFM_SPLINE_MODES is on: see sfm_spline_prefilter_mode below.
 * An integer image takes cval through the conversion of a sampled value and
 * needs a finite one.  A NaN coordinate, or one of magnitude 2^31 and above,
 * gives cval under every mode (SciPy casts it to an integer there, which is
 * undefined, except under CONSTANT); no coordinate reads outside the array.
 * ---------------------------------------------------------------------- */
#define SFM_MODE_CONSTANT 0        /* outside [0, len - 1]: cval                 */
#define SFM_MODE_GRID_CONSTANT 1   /* taps outside the array read cval           */
#define SFM_MODE_NEAREST 2         /* taps clamped to the edge sample            */
#define SFM_MODE_MIRROR 3          /* period 2 len - 2                           */
#define SFM_MODE_REFLECT 4         /* period 2 len ("grid-mirror")               */
#define SFM_MODE_WRAP 5            /* period len - 1                             */
#define SFM_MODE_GRID_WRAP 6       /* period len                                 */

/* sfm_ndimage_warp / sfm_ndimage_warp_spline (by desc->order: 2 .. 5 read
 * coefficients from desc->image) with a boundary mode on BOTH steps, as the
 * reference passes one map_coordinates callable to both (warp.py:308-314):
 * outside the node grid the dense coordinate is cval, in source voxels, or the
 * folded node value, and the image sample follows the same rule. */
int sfm_ndimage_warp_mode(const SfmNdWarpDesc* desc, int32_t mode, double cval);

/* scipy.ndimage.affine_transform(image, matrix, offset, order=, mode=, cval=)
 * with a [dim, dim] matrix, output of the input's shape, as ONE kernel and
 * without a coordinate map: per output voxel o the source coordinate
 *   c[h] = ((0 + o[0] M[h][0]) + o[1] M[h][1] [+ o[2] M[h][2]]) + offset[h]
 * in double and in this order (SciPy's, offset last), then the samplers. */
typedef struct SfmAffineWarpDesc {
  int32_t ndim;                 /* 2 or 3                                      */
  int32_t dtype;                /* SFM_DTYPE_U8 | U16 | F32 of image and out   */
  int32_t order;                /* 0 .. 5; 2 .. 5: image holds the float64
                                   B-spline coefficients (sfm_spline_prefilter),
                                   dtype is the type of out alone              */
  int32_t mode;                 /* SFM_MODE_*                                  */
  int32_t shape[3];             /* z, y, x of image and out; 2-D: shape[0] = 1 */
  int32_t reserved;             /* 0                                           */
  double matrix[9];             /* row-major [3][3] over the axes z, y, x; 2-D
                                   reads rows and columns 1 and 2              */
  double offset[3];             /* z, y, x                                     */
  double cval;
  const void* image;            /* device [z, y, x]                            */
  void* out;                    /* device [z, y, x]                            */
  void* stream;
} SfmAffineWarpDesc;

int sfm_affine_warp(const SfmAffineWarpDesc* desc);

/* sfm_ndimage_warp, _spline and _mode on the RELATIVE coordinate map, float32 or
 * float64, as the map functions of this library leave it on the device: no
 * absolute float64 copy is prepared.  Every node a tap reads becomes the absolute
 * source coordinate in registers, with the roundings of the reference's NumPy
 * statements (warp.py:249-262).  For channel c (x, y[, z]; its axis is
 * ndim - 1 - c), node index n along that axis and map type M:
 *   v = (double)(M)((double)rel[c][node] + (double)n * stride[axis])
 *   v = (double)(M)(v + shift[c])         only if has_shift: a map_box was given
 *   v = v * scale[c]
 * n * stride is one rounded double product.  The rest is sfm_ndimage_warp: the
 * same kernels with another map accessor, bit for bit the result of the absolute
 * entries on the map those statements produce.  order 0 .. 5 (2 .. 5: `image`
 * holds the float64 B-spline coefficients, dtype is the type of `out` alone);
 * the boundary fields are read only if has_boundary, as sfm_ndimage_warp_mode
 * reads its arguments. */
typedef struct SfmNdWarpRelDesc {
  int32_t ndim;                 /* 2 or 3                                      */
  int32_t dtype;                /* SFM_DTYPE_U8 | U16 | F32 of image and out   */
  int32_t order;                /* 0 .. 5                                      */
  int32_t image_shape[3];       /* z, y, x                                     */
  int32_t map_shape[3];         /* z, y, x nodes                               */
  int32_t out_shape[3];         /* z, y, x                                     */
  double stride[3];             /* z, y, x output voxels per map node          */
  double offset[3];             /* z, y, x of map node 0 relative to out voxel 0 */
  double shift[3];              /* per channel x, y, z: map_box.start[c] *
                                   stride of the channel's axis -
                                   image_box.start[c] / out_scale[c]           */
  double scale[3];              /* per channel x, y, z: out_scale              */
  double cval;                  /* fill value, if has_boundary                 */
  int32_t map_f64;              /* 0: rel_map is float32, else float64         */
  int32_t has_shift;            /* 0: the shift is not added at all            */
  int32_t has_boundary;         /* 0: mode "constant", cval 0                  */
  int32_t mode;                 /* SFM_MODE_*, if has_boundary                 */
  const void* image;            /* device [z, y, x]                            */
  const void* rel_map;          /* device [ndim, z, y, x], channels x, y[, z]:
                                   relative coordinates                        */
  void* out;                    /* device [z, y, x]                            */
  void* stream;
} SfmNdWarpRelDesc;

int sfm_ndimage_warp_rel(const SfmNdWarpRelDesc* desc);

/* ------------------------------------------------------------------------
 * Orders 2 .. 5 under SciPy's remaining boundary modes: NEAREST, REFLECT
 * ("grid-mirror"), GRID_CONSTANT and GRID_WRAP.  Opt-in: the switch
 * SFM_SPLINE_MODES=1 (sfm_set_option, or the environment variable as the
 * default); without it every call below and above rejects these modes at these
 * orders as before.  The switch lifts the mode restriction only; callers that
 * gate the orders themselves (the Python layer: SFM_SPLINE_ORDERS) still do.
 *
 * scipy.ndimage.spline_filter initialises its recursion in one of three ways:
 * mirror for MIRROR, CONSTANT, GRID_CONSTANT and WRAP (sfm_spline_prefilter),
 * reflect for REFLECT and NEAREST, wrap for GRID_WRAP alone.  And
 * map_coordinates / affine_transform pad the image by 12 samples on every axis
 * the array has before they filter for NEAREST (edge values) and GRID_CONSTANT
 * (cval, cast to the image's type), and sample the padded coefficients at
 * coordinate + 12 under the same mode.  sfm_spline_mode_pad returns that pad for
 * a mode: 12 or 0 (-1: no such mode).
 *
 * sfm_spline_prefilter_mode is sfm_spline_prefilter with the initialisation and
 * the pad of `mode`.  `ndim` is the real dimensionality of every item (2:
 * shape[0] = 1, and that axis is not padded; a real axis of length 1 IS padded
 * and filtered).  With a pad p the coefficients of an item are dense in
 * shape + 2p on its real axes -- coeff_offset and coeffs_len count those -- while
 * `shape` and `pitch` stay those of the source region, which is read through a
 * clamped index (NEAREST), or replaced by `pad_value` outside it (GRID_CONSTANT;
 * the value as the image's type holds it, the caller converts; ignored by the
 * other modes): no padded copy of the image exists.  SfmSplineItem.zn holds, per
 * axis k of the coefficients' length n and pole p, pow(pole, n - 1) for the
 * mirror initialisation and pow(pole, n) for the reflect one; the wrap one
 * reads none.  CONSTANT, MIRROR and WRAP are sfm_spline_prefilter itself.
 *
 * With the switch on, sfm_ndimage_warp_mode, sfm_ndimage_warp_rel (has_boundary)
 * and sfm_affine_warp accept the four modes at orders 2 .. 5.  `image` then
 * holds the coefficients of sfm_spline_prefilter_mode for the same mode and
 * ndim; image_shape / shape stays the shape of the image itself: for NEAREST and
 * GRID_CONSTANT the library adds the 12 to the image-step coordinate, in double
 * (after the offset in sfm_affine_warp; the map step of sfm_ndimage_warp is order
 * 1 and unpadded), and samples with the padded shape.
 * ---------------------------------------------------------------------- */
int sfm_spline_mode_pad(int32_t mode);
int sfm_spline_prefilter_mode(const SfmSplinePrefilterDesc* desc, int32_t mode, int32_t ndim,
                              double pad_value);

/* ------------------------------------------------------------------------
 * Map geometry: the one-pass helpers that the reference's renderers call
 * around invert_map and the warps (sfm_mapgeom.hip).  Maps are [ncomp, z, y,
 * x] with channels x, y[, z], float32 or float64 (`f64`).  Arithmetic is the
 * reference's NumPy arithmetic: offsets are formed in double, added to the
 * widened element, and the sum is narrowed once to the map's type.
 * ---------------------------------------------------------------------- */
#define SFM_SHIFT_TO_ABSOLUTE 0
#define SFM_SHIFT_TO_RELATIVE 1

/* map_utils.to_absolute / to_relative (map_utils.py:150-224):
 * out[c] = T(double(in[c]) +/- (index_c * stride_c + start_c)), index_c the
 * x / y / z node index for channel 0 / 1 / 2. */
typedef struct SfmMapShiftDesc {
  int32_t ncomp;                /* 2 or 3                                     */
  int32_t f64;                  /* 1: maps hold doubles, 0: floats            */
  int32_t direction;            /* SFM_SHIFT_*                                */
  int32_t shape[3];             /* z, y, x                                    */
  double stride[3];             /* z, y, x (entry 0 unused for ncomp 2)       */
  double start[3];              /* z, y, x: box.start * stride in double, 0
                                   without a box                              */
  const void* coord_map;        /* device [ncomp, z, y, x]                    */
  void* out;                    /* device, same shape; may equal coord_map    */
  void* stream;
} SfmMapShiftDesc;

int sfm_map_shift(const SfmMapShiftDesc* desc);

/* map_utils.outer_box / inner_box (map_utils.py:307-389): reductions over the
 * ABSOLUTE map (rounded as sfm_map_shift rounds it), which is never stored.
 *   OUTER  result[2c], result[2c + 1] = nanmin, nanmax of channel c; an
 *          all-NaN channel gives +inf, -inf.
 *   INNER  result[2a], result[2a + 1] = max over the lines along axis a of the
 *          line's min, min over the lines of the line's max, of channel a
 *          (a = 0: x, lines along x; 1: y; 2: z).  result[6] is non-zero when
 *          the map holds a NaN; the other entries are then meaningless.
 * result: 8 doubles on the device (values widened exactly from the map's
 * type), written by the last launch; deterministic.  workspace: at least
 * SFM_MAP_EXTENTS_WORKSPACE_BYTES. */
#define SFM_EXTENTS_OUTER 0
#define SFM_EXTENTS_INNER 1
#define SFM_MAP_EXTENTS_WORKSPACE_BYTES (3 * 1024 * 4 * 8)

typedef struct SfmMapExtentsDesc {
  int32_t ncomp;                /* 2 or 3                                     */
  int32_t f64;
  int32_t mode;                 /* SFM_EXTENTS_*                              */
  int32_t shape[3];             /* z, y, x                                    */
  double stride[3];             /* z, y, x                                    */
  double start[3];              /* z, y, x: box.start * stride                */
  const void* coord_map;        /* device [ncomp, z, y, x], relative format   */
  double* result;               /* device [8]                                 */
  void* workspace;
  size_t workspace_bytes;
  void* stream;
} SfmMapExtentsDesc;

int sfm_map_extents(const SfmMapExtentsDesc* desc);

/* map_utils.make_affine_map (map_utils.py:789-811):
 * p = (x * stride_x + start_x, y * stride_y + start_y, z * stride_z + start_z),
 * out[c] = ((m[c][0] p_x + m[c][1] p_y) + m[c][2] p_z) + m[c][3] - p_c, plain
 * left-to-right double arithmetic. */
typedef struct SfmAffineMapDesc {
  int32_t shape[3];             /* z, y, x nodes (box.size reversed)          */
  double stride[3];             /* z, y, x                                    */
  double start[3];              /* z, y, x: box.start (NOT times stride)      */
  double matrix[12];            /* row-major [3, 4], rows and columns x, y, z */
  double* out;                  /* device [3, z, y, x]                        */
  void* stream;
} SfmAffineMapDesc;

int sfm_affine_map(const SfmAffineMapDesc* desc);

/* warp.warp_points (warp.py:541-605): every point reads the four map nodes
 * around it in its section and combines them with bilinear weights in double
 * (linear extrapolation outside the grid), like scipy's
 * RegularGridInterpolator(bounds_error=False, fill_value=None) on the absolute
 * map.  A node is T(double(T(double(m) + index * stride)) + origin); the grid
 * coordinate of node j is (j + grid_start) * stride.  The result is narrowed to
 * float and, for integer points, rounded half to even. */
#define SFM_POINT_F32 0
#define SFM_POINT_F64 1
#define SFM_POINT_I32 2
#define SFM_POINT_I64 3

typedef struct SfmWarpPointsDesc {
  int32_t f64;                  /* type of coord_map                          */
  int32_t point_dtype;          /* SFM_POINT_* of points and out              */
  int32_t shape[3];             /* z, y, x of coord_map; y, x >= 2            */
  int64_t n;                    /* points                                     */
  double stride;                /* > 0                                        */
  double origin[2];             /* x, y: map_box.start * stride               */
  int64_t grid_start[2];        /* x, y: map_box.start                        */
  const void* coord_map;        /* device [2, z, y, x], relative format       */
  const void* points;           /* device [n, 3], xyz                         */
  const int32_t* section;       /* device [n]: section of every point, in
                                   [0, z); other values give NaN / 0           */
  void* out;                    /* device [n, 3]; columns x and y are written */
  void* stream;
} SfmWarpPointsDesc;

int sfm_warp_points(const SfmWarpPointsDesc* desc);

/* map_utils.fill_missing (map_utils.py:227-304), the branch without Delaunay
 * interpolation (interpolate_first=False).  A node is valid when all its
 * channels are finite.  A 2-channel map is filled per z slice, a 3-channel map
 * as one volume ("problem" below).  out is written as follows:
 *   - the map holds no NaN: out = coord_map (inf entries stay);
 *   - a problem without a valid node: zeros with invalid_to_zero, else NaN
 *     (quiet, positive, zero payload) with extrapolate, else unchanged;
 *   - otherwise, with extrapolate, every invalid node gets in all channels the
 *     bits of the valid node at the smallest squared Euclidean distance in node
 *     indices (isotropic; z counts for 3 channels only), the lowest C-order
 *     index of [z, y, x] among equidistant ones; valid nodes keep their bits.
 *     Without extrapolate the problem is copied.
 * Distances are exact 32-bit integers: every axis holds at most
 * SFM_FILL_MISSING_MAX_AXIS nodes and the map at most 2^31 - 1 nodes per
 * channel (SFM_ERR_INVALID above either).  has_nan receives non-zero when the
 * map holds a NaN.  Deterministic; coord_map is only read and must not overlap
 * out. */
#define SFM_FILL_MISSING_MAX_AXIS 16384

typedef struct SfmFillMissingDesc {
  int32_t ncomp;                /* 2: per z slice, 3: one volume              */
  int32_t f64;                  /* 1: the maps hold doubles, 0: floats        */
  int32_t shape[3];             /* z, y, x                                    */
  int32_t invalid_to_zero;
  int32_t extrapolate;
  const void* coord_map;        /* device [ncomp, z, y, x]                    */
  void* out;                    /* device, same shape and type                */
  int32_t* has_nan;             /* device [1]                                 */
  void* workspace;              /* sfm_fill_missing_nearest_workspace_bytes() */
  size_t workspace_bytes;
  void* stream;
} SfmFillMissingDesc;

/* 0 for a NULL or unacceptable descriptor (only ncomp and shape are read). */
size_t sfm_fill_missing_nearest_workspace_bytes(const SfmFillMissingDesc* desc);
int sfm_fill_missing_nearest(const SfmFillMissingDesc* desc);

/* ------------------------------------------------------------------------
 * Dynamic-range mask of an overlap strip, the step in front of the
 * whole-overlap correlation of a tile pair.
 * Replaces the mask construction of stitch_rigid._estimate_offset
 * (stitch_rigid.py:47-60): out = (maximum_filter(img, size) -
 * minimum_filter(img, size)) < range_limit, OR-ed with `extra_mask`
 * (scipy.ndimage filters: mode "reflect", window [i - size/2, i - size/2 +
 * size - 1]; uint8 images subtract in uint8).
 * ---------------------------------------------------------------------- */
typedef struct SfmRangeMaskDesc {
  int32_t dtype;                /* SFM_DTYPE_* of the image                  */
  int32_t shape[2];             /* y, x                                      */
  int32_t filter_size;
  double range_limit;
  const void* image;            /* device [y, x]                             */
  const uint8_t* extra_mask;    /* device bool bytes [y, x] or NULL          */
  void* stream;
} SfmRangeMaskDesc;

/* out: device uint8 [y, x] (1 = masked). */
int sfm_range_mask(const SfmRangeMaskDesc* desc, uint8_t* out);

/* ------------------------------------------------------------------------
 * Target mesh of an elastic tile montage.
 * Replaces stitch_elastic.compute_target_mesh (stitch_elastic.py:624-676,
 * with _update_mesh :573-620 and _apply_flow :456-570) vmapped over all
 * tiles: out[:, t] = positions in the meshes of tile t's neighbours that the
 * flow fields say its nodes correspond to; NaN where no neighbour overlaps.
 * ---------------------------------------------------------------------- */
typedef struct SfmTargetMeshDesc {
  int32_t ncomp;                /* 2 (in-plane montage) or 3 (volumetric)    */
  int32_t n_tiles;
  int32_t mesh_shape[3];        /* z, y, x of one tile mesh (z = 1 for 2)    */
  int32_t fx_shape[3];          /* z, y, x of one flow array in fx           */
  int32_t fy_shape[3];
  int32_t n_fx;                 /* flow arrays in fx (its dimension 1)       */
  int32_t n_fy;
  int32_t nbor_fields;          /* 8, or 11 with the z fields (ncomp 3)      */
  float stride[3];              /* zyx stride of flow and mesh               */
  const int32_t* nbors;         /* device [n_tiles, 4, nbor_fields]          */
  const float* fx;              /* device [ncomp, n_fx, *fx_shape]           */
  const float* fy;              /* device [ncomp, n_fy, *fy_shape]           */
  int32_t n_eval;               /* 0: all tiles; > 0: only the first n_eval
                                   rows of `nbors` are evaluated (the meshes in
                                   x still number n_tiles)                   */
} SfmTargetMeshDesc;

/* x: device float [ncomp, n_tiles, *mesh_shape]; out: [ncomp, n_eval or
 * n_tiles, *mesh_shape]. */
int sfm_target_mesh(const SfmTargetMeshDesc* desc, const float* x, float* out,
                    void* stream);

/* ------------------------------------------------------------------------
 * Spring mesh.
 * ---------------------------------------------------------------------- */
#define SFM_MESH_MAX_LINKS 13

/* Which mesh_force the integrator evaluates (the `mesh_force` argument of
 * mesh.relax_mesh / velocity_verlet, mesh.py:372-382). */
#define SFM_FORCE_SPRINGS 0    /* inplane_force / elastic_mesh_3d link stencils  */
#define SFM_FORCE_TILE_MESH 1  /* stitch_rigid.elastic_tile_mesh (stitch_rigid.py:
                                  330-388) for ncomp 2, elastic_tile_mesh_3d
                                  (:391-473) for ncomp 3: every node is a tile,
                                  cx / cy are the desired offsets to the +x / +y
                                  tile, force = displacement mismatch          */
#define SFM_FORCE_EXTERNAL 2   /* produced by the caller through force_cb        */

/* SFM_FORCE_EXTERNAL: called on the host before every force evaluation (once
 * for the initial a = F(x), then once per step after the position update).
 * It must enqueue, on SfmMeshDesc.stream, work that leaves mesh_force(x) in
 * SfmMeshDesc.ext_force.  Non-zero return aborts the chunk with SFM_ERR_INVALID. */
typedef int (*SfmForceCallback)(void* user);

typedef struct SfmMeshDesc {
  int32_t ncomp;                /* 2: inplane_force (mesh.py:42-169)
                                   3: elastic_mesh_3d (mesh.py:192-279)      */
  int32_t shape[4];             /* batch, z, y, x  (ncomp 2: batch = 1 and z
                                   slices are independent)                   */
  /* Configuration scalars are doubles so that host-side constant folding
     matches the reference's Python-float arithmetic before rounding to f32. */
  double stride[3];             /* x, y[, z] node spacing                    */
  double k;                     /* intra-mesh spring constant                */
  double k0;                    /* spring constant to `prev`                 */
  int32_t prefer_orig_order;
  int32_t n_links;              /* ncomp 3 only; 0 = the 13 default links    */
  int32_t links[SFM_MESH_MAX_LINKS][3];  /* xyz directions, |v| <= 1         */
  /* integrator (mesh.IntegrationConfig, mesh.py:282-338) */
  double dt;
  double gamma;
  int32_t num_iters;
  int32_t fire;
  double f_alpha, f_inc, f_dec, alpha0;  /* alpha0 = config.alpha            */
  int32_t n_min;
  double dt_max;                /* in units of dt, like the reference        */
  double final_cap;
  double cap_scale;
  int32_t cap_upscale_every;
  int32_t remove_drift;         /* 0 no; 1 subtract the global mean of x, v;
                                   2 per-x-column means: what the reference
                                   does for 5-D states (mesh.py:496-497)   */
  /* state, device float [ncomp, batch, z, y, x] */
  float* x;
  float* v;
  float* a;
  const float* prev;            /* or NULL                                   */
  void* workspace;
  size_t workspace_bytes;
  void* stream;
  /* Optional native prev_fn (mesh.py:429-430): when set, `prev` must be NULL
     and prev = target_mesh(x) is re-evaluated inside every force evaluation. */
  const SfmTargetMeshDesc* target;
  /* Force model; zero-initialised descriptors get the spring stencils. */
  int32_t force_kind;           /* SFM_FORCE_*                               */
  const float* cx;              /* TILE_MESH: device [ncomp, batch*z, y, x]  */
  const float* cy;
  float* ext_force;             /* EXTERNAL: device, same shape as x         */
  SfmForceCallback force_cb;
  void* force_user;
  /* Generic prev_fn (mesh.py:429-430, any callable): when prev_cb is set, `prev`
     and `target` must be NULL; the library calls it on the host in front of
     every force evaluation (initial a = F(x), then after each position update)
     and it must enqueue, on `stream`, work that leaves prev_fn(x) in ext_prev
     (device, same shape as x; NaN = no spring).  Non-zero return aborts. */
  float* ext_prev;
  SfmForceCallback prev_cb;
  void* prev_user;
} SfmMeshDesc;

/* FIRE scalars carried between chunks (mesh.py:449, :513, :589). */
typedef struct SfmFireState {
  float dt;
  float alpha;
  int32_t n_pos;
  float cap;
} SfmFireState;

typedef struct SfmChunkStats {
  float e_kin;                  /* sum |v|^2   (mesh.py:584-585)             */
  float v_max;                  /* max |v|     (mesh.py:586)                 */
} SfmChunkStats;

size_t sfm_mesh_workspace_bytes(const SfmMeshDesc* desc);

/* out = mesh_force(x): device float, same shape as x.  Uses desc->x only. */
int sfm_mesh_force(const SfmMeshDesc* desc, float* out);

/* One call of mesh.velocity_verlet (mesh.py:371-521): a = F(x); num_iters
 * damped-Verlet or FIRE steps on x, v, a in place; `fire` is in/out (n_pos
 * restarts at 0 like the reference); stats are copied back to the host, which
 * synchronises the stream. */
int sfm_mesh_relax_chunk(const SfmMeshDesc* desc, SfmFireState* fire,
                         SfmChunkStats* stats);

/* ------------------------------------------------------------------------
 * One mesh across GPUs (one process per GPU).  The reference has no
 * multi-device code; these entry points split the step of
 * sfm_mesh_relax_chunk (mesh.velocity_verlet, mesh.py:436-499) at its two
 * exchange points so that bands of rows of ONE mesh can live on different GPUs:
 * the 1-node halo of the 8 / 26-neighbour stencil (mesh.py:106-167, :230-277)
 * and the whole-array reductions of FIRE (power :455, drift means :494-497,
 * e_kin / v_max mesh.py:584-586).
 *
 * A band holds rows [own_y0, own_y1) of the local array plus the halo rows
 * next to them.  Per step the caller
 *   1. brings (x, v, a) of the halo rows from the neighbour bands and gathers
 *      every band's `my_sums` row into `sums` (sfm_comm_* below, or any other
 *      transport),
 *   2. sfm_mesh_shard_advance  (FIRE scalars from `sums`, reduced in rank order
 *      on every band -> identical everywhere; pending gate / drift; position
 *      update of owned and halo rows),
 *   3. sfm_mesh_shard_integrate (force, velocity update, partial sums of the
 *      owned rows -> my_sums).
 * Only SfmMeshDesc.prev (no prev_fn), spring / tile-mesh forces and
 * remove_drift 0 | 1 are supported.  Everything is enqueued on desc->stream;
 * only sfm_mesh_shard_finish synchronises.
 * ---------------------------------------------------------------------- */
typedef struct SfmMeshShard {
  int32_t own_y0, own_y1;       /* owned rows of the local [.., y, x] arrays  */
  int64_t global_nodes;         /* nodes of the whole mesh (drift mean)       */
  int32_t n_ranks;              /* rows of `sums`                             */
  float* sums;                  /* device [n_ranks, 8], gathered by the caller */
  float* my_sums;               /* device [8]: power, sum x[3], sum v[3], 0   */
  int32_t phase;                /* library state: steps advanced so far       */
  float cap0;                   /* library state: force cap without FIRE      */
} SfmMeshShard;

/* a = F(x) + pull on the local rows; FIRE scalars of the chunk from `fire`. */
int sfm_mesh_shard_begin(const SfmMeshDesc* desc, SfmMeshShard* shard,
                         const SfmFireState* fire);
int sfm_mesh_shard_advance(const SfmMeshDesc* desc, SfmMeshShard* shard);
int sfm_mesh_shard_integrate(const SfmMeshDesc* desc, SfmMeshShard* shard);
/* Pending gate / drift of the last step (needs the last `sums`); `fire` gets
 * the chunk's final scalars, `stats` e_kin and v_max of the OWNED rows. */
int sfm_mesh_shard_finish(const SfmMeshDesc* desc, SfmMeshShard* shard,
                          SfmFireState* fire, SfmChunkStats* stats);

/* The same split step with the loop INSIDE the library: one call runs
 * desc.num_iters steps of every local band, moving the edge rows between local
 * bands by device copies and between ranks through `comm` (grouped RCCL
 * send / recv), all-gathering the bands' partial sums once per step, with the
 * exchange of a step's edge rows overlapped with the integration of its
 * interior rows (second stream).  Band g = rank * n_local + i owns rows
 * [own_y0, own_y1) of bands[i]'s arrays; shards[i].global_nodes must be set,
 * sums / my_sums / n_ranks are filled in by the library.  In-plane spring
 * meshes need SfmMeshDesc.workspace as for sfm_mesh_relax_chunk (it holds the
 * second state set).  `fire` in/out and `stats` are those of the WHOLE mesh
 * (e_kin added up in band order, v_max the maximum), identical on every rank.
 * Synchronises desc.stream once, at the end of the chunk. */
#define SFM_BANDED_LOOPBACK 1   /* exchanges between LOCAL bands travel through
                                   comm as self send / recv too (exercises the
                                   RCCL path on one GPU)                       */
#define SFM_BANDED_NO_OVERLAP 2 /* one launch per band and step, exchange after it */
/* Host-staged transport (twin of force_cb / prev_cb): used between ranks when
 * `comm` is NULL and n_ranks > 1, so that the inter-rank branch of the loop --
 * peer indexing, packed edge rows, the in-place all-gather layout with several
 * bands per rank, the edge-first split on the second stream -- also runs where
 * RCCL cannot connect the ranks (several processes sharing one GPU, CPU-side
 * process groups).  The library synchronises the exchange stream, copies the
 * packed rows to host memory, calls back, and copies the received rows to the
 * device; every pointer the callbacks see is HOST memory.  Argument meaning as
 * sfm_comm_halo_exchange / sfm_comm_allgather below (peer = -1: no neighbour on
 * that side; `recv` of the all-gather holds n_ranks * count floats, rank r's
 * part at r * count, and the callee fills every part).  Return 0, or non-zero
 * to abort the chunk (SFM_ERR_INVALID, like force_cb). */
typedef int (*SfmHostHaloFn)(void* user, int peer_lo, const float* send_lo, float* recv_lo,
                             int peer_hi, const float* send_hi, float* recv_hi, size_t count);
typedef int (*SfmHostAllgatherFn)(void* user, const float* send, float* recv, size_t count);
struct SfmComm;
typedef struct SfmBandedDesc {
  int32_t n_local;              /* bands of this rank, consecutive, in y order  */
  const SfmMeshDesc* bands;     /* [n_local]                                   */
  SfmMeshShard* shards;         /* [n_local]                                   */
  struct SfmComm* comm;         /* NULL: this process holds the whole mesh      */
  int32_t rank;
  int32_t n_ranks;              /* every rank holds n_local bands               */
  int32_t flags;                /* SFM_BANDED_*                                 */
  void* comm_stream;            /* exchange stream; NULL: bands[0].stream       */
  void* scratch;                /* device, sfm_mesh_banded_scratch_bytes        */
  size_t scratch_bytes;
  SfmHostHaloFn host_halo;      /* both or neither; ignored when comm is given   */
  SfmHostAllgatherFn host_allgather;
  void* host_user;
} SfmBandedDesc;
size_t sfm_mesh_banded_scratch_bytes(const SfmBandedDesc* desc);
int sfm_mesh_relax_banded(const SfmBandedDesc* desc, SfmFireState* fire,
                          SfmChunkStats* stats);

/* RCCL transport of those exchanges (resolved at run time; SFM_ERR_NO_DEVICE
 * when no librccl can be loaded).  One communicator per process on the
 * current device; rank 0 creates the id and hands its SFM_COMM_ID_BYTES bytes
 * to the other ranks out of band. */
#define SFM_COMM_ID_BYTES 128
#define SFM_REDUCE_SUM 0
#define SFM_REDUCE_MAX 1
typedef struct SfmComm SfmComm;
int sfm_comm_unique_id(void* id128);
int sfm_comm_init(SfmComm** comm, const void* id128, int rank, int n_ranks);
int sfm_comm_destroy(SfmComm* comm);
/* Sends `count` floats to each existing neighbour and receives as many, as one
 * grouped send/recv (peer = -1: no neighbour on that side). */
int sfm_comm_halo_exchange(SfmComm* comm, int peer_lo, const float* send_lo,
                           float* recv_lo, int peer_hi, const float* send_hi,
                           float* recv_hi, size_t count, void* stream);
/* recv[r * count .. (r + 1) * count) = `send` of rank r. */
int sfm_comm_allgather(SfmComm* comm, const float* send, float* recv, size_t count,
                       void* stream);
/* In-place all-reduce of a few scalars (chunk statistics). */
int sfm_comm_allreduce_scalars(SfmComm* comm, float* inout, size_t count, int op,
                               void* stream);

/* Test hook (no reference counterpart; tests/test_gpu_fft_own.py): batched 1-D complex FFT of
 * `n_pencils` strided pencils through the FFT form's pencil kernel -- pencil p at in + p,
 * its n_in samples at stride n_pencils (float2 each), zero-extended to length n; out
 * [n, n_pencils].  n: any length the hand-written transforms take (radices 2, 3, 5). */
int sfm_debug_fft1d(const void* in, void* out, int n, int n_in, int n_pencils,
                    int inverse, void* stream);

/* Test hook (no reference counterpart; tests/test_gpu_mesh_edges.py): the integrator
 * sfm_mesh_relax_chunk would run for `desc` under the switches in effect, from the same
 * planner, without launching anything (no HIP call beyond the device's CU count; none of
 * desc's pointers is dereferenced except `target`).  A persistent launch that times out
 * falls back to what the other fields describe. */
typedef struct SfmMeshPlanInfo {
  int32_t persist_tile;         /* persistent single launch: tile edge 16 | 32, 0 not taken  */
  int32_t persist_spec;         /* ... in its speculative form                                */
  int32_t small;                /* mesh_small_kernel: every step of the chunk in one launch   */
  int32_t tiled;                /* tiled in-plane step (integrate_shared2d_kernel)            */
  int32_t fused;                /* ... as one launch per step (position update included)      */
  int32_t packed;               /* ... with the narrow last tile column packed                */
  int32_t march_t;              /* z-march kernel: threads per workgroup, 0 not taken         */
  int32_t grid;                 /* workgroups of the per-node kernels                         */
  int32_t march_ntx;            /* z-march kernel: tile columns along x and y of a volume,    */
  int32_t march_nty;            /*   planes per workgroup, workgroups (0 where not taken)     */
  int32_t march_run;
  int32_t march_grid;
} SfmMeshPlanInfo;

int sfm_debug_mesh_plan(const SfmMeshDesc* desc, SfmMeshPlanInfo* info);

#ifdef __cplusplus
}
#endif
#endif  /* SOFIMA_AMD_H_ */
