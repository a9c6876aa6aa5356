/*
 * klt_hip.h -- the device C ABI of libklt_amd.so (HIP / CDNA4 gfx950).
 *
 * Plain C: pointers, sizes and POD descriptors, no HIP or torch types.  The
 * klt.h host layer (csrc/klt_api.c) is the main caller; bench.py and the
 * tests call it through ctypes for device-resident work.  Each entry point
 * replaces a reference CPU routine:
 *
 *   klt_hip_build_pyramid  <- _KLTToFloatImage + _KLTComputeSmoothedImage +
 *                             _KLTComputePyramid + _KLTComputeGradients per level
 *                             (convolve.c:37-53,273-314; pyramid.c:87-131;
 *                              trackFeatures.c:1296-1321)
 *   klt_hip_min_eigen      <- the trackability loop of _KLTSelectGoodFeatures
 *                             (selectGoodFeatures.c:375-424, :289-292)
 *   klt_hip_track          <- the per-feature loop of KLTTrackFeatures with
 *                             _trackFeature (trackFeatures.c:1343-1501, :381-486)
 *   klt_hip_track_affine   <- the same loop with the affine consistency check
 *                             (_am_trackFeatureAffine and the record stage,
 *                              trackFeatures.c:952-1225, :1438-1497)
 *
 * All functions return 0 on success and a negative code on failure; the
 * message is available from klt_hip_last_error().  Work is queued on the
 * context's stream (its own, or one handed in with klt_hip_set_stream) and is
 * asynchronous unless documented otherwise.
 */
#ifndef KLT_HIP_H
#define KLT_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KLT_HIP_MAX_TAPS 71  /* MAX_KERNEL_WIDTH, convolve.c:16 */
#define KLT_HIP_MAX_LEVELS 8
#define KLT_HIP_MAX_SLOTS 4  /* pyramid slots per context */

/* reduction order inside the Newton loop */
#define KLT_HIP_EXACT 0 /* reference order: bit-identical to the CPU path */
/* KLT_HIP_FAST: each window sum -- gxx, gxy, gyy, ex, ey, the residue and, in
   lighting-insensitive mode, the gain/bias moments -- is a float32 sum of the
   reference's terms in an unspecified order (a wave64 tree); everything else
   is as in KLT_HIP_EXACT.  Not bit-identical, and the order may differ between
   kernels, schedules and releases.  What the tests hold it to
   (tests/sum_scenes.py, tests/test_gpu_fast_sums.py): tracked one frame from
   the same start, at most 0.5 % of the features differ in status from, or lie
   more than B ulps of a coordinate from, the same tracker with float64 sums;
   B is 4 or 8 ulps by configuration, four times the 99th percentile of
   float32 sums in seven orders on the CPU
   (tests/golden/fast_sums_160x120.json).  Over a sequence the differences
   compound (tests/test_gpu_long.py: 0.5 px, 1e-3 of the statuses). */
#define KLT_HIP_FAST 1

/* taps exactly as _computeKernels produces them: k[0..width-1], un-reversed */
typedef struct {
  int width;
  float k[KLT_HIP_MAX_TAPS];
} klt_hip_taps;

/* how to turn a u8 frame into a pyramid slot */
typedef struct {
  int ncols, nrows;      /* level-0 size */
  int nlevels;           /* tc->nPyramidLevels (1 for selection images) */
  int subsampling;       /* tc->subsampling */
  int smooth_input;      /* 1: smooth the u8 frame with `smooth` first */
  klt_hip_taps smooth;   /* gauss, sigma = _KLTComputeSmoothSigma(tc) */
  klt_hip_taps pyr;      /* gauss, sigma = subsampling * pyramid_sigma_fact */
  klt_hip_taps grad_gauss; /* sigma = grad_sigma */
  klt_hip_taps grad_deriv;
} klt_hip_pyr_desc;

/* _trackFeature / KLTTrackFeatures parameters */
typedef struct {
  int window_width, window_height;
  int max_iterations;
  float min_determinant, min_displacement, max_residue, step_factor;
  int borderx, bordery;
  int lighting_insensitive;
  int reduction; /* KLT_HIP_EXACT or KLT_HIP_FAST */
} klt_hip_track_desc;

/* affine consistency check parameters (klt.h:71-83; trackFeatures.c:1472-1489) */
typedef struct {
  int mode;                          /* tc->affineConsistencyCheck: 0, 1 or 2 */
  int window_width, window_height;   /* tc->affine_window_*, odd */
  int max_iterations;                /* tc->affine_max_iterations */
  float min_determinant;             /* tc->min_determinant */
  float min_displacement;            /* tc->min_displacement */
  float affine_min_displacement;     /* tc->affine_min_displacement */
  float max_residue;                 /* tc->affine_max_residue */
  float max_displacement_differ;     /* tc->affine_max_displacement_differ */
  float step_factor;                 /* tc->step_factor */
  int lighting_insensitive;          /* tc->lighting_insensitive (mode 0) */
} klt_hip_affine_desc;
/* trackability-map parameters */
typedef struct {
  int window_width, window_height;
  int borderx, bordery; /* already max'ed with the window half sizes */
  int nSkippedPixels;
} klt_hip_select_desc;

/* per-kernel timing (HIP events on the context stream), milliseconds */
typedef struct {
  int n_pyr_l0, n_pyr_l1, n_track, n_eigen, n_generic;
  double ms_pyr_l0, ms_pyr_l1, ms_track, ms_eigen, ms_generic;
  long frames_pyr_l0, frames_pyr_l1, frames_track; /* frames covered by the timed launches */
} klt_hip_timing;

typedef struct klt_hip_ctx klt_hip_ctx;

/* device < 0: the calling thread's current HIP device */
klt_hip_ctx *klt_hip_ctx_create(int device);
void klt_hip_ctx_destroy(klt_hip_ctx *ctx);
/* back to a fresh context's settings (own stream, default tuning and host
   threads, no timing or counters, no current pyramid), after its own streams
   drain; it keeps its allocations for reuse unless they exceed 2 GiB, in which
   case the pyramid banks, the upload ring and the pinned staging are freed */
int klt_hip_ctx_reset(klt_hip_ctx *ctx);
int klt_hip_ctx_device(klt_hip_ctx *ctx);
/* the calling thread's current HIP device, -1 on error */
int klt_hip_current_device(void);
const char *klt_hip_last_error(klt_hip_ctx *ctx);
/* the tracker kernel instance the context launched last, as rocprofv3 names it
   (e.g. "kltdev::k_track7<false, true, 2, false>"); "" before any launch */
const char *klt_hip_track_kernel(klt_hip_ctx *ctx);
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL
   restores the context's own non-blocking stream */
int klt_hip_set_stream(klt_hip_ctx *ctx, void *stream);
void *klt_hip_get_stream(klt_hip_ctx *ctx);
int klt_hip_sync(klt_hip_ctx *ctx);
int klt_hip_device_count(void);

/* host u8 frame -> device staging buffer `buf` (0 or 1), via pinned memory */
int klt_hip_upload_frame(klt_hip_ctx *ctx, int buf, const unsigned char *host, int ncols,
                         int nrows);
/* build pyramid slot `slot` from device u8 frame (row pitch in bytes; pixels
   in the context's frame format, below);
   frame == NULL -> staging buffer `buf` from klt_hip_upload_frame (gray) */
int klt_hip_build_pyramid(klt_hip_ctx *ctx, int slot, const klt_hip_pyr_desc *desc,
                          const unsigned char *frame, long pitch, int buf);

/* Pixel format of DEVICE frames: 8-bit gray (default), or interleaved 8-bit
   RGB / BGR with or without a fourth (alpha) byte, which is ignored.  A colour
   pixel counts as the gray value
       gray = (4899*R + 9617*G + 1868*B + 8192) >> 14        (integers)
   -- the BT.601 luma weights in 14-bit fixed point.  The weights sum to 16384,
   so white stays 255 and a pixel with R = G = B keeps its value.  This formula
   is the definition; no equality with any other library's conversion is
   claimed.  A pyramid, a trackability map or a tracked list made from a colour
   frame is, byte for byte, what the same call gives on that frame converted
   by the formula (klt_hip_gray_host, klt_hip_to_gray).
   The setting covers klt_hip_build_pyramid with frame != NULL,
   klt_hip_frames_begin, klt_hip_track_frames, klt_hip_track_sequence and
   klt_hip_track_frames_multi: the conversion happens while the level-0 kernel
   (or, on the generic pyramid path, its u8 -> f32 pass) loads the pixels, so
   no gray copy of a frame is written.  pitch, stride and seq_stride stay byte
   counts, and a call whose pitch < ncols * bytes-per-pixel fails.  Everything
   downstream reads pyramids and composes unchanged (forward-backward and
   affine checks, replacement, lazy gradients, every schedule).
   Host-frame paths stay gray whatever the setting -- klt_hip_upload_frame and
   pyramids built from its staging buffers, klt_hip_track_frames_host, and the
   whole klt.h / klt_amd.h surface: colour would triple their bus traffic;
   convert with klt_hip_gray_host first.  klt_hip_track_frames_band, and with
   it the sharded drivers (klt_shard.h), fail with -1 and a message before any
   launch while the format is not gray, leaving the arrays untouched:
   klt_hip_to_gray is the route for those callers. */
#define KLT_HIP_FRAME_GRAY8 0
#define KLT_HIP_FRAME_RGB8 1
#define KLT_HIP_FRAME_BGR8 2
#define KLT_HIP_FRAME_RGBA8 3
#define KLT_HIP_FRAME_BGRA8 4
/* bytes per pixel of a format: 1, 3, 3, 4, 4; -1 for anything else.  Host only. */
int klt_hip_frame_bpp(int format);
/* an unknown format gives -1 with a message and leaves the setting unchanged;
   klt_hip_ctx_reset restores KLT_HIP_FRAME_GRAY8 */
int klt_hip_set_frame_format(klt_hip_ctx *ctx, int format);
int klt_hip_get_frame_format(klt_hip_ctx *ctx);
/* the formula on the host, no device needed: ncols x nrows pixels of `format`
   at src (row pitch in bytes) to gray bytes at dst (row pitch dst_pitch);
   KLT_HIP_FRAME_GRAY8 copies.  -1 for a null pointer, an unknown format,
   negative sizes, pitch < ncols * bytes-per-pixel or dst_pitch < ncols. */
int klt_hip_gray_host(int format, const unsigned char *src, long pitch, int ncols, int nrows,
                      unsigned char *dst, long dst_pitch);
/* the same on the device, as a plain kernel (k_to_gray) on the context's
   stream, asynchronous: nframes frames (frame f at dev_src + f*stride, bytes)
   to gray frames at dev_dst + f*dst_stride.  For callers of the paths that stay
   gray, and for anyone who wants the gray frame itself. */
int klt_hip_to_gray(klt_hip_ctx *ctx, int format, const unsigned char *dev_src, long pitch, long stride,
                    int nframes, int ncols, int nrows, unsigned char *dev_dst, long dst_pitch, long dst_stride);
/* test hook: 1 forces the generic one-pass-per-launch path even when the
   fused kernels apply (they must agree bit for bit) */
int klt_hip_set_path(klt_hip_ctx *ctx, int force_generic);
/* tuning hook: 1 tracks features in input order; 0 (default) in row-band
   order with each XCD given one band (L2 locality) and its share of the lost
   features (klt_hip_order_slot).  Results do not depend on it.
   Either call also drops the cached band order (reused by short calls while it
   covers at most 32 tracked frames), so the next call sorts afresh. */
int klt_hip_set_track_order(klt_hip_ctx *ctx, int input_order);
/* tracker kernel for the default configuration (7x7 window, exact sums, no
   gain/bias): 0 (default) the latency-lean k_track7 (track7_kernels.h), 1 the
   generic k_track_frames_g; identical results (A/B hook) */
int klt_hip_set_track_impl(klt_hip_ctx *ctx, int impl);
/* tuning hook: 1 (default) folds the finest level's residue pass of frame j
   into the first pass of frame j+1 within a batched launch (one-feature
   waves, exact sums, default gain): its gather goes out with that pass's and
   its sum is a sixth ordered chain; frame j+1's work is dropped when the
   verdict loses frame j's feature.  0: a residue pass of its own.  Results do
   not depend on it. */
int klt_hip_set_track_merge(klt_hip_ctx *ctx, int on);
/* 1 (default): a plain klt_hip_track_frames* call on the fused pyramid path,
   tracked by the default 7x7 kernel (exact sums, or fast sums on a two-level
   pyramid) with the forward-backward check off, keeps level 0 of its pyramid
   banks as the image plane alone; the
   tracker computes the level-0 gradients of the pixels its windows read, bit
   for bit the pyramid kernels' values.  0: level 0 with its gradients for
   every pixel, as every other call (band, forward-backward, other windows,
   lighting-insensitive, the generic pyramid path, per-call tracking) builds it.  A later
   reader of the kept pyramid that needs level-0 gradients (a call in another
   layout, klt_hip_frames_end_slot, klt_hip_min_eigen_rows) first completes
   that one frame (a replacement inside the call, klt_hip_set_frames_replace,
   reads the image plane directly where k_min_eigen7_img applies).  Results do
   not depend on it.  klt_hip_ctx_reset restores 1. */
int klt_hip_set_lazy_grad(klt_hip_ctx *ctx, int on);
/* tuning hook: 1 (default) builds the image-only level 0 of klt_hip_set_lazy_grad
   (whole gray frames whose width is a multiple of 8, with aligned rows) with
   k_pyr_l0s, barrier-free one-wave strips; 0 with the 64x32 tiles that every
   other level-0 build runs.  The environment variable KLT_L0_STRIP=0|1, read
   once, overrides it for every context (A/B in one tree).  Results do not
   depend on it.  klt_hip_ctx_reset restores 1. */
int klt_hip_set_l0_strip(klt_hip_ctx *ctx, int on);
/* Forward-backward (FB) consistency check, off by default.  With it on, every
   tracked frame img1 -> img2 of klt_hip_track (host or device arrays),
   klt_hip_track_sequence, klt_hip_track_frames and klt_hip_track_frames_host
   is followed, in the same tracker launch, by the reference's own step with
   the two images exchanged -- KLTTrackFeatures(img2, img1) on a copy of the
   forward result, same parameters, every level started from the forward
   position, the residue taken against img2 -- for every feature the forward
   step tracked.  The feature is rejected (x = y = -1, val =
   KLT_HIP_FB_REJECTED) when the backward step loses it, or when it returns to
   (xb, yb) with e = (xb - x0)^2 + (yb - y0)^2 > max_dist * max_dist, (x0, y0)
   being where the frame started: five float operations each rounded to float,
   the threshold one float product on the host.  A kept feature is exactly
   the forward result; a rejected one is lost from that frame on.  max_dist
   (pixels) must be finite and >= 0 (else -1, settings unchanged).
   The FB kernels take the residue pass in place, so klt_hip_set_track_merge
   is ignored while FB is on; the other tuning hooks apply and do not change
   results.  Not covered, failing with -1 and a message before any launch:
   KLT_HIP_FAST sums, klt_hip_track_frames_band (and the sharded drivers built
   on it), klt_hip_track_affine.  klt_hip_ctx_reset turns FB off. */
#define KLT_HIP_FB_REJECTED (-6)
int klt_hip_set_fb(klt_hip_ctx *ctx, int on, float max_dist);
int klt_hip_get_fb(klt_hip_ctx *ctx, int *on, float *max_dist);
/* optional device table of e with FB on: row f (stride elements apart, stride
   >= n) of a klt_hip_track_frames / _host call receives tracked frame f's e
   per feature, row 0 that of a klt_hip_track call or klt_hip_track_sequence
   step; -1.0f where there is no distance (the feature was lost before or by
   the forward step, or by the backward one).  NULL clears it, and so does
   klt_hip_ctx_reset.  The caller keeps the memory valid while it is set. */
int klt_hip_set_fb_table(klt_hip_ctx *ctx, float *dev_err, long stride);
/* Motion prior: every frame's search starts from the feature's displacement
   over the frame before, not from zero motion (the reference starts image 2 at
   image 1's position, which loses a steadily moving feature once its step
   passes what the coarsest level's Newton loop reaches).  dev_vx / dev_vy are
   device arrays of n floats, the state (vx, vy) per feature: read at every
   tracker launch, written at its end; the caller seeds them (zero: no prior)
   and keeps them valid while the setting is on.  One frame img1 -> img2 of a
   feature at (x, y) with status val:
     1. val != 0 on entry sets the state to (0, 0): val < 0 is lost and not
        tracked, val > 0 (fresh from selection or replacement) is tracked from
        a zero prior;
     2. gx = x + vx, gy = y + vy (one float addition each) go through the
        divisions by the subsampling as (x, y) does and give image 2's start;
        image 1's position is unchanged;
     3. at the coarsest level, after the first multiplication by the
        subsampling, a start whose window is not inside that level (the
        tracker's own bounds test; a NaN is not inside) is replaced by image
        1's position there, the unpredicted start;
     4. everything else is KLTTrackFeatures as it stands;
     5. a tracked feature's state becomes (x_new - x, y_new - y), two float
        subtractions; a lost feature's (0, 0).
   With an all-zero state the first frame is exactly the plain tracker's.
   Honoured by klt_hip_track with device arrays, klt_hip_track_sequence,
   klt_hip_track_frames and klt_hip_track_frames_host (which copies the state
   into a device block of its own before its first launch and back with the
   final list, so its arrays may be host arrays as x, y and val are), with or
   without klt_hip_set_frames_replace (rule 1 covers a replaced slot).
   Covered: the 7x7 window with KLT_HIP_EXACT sums on fused or generic
   pyramids of any depth, tracked by the k_track7_pred instances.  They read
   full level-0 records (klt_hip_set_lazy_grad does not apply) and take the
   residue pass in place (klt_hip_set_track_merge is ignored).  Refused with -1
   and a message before any launch, settings and lists untouched: the
   forward-backward check, the affine check (inside the launch and
   klt_hip_track_affine), KLT_HIP_FAST sums, any other window,
   lighting-insensitive mode and the generic tracker (klt_hip_set_track_impl 1,
   klt_hip_set_track_patch 0, klt_hip_set_prof), klt_hip_track_frames_band and
   the sharded drivers, the multi-sequence calls (klt_hip_multi_covers returns
   -1 as well), klt_hip_track with host arrays.  on = 0 clears the arrays;
   klt_hip_ctx_reset turns the setting off. */
int klt_hip_set_predict(klt_hip_ctx *ctx, int on, float *dev_vx, float *dev_vy);
int klt_hip_get_predict(klt_hip_ctx *ctx, int *on, float **dev_vx, float **dev_vy);
/* optional device tables of the state with the prior on: row f (stride
   elements apart, stride >= n) receives the state after tracked frame f, rows
   counted as klt_hip_set_fb_table's.  Both or neither; NULL clears them, and
   so does klt_hip_ctx_reset. */
int klt_hip_set_predict_table(klt_hip_ctx *ctx, float *dev_tab_vx, float *dev_tab_vy, long stride);
/* Region mask: the parts of the image that are not scene (a vehicle hood, the
   rig's own body, a burnt-in timestamp, a vignetted rim).  dev_mask is device
   memory, one byte per level-0 pixel, nrows rows `pitch` >= ncols bytes apart;
   nonzero = allowed, zero = masked (OpenCV's convention).  flags is an OR of
   the two uses, switched separately:
     KLT_HIP_MASK_SELECT  selection and replacement never place a feature on a
       masked pixel.  The walk of _KLTSelectGoodFeatures /
       KLTReplaceLostFeatures is the reference's, with every masked pixel
       marked in its feature map before the first point is visited (when
       replacing: in addition to the squares of the live features).  The point
       list and its sort are those of the whole map, so the order, ties
       included, is unchanged and an all-allowed mask gives the bytes of no
       mask; slots that cannot be filled become (-1, -1, KLT_NOT_FOUND) and
       `changed` keeps its meaning.  Honoured wherever the selection engine
       runs: klt_hip_select, klt_hip_select_dev_map, klt_hip_select_map, the
       replacement inside klt_hip_track_frames / _host
       (klt_hip_set_frames_replace) and klt_hip_track_frames_multi_replace (one
       mask for every sequence), and the sharded replacement (each rank's
       context carries its mask).  It composes with every tracker
       configuration and never refuses anything.
     KLT_HIP_MASK_TRACK  a tracked feature whose new position lies on a masked
       pixel is lost.  One frame of KLTTrackFeatures gives a status val and a
       position (xo, yo); after the level loop the status becomes KLT_OOB if
       val is KLT_OOB or the border test fails (unchanged, and first);
       otherwise KLT_HIP_MASKED with x = y = -1 if val != KLT_SMALL_DET and
       mask[(int)yo * pitch + (int)xo] == 0; otherwise val.  Like the border
       test it is a test of position: it beats KLT_LARGE_RESIDUE and
       KLT_MAX_ITERATIONS (every level ran, the position is a level-0 one) and
       not KLT_SMALL_DET (the loop broke at a coarser level).  A feature that
       starts on a masked pixel is tracked and tested like any other; a masked
       feature is lost from that frame on, and a replacement inside the call
       refills its slot.  Honoured by klt_hip_track with device arrays,
       klt_hip_track_sequence, klt_hip_track_frames and
       klt_hip_track_frames_host, with or without klt_hip_set_frames_replace:
       the 7x7 window with KLT_HIP_EXACT sums on fused or generic pyramids of
       any depth.  The batched calls whose banks hold level 0 as the image
       plane alone (klt_hip_set_lazy_grad 1) run the k_track7_mask_lazy
       instances, which keep the lazy gradients and the deferred residue
       (klt_hip_set_track_merge): the tentative position is tested at once and
       a pending residue verdict is dropped.  Every other honoured call runs
       the k_track7_mask instances on full level-0 records with the residue
       taken in place.  Results do not depend on either setting, on the track
       order, the chunk, or how frames are split over calls.
       Refused with -1 and a message before any launch,
       lists untouched, while this bit is on: the forward-backward check, the
       affine check (inside the launch and klt_hip_track_affine), the motion
       prior, KLT_HIP_FAST sums, any other window, lighting-insensitive mode
       and the generic tracker, klt_hip_track_frames_band and the sharded
       drivers, the multi-sequence calls (klt_hip_multi_covers returns -1 as
       well), klt_hip_track with host arrays.
   NULL or flags 0 clears the setting, and so does klt_hip_ctx_reset.  Flags
   outside the two bits return -1 with the setting unchanged.  The caller keeps
   the memory valid while the mask is set.  A pitch below the image width is
   refused by the calls that learn the width, before any launch. */
#define KLT_HIP_MASKED (-7)
#define KLT_HIP_MASK_SELECT 1
#define KLT_HIP_MASK_TRACK 2
int klt_hip_set_mask(klt_hip_ctx *ctx, const unsigned char *dev_mask, long pitch, int flags);
int klt_hip_get_mask(klt_hip_ctx *ctx, const unsigned char **dev_mask, long *pitch, int *flags);
/* tuning hook: 1 (default) raises the tracker waves' issue priority
   (s_setprio 3) so that, when the next chunk's pyramids are built beside the
   tracker (overlapped schedule, band calls with build-ahead), a feature's
   dependent chain issues ahead of the pyramid waves; 0 leaves it at 0.
   Results do not depend on it. */
int klt_hip_set_track_prio(klt_hip_ctx *ctx, int on);
/* measurement hook: on != 0 zeroes (allocating on first use) two device
   counters that every later tracker launch of this context adds to -- the 2x2
   systems formed, i.e. the reference's Newton loop bodies
   (trackFeatures.c:418-455, the SMALL_DET one included), and the gather round
   trips -- one pair of atomics per feature per launch; 0 frees them.  Results
   do not depend on it.  klt_hip_get_track_count synchronizes the device, reads
   both counters and zeroes them when reset != 0; it fails while counting is
   off. */
int klt_hip_set_track_count(klt_hip_ctx *ctx, int on);
int klt_hip_get_track_count(klt_hip_ctx *ctx, unsigned long long *solves, unsigned long long *passes,
                            int reset);
/* tuning hook: 0 disables the lane-patch gather of one-feature waves (default
   1: on where (ww+1)*(wh+1) <= 64).  Results do not depend on it. */
int klt_hip_set_track_patch(klt_hip_ctx *ctx, int on);
/* instrumented build only (make -C csrc prof): device buffer receiving 10
   u64 phase counters per tracker wave; a no-op buffer in the product build */
int klt_hip_set_prof(klt_hip_ctx *ctx, void *dev);
/* host threads of klt_hip_track_frames_host besides the caller (frame copies
   into pinned staging, table-row delivery); 0..16, default 7 */
int klt_hip_set_host_threads(klt_hip_ctx *ctx, int workers);
int klt_hip_get_host_threads(klt_hip_ctx *ctx);
/* Page-lock a caller buffer (hipHostRegister) so that frames inside it are
   uploaded by one DMA from the caller's pages, without the copy into pinned
   staging; for callers that reuse fixed frame buffers (the reference harness:
   img1/img2, example3.c:45-46,56,75).  Registered buffers must not overlap;
   they are released by klt_hip_unregister_host (after the context's streams
   drain), when the context is reset (parked) or destroyed.
   Lifetime: klt_hip_upload_frame from a registered buffer only QUEUES that
   DMA (the pageable path has finished reading the caller's bytes when it
   returns), so a direct klt_hip_* caller must not modify the frame's bytes
   until the context's stream has drained past the upload (klt_hip_sync, or
   any synchronous call after it).  The klt.h entry points (KLTTrackFeatures,
   KLTSelectGoodFeatures, KLTReplaceLostFeatures) synchronize before they
   return, so their callers may reuse the buffer at once. */
int klt_hip_register_host(klt_hip_ctx *ctx, const void *ptr, size_t bytes);
int klt_hip_unregister_host(klt_hip_ctx *ctx, const void *ptr);
/* Byte budget of the three pyramid banks of klt_hip_track_frames* (one device
   arena per context; 0 restores the default: a quarter of the device memory,
   at most 64 GiB).  A klt_hip_track_frames call whose chunk does not fit runs
   with the largest chunk that does (results do not depend on the chunk); a
   klt_hip_track_frames_band call fails instead, before allocating.  Either
   fails cleanly when not even one frame fits, or when the arena exceeds the
   device's free memory. */
int klt_hip_set_bank_budget(klt_hip_ctx *ctx, size_t bytes);
size_t klt_hip_get_bank_budget(klt_hip_ctx *ctx);
/* frames per bank (launch) of the last klt_hip_track_frames* call */
int klt_hip_frames_chunk(klt_hip_ctx *ctx);
/* device bytes the context holds (pyramid slots, banks, upload ring, maps) */
size_t klt_hip_ctx_footprint(klt_hip_ctx *ctx);
/* The schedule of a klt_hip_track_frames call that spans several chunks (a
   call of one chunk, and each chunk of klt_hip_track_frames_host, stays on the
   context stream; band calls always use both streams).  Results are the same,
   bit for bit, in every schedule; klt_hip_ctx_reset restores 0.
     0  one stream (default): each chunk's pyramids, then its tracker.
     1  automatic: the library picks per call.  Lazy-gradient calls
        (klt_hip_set_lazy_grad), whose tracker fills the register file so
        that pyramid waves beside it only slow both down, take 3; every other
        call takes 2.
     2  beside: chunk c+1's pyramids are built on a second stream as soon as
        their bank is free, for the whole length of chunk c's tracker.
     3  tail: as 2, but the build is also held back until at most
        klt_hip_set_frames_tail waves of chunk c's tracker are still running:
        every wave of the launch adds 1 to a device counter as it leaves, the
        one that brings it to the threshold writes it to signal memory, and
        the second stream waits for that value (hipStreamWaitValue32).  The
        events of 2 remain the dependencies, the counter is only a release
        hint.  Only the lazy-gradient tracker kernels count (twin instances,
        k_track7_hook); calls tracked by any other kernel run as in 2.
   Anything else fails.  KLT_FRAMES_SCHED=0..3 in the environment replaces the
   value for every context of the process (A/B in one tree). */
int klt_hip_set_frames_overlap(klt_hip_ctx *ctx, int overlap);
/* schedule 3: the tracker waves that may still be running when the next
   chunk's build is released (default 4096, four per SIMD; 0: none, the build
   follows the tracker).  A launch of no more waves than this is not waited
   for.  KLT_FRAMES_TAIL=K in the environment replaces it. */
int klt_hip_set_frames_tail(klt_hip_ctx *ctx, int waves_left);
/* schedule 3's arithmetic, host only: with `base` exits counted before a launch
   of `launched` waves, returns 1 and the counter value to wait for in
   *threshold (base + launched - waves_left, so 1 <= *threshold - base <=
   launched), or 0 (nothing to wait for) when launched <= waves_left. */
int klt_hip_tail_threshold(unsigned base, unsigned launched, unsigned waves_left, unsigned *threshold);
/* measurement hook, off (NULL) by default: a device buffer of 4 + 2 * cap
   u64, zeroed but for [2] = cap, that every k_track7 launch fills with its
   waves' wall_clock64() (100 MHz) times: [4 + k] is the entry time of wave k
   of the launch's grid (4 * workgroup + wave in the workgroup), [4 + cap + i]
   the exit time of the wave that tracked feature i, or that had slot i >= n
   of the processing order and no feature.  The two lists are not paired (the
   sum of the wave durations is the difference of the two sums); an index >=
   cap leaves no time, a place no wave wrote stays 0, and [0], [1] and [3] are
   not written.  Bits 60..63 of every time hold the XCD the wave ran on (the
   hardware's XCC_ID), bits 0..59 the time.  The waves share no counter, so
   that the hook does not hold them back. */
int klt_hip_set_wave_times(klt_hip_ctx *ctx, void *dev);
/* The processing order's balanced layout, host only (the arithmetic
   k_band_order uses on the device).  A tracker launch over n features hands
   XCD x the slots [min(x S, n), min((x + 1) S, n)) with S = 4 * xcd_per.  With
   n_live live features in band order and n - n_live lost ones, segment x
   starts with the live ranks [B_x, B_{x+1}), B_x = floor(n_live * min(x S, n)
   / n), and is filled up with lost ranks in order.  Writes the slot of live
   rank `rank` (lost = 0, rank < n_live) or of lost rank `rank` (lost = 1,
   rank < n - n_live) to *slot and returns 0; -1 for arguments outside that
   (n < 1, 8 S < n, n_live outside 0..n, a rank out of range, slot NULL). */
int klt_hip_order_slot(int n, int xcd_per, int n_live, int rank, int lost, int *slot);
/* test hook: runs the processing-order kernel (k_band_order) as a whole-frame
   tracker launch over n features would -- y and val are device arrays, nrows
   the image height -- and copies the order (slot -> feature) to the host
   array perm_out[n].  Synchronous.  KLT_ORDER_BALANCE=0 in the environment
   (read once, A/B only) restores the earlier layout, live features in band
   order and all lost ones last, for every order of the process. */
int klt_hip_band_order_probe(klt_hip_ctx *ctx, const float *y, const int *val, int n, int nrows, int *perm_out);
/* 1 if pyramids for `desc` would be built by the fused gfx950 kernels, else 0 */
int klt_hip_fused_path(klt_hip_ctx *ctx, const klt_hip_pyr_desc *desc);
/* 1 if the slot was built by the fused gfx950 kernels, 0 generic, <0 invalid */
int klt_hip_pyramid_path(klt_hip_ctx *ctx, int slot);
int klt_hip_level_dims(klt_hip_ctx *ctx, int slot, int level, int *ncols, int *nrows);
/* synchronous copy of one level plane (which: 0 img, 1 gradx, 2 grady) */
int klt_hip_download_level(klt_hip_ctx *ctx, int slot, int level, int which, float *host);
/* 1 if the level is stored interleaved ({gradx, grady, img} per pixel: the
   fused default-parameter pyramid, the layout k_track7 reads), 0 if as three
   planes (the generic path), -1 for a bad slot/level */
int klt_hip_level_interleaved(klt_hip_ctx *ctx, int slot, int level);
/* device pointer of a level plane (valid until the slot is rebuilt at a new
   size); for an interleaved level: which 0 gives the level's base
   (pixel i at base + 3 i), 1 and 2 give NULL */
const float *klt_hip_level_ptr(klt_hip_ctx *ctx, int slot, int level, int which);

/* track n features from slot1 (previous image) to slot2 (current image).
   on_device = 0: x/y/val are host arrays (copied in/out, synchronous);
   on_device = 1: x/y/val are device arrays, updated in place, asynchronous. */
int klt_hip_track(klt_hip_ctx *ctx, int slot1, int slot2, const klt_hip_track_desc *desc,
                  float *x, float *y, int *val, int n, int on_device);

/* The affine consistency check keeps each feature's stored window (img,
   gradx, grady of (ww+2) x (wh+2) floats: _KLTCreateFloatImage of
   trackFeatures.c:1449-1451) in a device store indexed by feature slot.
   klt_hip_affine_reserve sizes it for n features of window ww x wh and
   returns 1 when it was (re)allocated -- every stored window is then gone --,
   0 when it was kept.  klt_hip_affine_put / _get copy m windows between the
   store entries idx[0..m-1] and host memory win ([m][3][(ww+2)*(wh+2)],
   img | gradx | grady).  Synchronous. */
int klt_hip_affine_reserve(klt_hip_ctx *ctx, int n, int window_width, int window_height);
int klt_hip_affine_put(klt_hip_ctx *ctx, const int *idx, int m, const float *win);
int klt_hip_affine_get(klt_hip_ctx *ctx, const int *idx, int m, float *win);
/* klt_hip_track (host arrays, synchronous) followed by the affine consistency
   check of KLTTrackFeatures for every feature the translation tracker left
   TRACKED (trackFeatures.c:1438-1497).  Per feature k:
     aff[6k..6k+5]  aff_x, aff_y, Axx, Ayx, Axy, Ayy (in/out);
     state[k] in:   1 the store holds k's window, 0 it holds none;
              out:  0 none (lost, or never stored), 1 held, 2 stored by this call.
   A feature the affine stage rejects gets x = y = -1, aff_x = aff_y = -1 and
   its status in val, as in the reference. */
int klt_hip_track_affine(klt_hip_ctx *ctx, int slot1, int slot2, const klt_hip_track_desc *tdesc,
                         const klt_hip_affine_desc *adesc, float *x, float *y, int *val, float *aff,
                         int *state, int n);
/* The same check inside the tracker launch of the device-resident calls, off
   by default.  With it on (adesc != NULL), every tracked frame of
   klt_hip_track (on_device = 1), klt_hip_track_sequence, klt_hip_track_frames
   and klt_hip_track_frames_host is followed, in the same launch and before the
   next frame's translation step, by the reference's record stage
   (trackFeatures.c:1438-1497) for every feature that step left TRACKED:
     no window held -- the (ww+2) x (wh+2) img/gradx/grady window of the
       previous frame's level 0 around the position the frame started from is
       stored and aff_x / aff_y are set; nothing else changes;
     window held    -- _am_trackFeatureAffine runs from the stored window into
       the current frame's level 0.  On failure x = y = aff_x = aff_y = -1, val
       gets the status and the window is dropped; on success x / y stay the
       translation result and A is updated.
   A feature the translation step loses has no window afterwards.
     dev_aff    device array, 6 floats per feature (aff_x, aff_y, Axx, Ayx,
                Axy, Ayy), read and written;
     dev_state  device array, one int per feature.  In: nonzero = the window
                store holds this feature's window.  Out: 0 no window held, 1 a
                window held from before the call, 2 a window stored during
                this call and still held.
   The caller keeps both valid while the setting is on.  The window store is
   klt_hip_affine_reserve / _put / _get's: it must be reserved for at least n
   features of this window size, or the tracking call fails before any launch.
   Results are those of klt_hip_track_affine frame by frame, bit for bit, and do
   not depend on the chunk or on the tuning hooks.  Such calls run the generic
   tracker kernels on full level-0 records (klt_hip_set_lazy_grad does not
   apply; a kept image-only pyramid is completed first, as for any reader that
   needs its gradients) and take the residue pass in place
   (klt_hip_set_track_merge is ignored).  Failing with -1 and a message before
   any launch while it is on: klt_hip_track with host arrays,
   klt_hip_track_affine, klt_hip_track_frames_band (and the sharded drivers
   built on it), KLT_HIP_FAST sums, and any tracking call while the
   forward-backward check is on.  Argument checks as klt_hip_track_affine's
   (mode 0..2, window odd and >= 3; else -1, settings unchanged).
   adesc == NULL turns it off, and so does klt_hip_ctx_reset. */
int klt_hip_set_frames_affine(klt_hip_ctx *ctx, const klt_hip_affine_desc *adesc, float *dev_aff,
                              int *dev_state);
int klt_hip_get_frames_affine(klt_hip_ctx *ctx, int *on);
/* optional device tables with the setting on, either may be NULL: row f of a
   klt_hip_track_frames / _host call (row 0 of a klt_hip_track call or
   klt_hip_track_sequence step) receives, after tracked frame f, every
   feature's six values (dev_aff_tab, rows 6 * stride floats apart) and state
   (dev_state_tab, rows stride ints apart), stride >= n; lost features too:
   their current values and state 0.  Both NULL clears it, and so does
   klt_hip_ctx_reset.  The caller keeps the memory valid while it is set. */
int klt_hip_set_affine_table(klt_hip_ctx *ctx, float *dev_aff_tab, int *dev_state_tab, long stride);
/* for callers with host lists (KLTTrackSequence): copy aff[6n] / state[n] into
   device arrays the context owns and return them (for
   klt_hip_set_frames_affine), and copy them back.  Synchronous.  The arrays
   are also klt_hip_track_affine's scratch: valid until the next such call. */
int klt_hip_affine_state_put(klt_hip_ctx *ctx, const float *aff, const int *state, int n, float **dev_aff,
                             int **dev_state);
int klt_hip_affine_state_get(klt_hip_ctx *ctx, float *aff, int *state, int n);
/* device-resident sequential tracking, one frame per step: for step k, build
   frame t0+k (frames + (t0+k)*stride) on a second stream into the next of
   three slots (one frame ahead of the tracker), then track the device feature
   arrays from *cur_slot (0..2, the previous frame's pyramid) into it and
   advance *cur_slot.  Asynchronous.  klt_hip_track_frames is the batched form. */
int klt_hip_track_sequence(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc,
                           const klt_hip_track_desc *tdesc, const unsigned char *frames, long pitch,
                           long stride, int t0, int nsteps, float *x, float *y, int *val, int n,
                           int *cur_slot);

/* batched device-resident sequence -- the KLTTrackFeatures +
   KLTStoreFeatureList loop of the reference harness (example3.c:54-74) with
   no feature replacement, `chunk` frames per pair of pyramid launches and per
   tracking launch (pyramids of a chunk, then its tracking; see
   klt_hip_set_frames_overlap).
   klt_hip_frames_begin builds the pyramid the first tracked frame starts from;
   klt_hip_track_frames then tracks the device arrays x/y/val (n features)
   through frames[0..nframes-1] (frame f at frames + f*stride, row pitch
   `pitch`, both in bytes; pixels in the context's frame format,
   klt_hip_set_frame_format), and leaves the last frame's pyramid as the start
   of the next call.
   tab_* (device, optional: all three or NULL) receive the list after each
   frame in row f (row stride tab_stride >= n).  Three banks of `chunk`
   pyramids are allocated on first use (and regrown, after draining the
   streams, when chunk or the frame size grows).  Asynchronous. */
int klt_hip_frames_begin(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc, const unsigned char *frame,
                         long pitch);
int klt_hip_track_frames(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc, const klt_hip_track_desc *tdesc,
                         const unsigned char *frames, long pitch, long stride, int nframes, int chunk,
                         float *x, float *y, int *val, int n, float *tab_x, float *tab_y, int *tab_val,
                         long tab_stride);
/* start the next klt_hip_track_frames* call from pyramid slot `slot` (built by
   klt_hip_build_pyramid) instead of klt_hip_frames_begin's seed */
int klt_hip_frames_begin_slot(klt_hip_ctx *ctx, int slot);
/* copy the pyramid the next klt_hip_track_frames* call would start from (the
   last tracked frame's) into pyramid slot `slot` (device-to-device) */
int klt_hip_frames_end_slot(klt_hip_ctx *ctx, int slot);

/* nseq independent sequences of the same geometry and parameters in one
   batched call: one pair of pyramid launches and one tracker launch per chunk
   serve all of them (a feature's wave walks its chunk alone, so a launch of
   few features leaves most of the device idle; the sequences fill it).
   Sequence s has nframes + 1 device frames at frames + s*seq_stride + f*stride:
   f = 0 is the image its list starts on, f = 1..nframes are tracked.  n_seq
   (host int[nseq]) gives its feature count, 0 allowed; x/y/val (device, updated
   in place) hold the lists one after the other, sequence 0 first (n = the sum
   of n_seq).  tab_* (device, optional: all three or NULL) row j (tab_stride >=
   n apart) receives all nseq lists after tracked frame j, in that order.
   The result is, byte for byte, what klt_hip_frames_begin on frame 0 followed
   by klt_hip_track_frames on frames 1..nframes gives for each sequence on its
   own; it does not depend on chunk, on the bank budget or on the tuning hooks.
   Asynchronous, on the context's stream alone: klt_hip_set_frames_overlap's
   schedules are ignored (each chunk's pyramids, then its tracker), and so is
   klt_hip_set_track_order (features are processed in input order, which is
   one image per run of workgroups already).
   Banks: frame-major, frame j of every sequence adjacent, each bank nseq*chunk
   pyramids; the nseq pyramids a chunk starts from are the previous bank's last
   group, for the first chunk a group of their own in the bank that the third
   chunk reuses.  Level 0
   is kept as full records ({gx, gy, img} per pixel); klt_hip_set_lazy_grad does
   not apply to this call.  Pyramids are built by one pair of launches per chunk
   when stride == nseq*seq_stride (frame-major frames), else by one pair per
   sequence.  A bank budget too small for the requested chunk gives the largest
   chunk that fits (klt_hip_frames_chunk reports it); the call fails cleanly
   when not even one group of nseq pyramids per bank fits.
   The kept pyramid: the call carries its own start images and does not read
   the pyramid kept by klt_hip_frames_begin* or an earlier call; afterwards the
   context has no current pyramid, as after klt_hip_ctx_reset -- a later plain
   klt_hip_track_frames* call needs klt_hip_frames_begin* first.  (The nseq last
   pyramids are not carried into a next multi call either: that call builds its
   start images again.)
   Covered: the default configuration -- fused pyramids (klt_hip_fused_path),
   7x7 window, KLT_HIP_EXACT sums, tracked by k_track7.  Refused with -1 and a
   message before any launch, x/y/val untouched (klt_hip_multi_covers asks
   beforehand: 1 covered, 0 refused with the message set): the forward-backward
   check (klt_hip_set_fb), the affine check (klt_hip_set_frames_affine),
   KLT_HIP_FAST sums, any other window, lighting-insensitive mode, the generic
   pyramid path (other pyramid parameters, klt_hip_set_path), the generic
   tracker (klt_hip_set_track_impl 1, klt_hip_set_track_patch 0, klt_hip_set_prof);
   nseq < 1 or > KLT_HIP_MAX_SEQUENCES, a negative n_seq[s], nframes < 0,
   chunk < 1, pitch < ncols * bytes per pixel (klt_hip_set_frame_format), one
   or two of the three table arrays,
   tab_stride < n. */
#define KLT_HIP_MAX_SEQUENCES 64
int klt_hip_multi_covers(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc, const klt_hip_track_desc *tdesc);
int klt_hip_track_frames_multi(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc, const klt_hip_track_desc *tdesc,
                               const unsigned char *frames, long pitch, long stride, long seq_stride, int nseq,
                               int nframes, int chunk, const int *n_seq, float *x, float *y, int *val, float *tab_x,
                               float *tab_y, int *tab_val, long tab_stride);

/* feature-table rows handed back by klt_hip_track_frames_host: tracked frames
   frame0 .. frame0+nframes-1 (row j at x + j*stride), features [f0, f1).
   Called from several threads at once, on disjoint feature ranges. */
typedef void (*klt_hip_rows_fn)(void *user, int frame0, int nframes, int f0, int f1, const float *x,
                                const float *y, const int *val, long stride);
/* The batched sequence for frames in HOST memory (frames[f]: ncols*nrows u8,
   tight rows, pageable): chunk by chunk, a few host threads copy the chunk's
   frames into pinned staging, one DMA per chunk moves them into a device ring
   (copy stream), the chunk's pyramids and tracking run on the context stream,
   its feature-table rows come back by one D2H (a third stream) and are handed
   to `rows` (optional) -- the upload of chunk c+1 and the delivery of chunk
   c-1 overlap the device work on chunk c.  seed_first != 0: frames[0] is the
   image before the first tracked one (its pyramid is built from the uploaded
   copy) and frames[1..] are tracked; 0: the pyramid of klt_hip_frames_begin*
   or the previous call is the start and every frame is tracked.  x/y/val are
   HOST arrays of n features, updated in place.  Returns when every row has
   been delivered and x/y/val are written. */
int klt_hip_track_frames_host(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc,
                              const klt_hip_track_desc *tdesc, const unsigned char *const *frames,
                              int nframes, int seed_first, int chunk, float *x, float *y, int *val, int n,
                              klt_hip_rows_fn rows, void *user);

/* one chunk of the feature-sharded sequence (BASELINE config 4), for one rank
   of a row-band decomposition: like klt_hip_track_frames over nframes frames
   (one chunk), but the pyramids are built only for level-0 rows
   [row_lo, row_hi) (whole tiles, full-frame values; level-1 rows are valid
   where their sigma-3.6 support lies inside them) and only live features
   with own_lo <= y < own_hi at the chunk start are tracked (updated in place;
   the others are left untouched for the caller's exchange).  A feature whose
   window needs rows outside the built ones sets *escape (device int, caller
   zeroes it) and its result is invalid: the caller then redoes the chunk from
   full-frame pyramids (klt_hip_frames_begin on the frame before the chunk,
   row_lo = 0, row_hi = nrows).  next_frames (optional, next_nframes frames
   at the same pitch/stride): the next chunk, whose band pyramids are then
   built on the context's pyramid stream while this chunk is tracked and the
   caller exchanges results; the next call with exactly those frames and rows
   uses them.  Needs the default (fused) pyramid parameters. */
/* band calls of this context: ready != 0 promises that next_frames are ready
   when each call is made (device-resident, not written by work still queued on
   the context's stream), so the build-ahead waits for its bank and starts with
   this chunk's tracker instead of behind everything the caller queued before
   the call (its exchange) -- the short kernels between two trackers then run
   alone.  Default 0; kltamd.shard.ShardedSequence sets it (its frames are
   loaded up front). */
int klt_hip_set_ahead_ready(klt_hip_ctx *ctx, int ready);
int klt_hip_track_frames_band(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc,
                              const klt_hip_track_desc *tdesc, const unsigned char *frames, long pitch,
                              long stride, int nframes, float *x, float *y, int *val, int n, float own_lo,
                              float own_hi, int row_lo, int row_hi, int *escape,
                              const unsigned char *next_frames, int next_nframes);

/* Feature selection on the device (selectGoodFeatures.c:297-453 after the
   smoothing): the trackability map of slot `slot`'s level 0, then the
   reference's quicksort order produced lazily -- the top-level partition steps
   on the device, exactly (parallel form of the same step), the segments the
   walk reaches on the host -- and the minimum-distance walk.  x/y/val: the
   host feature list (in/out); overwrite_all 1 = KLTSelectGoodFeatures
   (every slot), 0 = KLTReplaceLostFeatures (slots with val < 0, live
   features' squares blocked).  changed[k] = 1 for every slot written (a new
   feature or NOT_FOUND; the caller resets its affine fields).  mindist as in
   the tracking context (the walk uses mindist-1, :157). */
int klt_hip_select(klt_hip_ctx *ctx, int slot, const klt_hip_select_desc *sd, int ncols, int nrows, int mindist,
                   int min_eigenvalue, int overwrite_all, float *x, float *y, int *val, unsigned char *changed,
                   int n);
/* the same walk over a device trackability map (nx x ny grid) */
int klt_hip_select_dev_map(klt_hip_ctx *ctx, const int *dev_map, int nx, int ny, const klt_hip_select_desc *sd,
                           int ncols, int nrows, int mindist, int min_eigenvalue, int overwrite_all, float *x,
                           float *y, int *val, unsigned char *changed, int n);
/* segments longer than `threshold` map points are split on the device (default 32768) */
int klt_hip_select_tune(klt_hip_ctx *ctx, int threshold);
/* last selection: map points copied to the host, device partition steps, sorted positions visited;
   host_us (optional, 4 values): wall clock of the map + init (queued and drained), the device
   splits, the segment downloads with their host sorts, and the whole walk */
int klt_hip_select_stats(klt_hip_ctx *ctx, long *downloaded, long *device_steps, long *visited, double *host_us);
/* test hook: the whole lazy order of host vals[0..n) as klt_sort_pairs_full gives it */
int klt_hip_select_sort_test(klt_hip_ctx *ctx, const int *vals, int n, int *out_val, int *out_idx);
/* trackability map of level 0 of `slot`: nx*ny int values, row-major over the
   border-trimmed grid; vals == NULL only reports nx, ny.  Synchronous. */
int klt_hip_min_eigen(klt_hip_ctx *ctx, int slot, const klt_hip_select_desc *desc, int *vals,
                      int *nx, int *ny);

/* the trackability map rows of the last tracked frame (the previous pyramid,
   as sequential-mode replacement reads it: selectGoodFeatures.c:342-348)
   whose pixel row lies in [row_lo, row_hi): grid rows [*r0, *r1) of the
   nx*ny map, written into dev_map (device, the whole map's layout; other rows
   untouched; NULL: only the sizes).  Returns 1 without writing when those
   rows' windows reach rows a band-built pyramid does not hold. */
int klt_hip_min_eigen_rows(klt_hip_ctx *ctx, const klt_hip_select_desc *desc, int row_lo, int row_hi, int *dev_map,
                           int *nx, int *ny, int *r0, int *r1);

/* test hook: the trackability map of a level-0 image plane in device memory
   (dev_img: ncols x nrows floats, tight rows -- what an image-only bank frame
   of klt_hip_set_lazy_grad holds) into dev_map (nx * ny ints), by
   k_min_eigen7_img: the kernel forms the gradients of each tile itself, with
   the default gradient taps (sigma 1.0), bit for bit what the pyramid kernels
   store, and then sums as the 7x7 map kernel does.  Synchronous.  Returns -1
   with a message for a window other than 7x7, a step (nSkippedPixels + 1)
   outside 1..2, or a border smaller than the window's half size. */
int klt_hip_min_eigen_plane(klt_hip_ctx *ctx, const float *dev_img, int ncols, int nrows,
                            const klt_hip_select_desc *desc, int *dev_map);
/* the trackability-map kernel the context launched last, as rocprofv3 names it
   (e.g. "kltdev::(anonymous namespace)::k_min_eigen7_img<1>"); "" before any
   launch and after klt_hip_ctx_reset */
const char *klt_hip_eigen_kernel(klt_hip_ctx *ctx);

/* Replacement of lost features inside the device-resident batched calls, off
   by default.  While it is on, klt_hip_track_frames and
   klt_hip_track_frames_host do, after every tracked frame whose 1-based count
   since the setting was turned on is a multiple of `every` and before the
   next frame is tracked, what KLTReplaceLostFeatures does to the list in
   sequential mode (selectGoodFeatures.c:514-541, :342-348): nothing when no
   slot is lost (val < 0); otherwise the lost slots are filled from the
   trackability map of the frame just tracked (klt_hip_select_dev_map with
   overwrite_all 0; slots it cannot fill become (-1, -1, KLT_NOT_FOUND)).
   Table row f and the `rows` callback carry the list after the replacement.
   The result is, bit for bit, that of the loop
       track frame; if (count % every == 0) replace; store
   and does not depend on chunk, on how the frames are split over calls (the
   count runs on from call to call) or on any tuning hook.
   Only the tracker launch is cut at the replacement frames: a sub-launch
   tracks frames [a, b) of a bank; the pyramid launches keep the call's chunk,
   and the next chunk's pyramids are queued before the host waits for the
   list.  The call runs on the context's stream (klt_hip_set_frames_overlap is
   ignored while the setting is on).  The map reads the frame where it lies in
   its bank: an image-only level 0 (klt_hip_set_lazy_grad) with a 7x7 window
   and step <= 2 by k_min_eigen7_img, records or planes by the kernels
   klt_hip_min_eigen_rows launches; an image-only frame with any other window
   or step is completed first.  A replacement that filled a slot drops the
   cached processing order.  A replacement due at the last frame of a call is
   run.  The forward-backward check composes with it (a rejected feature is
   lost and gets replaced; klt_hip_set_fb_table rows are unchanged).
   Failing with -1 and a message before any launch, arrays untouched, while it
   is on: klt_hip_track_frames_band, klt_hip_track_frames_multi,
   klt_hip_track_frames_multi_replace (which takes its replacement as an
   argument), klt_hip_track_sequence, and any call with
   klt_hip_set_frames_affine on.
   klt_hip_set_frames_replace(NULL) turns it off, and so does
   klt_hip_ctx_reset; turning it on zeroes the three counters of
   klt_hip_get_frames_replace (frames tracked, replacements run -- those with
   a lost slot --, slots filled; any pointer may be NULL) and the marks of
   klt_hip_frames_replace_changed.  It returns -1, settings unchanged, for
   every < 1, a border smaller than the window's half size, a window smaller
   than 1, or a negative nSkippedPixels. */
typedef struct {
  klt_hip_select_desc sel;     /* window, borders (already max'ed), nSkippedPixels */
  int mindist, min_eigenvalue; /* as in the tracking context */
  int every;                   /* >= 1 */
} klt_hip_replace_desc;
int klt_hip_set_frames_replace(klt_hip_ctx *ctx, const klt_hip_replace_desc *desc);
int klt_hip_get_frames_replace(klt_hip_ctx *ctx, int *on, long *frames, long *replacements, long *filled);
/* changed[k] = 1 for every slot k < n a replacement has written (a new
   feature or NOT_FOUND) since the setting was turned on, else 0: the slots
   whose affine fields a klt.h caller resets (KLTTrackSequenceReplace) */
int klt_hip_frames_replace_changed(klt_hip_ctx *ctx, unsigned char *changed, int n);

/* klt_hip_track_frames_multi with lost features replaced inside the call: for
   every sequence s the list, the table rows, the marks and the counters are,
   byte for byte, what
       klt_hip_frames_begin(frame 0 of s); klt_hip_set_frames_replace(rep);
       klt_hip_track_frames(frames 1..nframes of s)
   gives on a context of its own.  Frames, banks, coverage
   (klt_hip_multi_covers), argument checks and frame formats are
   klt_hip_track_frames_multi's.  The replacement is an argument, not a
   setting: the multi call keeps no state from call to call.  A replacement is
   due after tracked frame j (1-based within the call) when
   (count0 + j) % rep->every == 0; count0 is the number of frames tracked
   before this call, so a sequence split over several calls gives the bytes of
   one call.  A replacement due at the call's last frame is run.  It does to
   each sequence, on its own list and its own frame j, what
   klt_hip_set_frames_replace describes: nothing, counters included, when none
   of its slots is lost; otherwise its lost slots are filled from the
   trackability map of its frame, its live features blocking their squares,
   and the slots that cannot be filled become (-1, -1, KLT_NOT_FOUND).  No
   sequence sees another's features or map.  Table row j-1 carries every list
   after the replacement.  changed (host, n bytes, optional; the caller zeroes
   it): changed[k] |= 1 for every slot written.  runs / filled (host, nseq
   longs each, optional): added to, per sequence, the replacements run -- those
   with a lost slot -- and the slots filled.
   Schedule: the pyramid launches keep the chunk; the tracker launch alone is
   cut at the replacement frames, for all sequences at once.  At a cut the n
   features of x | y | val come to pinned host memory (one transfer when
   y == x + n and val == y + n, else three), the next chunk's pyramids are
   queued before the host waits, the sequences with a lost slot get their maps
   from one k_min_eigen7_multi launch (a 7x7 window with step <= 2; any other
   description from one k_min_eigen launch per sequence), and
   klt_hip_select_dev_map runs per sequence, one after the other; the lists and
   the table row go back when anything was written.  The call returns with the
   work after its last cut still queued, like klt_hip_track_frames_multi.
   Refused with -1 and a message before any launch, arrays untouched:
   everything klt_hip_track_frames_multi refuses, rep == NULL, the descriptions
   klt_hip_set_frames_replace refuses, count0 < 0, and the context's own
   klt_hip_set_frames_replace setting being on (it belongs to the
   single-sequence calls). */
int klt_hip_track_frames_multi_replace(klt_hip_ctx *ctx, const klt_hip_pyr_desc *pdesc,
                                       const klt_hip_track_desc *tdesc, const klt_hip_replace_desc *rep, long count0,
                                       const unsigned char *frames, long pitch, long stride, long seq_stride, int nseq,
                                       int nframes, int chunk, const int *n_seq, float *x, float *y, int *val,
                                       float *tab_x, float *tab_y, int *tab_val, long tab_stride,
                                       unsigned char *changed, long *runs, long *filled);
/* test hook: the trackability maps of nsel (1..KLT_HIP_MAX_SEQUENCES) frames of
   level-0 records in device memory ({gx, gy, img} per pixel, ncols x nrows,
   frame f at dev_rec + f*frame_stride floats -- what a multi bank holds) by
   one k_min_eigen7_multi launch: which (host, nsel frame indices, any subset
   in any order) picks the frames, map i goes to dev_maps + i*nx*ny.  Each map
   is bit for bit klt_hip_min_eigen's of that frame.  Synchronous.  Returns -1
   with a message for a window other than 7x7, a step (nSkippedPixels + 1)
   outside 1..2, a border below 3, or nsel out of range. */
int klt_hip_min_eigen_records(klt_hip_ctx *ctx, const float *dev_rec, long frame_stride, const int *which, int nsel,
                              int ncols, int nrows, const klt_hip_select_desc *desc, int *dev_maps);

/* the host half of KLTReplaceLostFeatures (selectGoodFeatures.c:514-541 ->
   _KLTSelectGoodFeatures' sort and minimum-distance fill, :425-453) over a
   complete trackability map in device memory (dev_map, nx*ny values as
   klt_hip_min_eigen_rows lays them out): fills the lost slots of the device
   feature arrays.  Synchronous.  The sharded drivers run it on every rank. */
int klt_hip_select_map(klt_hip_ctx *ctx, int ncols, int nrows, const klt_hip_select_desc *desc, int mindist,
                       int min_eigenvalue, const int *dev_map, float *x, float *y, int *val, int n);

/* The sharded schedule's exchange as an all-gather of per-rank slots (SURVEY
   8e; kltamd/shard.py and klt_shard_track use it).  Rank r owns the live
   features (val >= 0) whose chunk-start y0 lies in [edges[r], edges[r+1])
   (edges: world+1 floats, edges[0] = -inf, edges[world] = +inf; the band
   test of klt_hip_track_frames_band).  gather_order fills the device int
   array work[klt_hip_gather_work_ints(n, world)] (zeroed by the caller once,
   before its first use): per feature its owner and place among the owner's
   features in index order, every rank's count (work + n), and the
   bookkeeping pack and unpack read.  gather_pack
   writes rank `rank`'s owned (x, y, val) bit patterns into its slot of
   KLT_HIP_GATHER_SLOT_WORDS(S) int32 (S >= the largest count) with the escape
   flag (device int, may be NULL) and a failure count; the caller all-gathers
   the slots; gather_unpack takes every feature from its owner's slot
   (slots[k] is rank first_rank + k's, k < nslots; features of ranks outside
   them are left as they are) and writes flags[0] = the escape flags summed,
   flags[1] = the failures summed (a slot shorter than its count counts as
   one; nothing is unpacked then).  All three queue on the context's stream. */
#define KLT_HIP_GATHER_MAX_RANKS 16
#define KLT_HIP_GATHER_SLOT_WORDS(S) (4 + 3 * (long)(S))
/* gather_order options, each may be NULL: save (device int[3n]) receives a
   copy of x0 | y0 | v0 bit patterns (the chunk-start state a redo restarts
   from; needs x0) and *escape (device int) is zeroed, in the same launches
   (two: per-block counts, then places; no cross-workgroup handshake);
   host_counts (pinned host int[world]) and gather_unpack's host_flags (pinned
   host int[2]) receive the counts / flags from the kernels themselves, to be
   read once an event recorded after the launch has completed */
long klt_hip_gather_work_ints(int n, int world);
int klt_hip_gather_order(klt_hip_ctx *ctx, const float *x0, const float *y0, const int *v0, int n, const float *edges,
                         int world, int *work, int *save, int *escape, int *host_counts);
int klt_hip_gather_pack(klt_hip_ctx *ctx, const float *x, const float *y, const int *val, const int *work, int n,
                        int world, int rank, const int *escape, int nfail, int *slot, int S);
int klt_hip_gather_unpack(klt_hip_ctx *ctx, const int *slots, int nslots, int first_rank, const int *work, int n,
                          int world, int S, float *x, float *y, int *val, int *flags, int *host_flags);
/* gather_unpack then gather_order of the merged state (the next chunk's
   ownership, save, escape reset, counts) in two launches -- the step between
   two chunks' trackers; work is read for the unpack and rewritten */
int klt_hip_gather_unpack_order(klt_hip_ctx *ctx, const int *slots, int nslots, int first_rank, int *work, int n,
                                int world, int S, float *x, float *y, int *val, int *flags, int *host_flags,
                                const float *edges, int *save, int *escape, int *host_counts);

/* synthetic frames t0..t0+n-1 (include/klt_synth.h) into device memory */
int klt_hip_synth_frames(klt_hip_ctx *ctx, unsigned long long seed, int t0, int n, int ncols,
                         int nrows, unsigned char *dev, long pitch, long frame_stride);
/* rows row0 .. row0+nrows-1 of the same frames (one rank's band of a
   row-sharded sequence): row row0 of frame t0+f lands at dev + f*frame_stride */
int klt_hip_synth_rows(klt_hip_ctx *ctx, unsigned long long seed, int t0, int n, int ncols, int row0,
                       int nrows, unsigned char *dev, long pitch, long frame_stride);

/* device memory helpers (for callers without torch) */
void *klt_hip_malloc(klt_hip_ctx *ctx, size_t bytes);
void klt_hip_free(klt_hip_ctx *ctx, void *p);
int klt_hip_memcpy(klt_hip_ctx *ctx, void *dst, const void *src, size_t bytes, int kind);

int klt_hip_set_timing(klt_hip_ctx *ctx, int on);
/* synchronises, resolves the recorded events, resets the counters */
int klt_hip_get_timing(klt_hip_ctx *ctx, klt_hip_timing *out);

/* numerics self-checks used by the tests: f64 sqrt and f32 divide on device */
int klt_hip_selftest_sqrt(klt_hip_ctx *ctx, const double *in, double *out, int n);
int klt_hip_selftest_div(klt_hip_ctx *ctx, const float *a, const float *b, float *out, int n);
/* the default tracker's 2x2 solve, wave-uniform and on two lanes, on the same
   n cases (host arrays): sums[5 i ..] = {gxx, gxy, gyy, sum(dif gx), sum(dif gy)},
   step the step factor; out[6 i ..] = {dx, dy} of the uniform solve, of the
   two-lane solve from the ordered sums' lanes, of the two-lane solve from uniform
   sums; ok[i] bit k: solve k found det >= min_det (its outputs are 0 otherwise) */
int klt_hip_selftest_solve2(klt_hip_ctx *ctx, const float *sums, float step, float min_det, float *out, int *ok,
                            int n);
/* host-only self-check of the thread pool behind klt_hip_track_frames_host's
   pinned staging: `rounds` back-to-back groups of pieces (sizes and offsets
   varying per round, up to max_bytes) copied by `workers` threads plus the
   caller, each verified byte for byte.  0 on success, else the failing round
   + 1.  Needs no device. */
int klt_hip_selftest_copy_pool(int workers, int rounds, size_t max_bytes);

#ifdef __cplusplus
}
#endif

#endif /* KLT_HIP_H */
