/*
 * klt_amd.h -- libklt_amd.so extensions beyond the reference klt.h surface.
 * Used by bench.py / tests / tools for device-resident work; a reference
 * caller never needs them.
 */
#ifndef KLT_AMD_EXT_H
#define KLT_AMD_EXT_H

#include <stdint.h>

#include "klt.h"
#include "klt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the device context behind a tracking context (created on first use) */
klt_hip_ctx *klt_amd_device_context(KLT_TrackingContext tc);
/* Device contexts of freed tracking contexts are parked (at most 4, each
   trimmed to 2 GiB) for the next KLTCreateTrackingContext on the same device.
   This destroys the parked ones and returns their memory; returns how many. */
int klt_amd_release_cached_devices(void);
/* Opt-in for callers that reuse fixed frame buffers (example3.c's img1 and
   img2): page-lock [ptr, ptr+bytes) once, so that every KLTTrackFeatures /
   KLTSelectGoodFeatures / KLTReplaceLostFeatures on a frame inside it uploads
   the frame by one DMA from the caller's pages instead of copying it into
   pinned staging first.  Results are unchanged.  The buffer stays registered
   until klt_amd_unregister_buffer or KLTFreeTrackingContext; it must stay
   allocated that long.  0 on success, -1 (with a KLTWarning) otherwise. */
int klt_amd_register_buffer(KLT_TrackingContext tc, const void *ptr, size_t bytes);
int klt_amd_unregister_buffer(KLT_TrackingContext tc, const void *ptr);
/* the descriptors KLTTrackFeatures would build for this context */
void klt_amd_pyr_desc(KLT_TrackingContext tc, int ncols, int nrows, int nlevels, int smooth,
                      klt_hip_pyr_desc *desc);
void klt_amd_track_desc(KLT_TrackingContext tc, klt_hip_track_desc *desc);
/* KLT_HIP_EXACT (default) or KLT_HIP_FAST; env KLT_AMD_REDUCTION=fast sets FAST */
void klt_amd_set_reduction(KLT_TrackingContext tc, int reduction);
/* Forward-backward consistency check (klt_hip_set_fb in klt_hip.h has the
   exact definition), off by default: with it on, KLTTrackFeatures and
   KLTTrackSequence (which stays on its batched path) track every feature back
   from img2 to img1 in the same kernel launch and reject it -- x = y = -1,
   val = KLT_AMD_FB_REJECTED -- when it is lost on the way or returns farther
   than max_dist pixels from where it started.  max_dist must be finite and
   >= 0: otherwise -1 with a KLTWarning and the setting unchanged; 0 on
   success.  KLTTrackFeatures with the check on and affineConsistencyCheck >= 0
   or KLT_HIP_FAST sums is a KLTError. */
#define KLT_AMD_FB_REJECTED -6
int klt_amd_set_fb_check(KLT_TrackingContext tc, int on, float max_dist);
/* Motion prior (klt_hip_set_predict in klt_hip.h has the exact definition),
   off by default: with it on, every frame's search starts from the feature's
   displacement over the frame before, so that a feature moving steadily by
   more than the pyramid follows from a zero start is kept.  The tracking
   context keeps one state per list slot: zero when the setting is turned on
   (or off), when the list's size changes, for a slot that enters a frame lost
   or with val > 0 (fresh from selection or replacement), and for a feature
   lost by a frame.  Honoured by KLTTrackSequence and KLTTrackSequenceReplace
   (which stay on their batched path) and by KLTTrackFeatures, all in
   sequential mode, where consecutive calls are consecutive frames; without
   sequential mode the calls track from a zero start and drop the state.
   KLTTrackSequences* run their per-sequence loop with it on.  With
   klt_amd_set_fb_check on, affineConsistencyCheck >= 0 or KLT_HIP_FAST sums a
   tracking call is a KLTError; so is one with a window other than 7x7 or
   lighting_insensitive (the device call's refusal).  Returns 0. */
int klt_amd_set_prediction(KLT_TrackingContext tc, int on);

/* Region mask (klt_hip_set_mask in klt_hip.h has the exact definition): one
   byte per pixel, ncols x nrows, rows ncols bytes apart, nonzero = allowed,
   zero = masked; flags is an OR of KLT_HIP_MASK_SELECT and KLT_HIP_MASK_TRACK.
   The mask is copied into device memory that the tracking context owns, freed
   with it or with the next klt_amd_set_mask; NULL (or flags 0) clears it.
   With KLT_HIP_MASK_SELECT, KLTSelectGoodFeatures, KLTReplaceLostFeatures,
   KLTTrackSequenceReplace and KLTTrackSequencesReplace never place a feature
   on a masked pixel.  With KLT_HIP_MASK_TRACK, KLTTrackFeatures,
   KLTTrackSequence and KLTTrackSequenceReplace (which stay on their batched
   path), in sequential mode or not, lose a feature whose new position lies on a
   masked pixel: x = y = -1, val = KLT_AMD_MASKED.  KLTTrackSequences* run their
   per-sequence loop with the tracking use on.  A call whose image is not
   ncols x nrows is a KLTError while a mask is set; so is a tracking call with
   the tracking use on and klt_amd_set_fb_check, klt_amd_set_prediction,
   affineConsistencyCheck >= 0 or KLT_HIP_FAST sums, or with a window other than
   7x7 or lighting_insensitive (the device call's refusal).  Returns 0, or -1
   with a KLTWarning and the setting unchanged for flags outside the two bits,
   an empty size, or a failed device copy. */
#define KLT_AMD_MASKED -7
int klt_amd_set_mask(KLT_TrackingContext tc, const unsigned char *host_mask, int ncols, int nrows, int flags);

/* The reference harness loop (example3.c:54-74 without REPLACE) in one call:
     for (i = 1; i < nframes; i++) {
       KLTTrackFeatures(tc, frames[i-1], frames[i], ncols, nrows, fl);
       if (ft) KLTStoreFeatureList(fl, ft, ft_col + i - 1);
     }
   with bit-identical results (sequential mode included), run on the batched
   device path: frames uploaded asynchronously in chunks, pyramids built and
   features tracked 16 frames per launch.  Where one pyramid description
   cannot serve every frame (a kernel-cache corner case) or internal images are
   requested, it runs exactly that loop instead. */
void KLTTrackSequence(KLT_TrackingContext tc, KLT_PixelType **frames, int nframes, int ncols, int nrows,
                      KLT_FeatureList fl, KLT_FeatureTable ft, int ft_col);

/* The reference harness loop with REPLACE (example3.c:54-76) in one call,
   lost features replaced after every `every`-th tracked frame:
     for (i = 1; i < nframes; i++) {
       KLTTrackFeatures(tc, frames[i-1], frames[i], ncols, nrows, fl);
       if (i % every == 0) KLTReplaceLostFeatures(tc, frames[i], ncols, nrows, fl);
       if (ft) KLTStoreFeatureList(fl, ft, ft_col + i - 1);
     }                                     every == 1: example3.c with REPLACE
   The list (the aff_* fields of replaced slots included), the table, the kept
   pyramid and the kernel cache end exactly as that loop leaves them.  It runs
   on KLTTrackSequence's batched path with klt_hip_set_frames_replace on (off
   again when the call returns): only the tracker launch is cut at the
   replacement frames, where the list comes to the host for the selection.
   every < 1 is a KLTError; the other argument checks are KLTTrackSequence's.  A
   negative tc->mindist gets the reference's warning once and is set to 0.
   It runs exactly the loop above where KLTTrackSequence would fall back to
   its loop, when tc->sequentialMode is off (KLTReplaceLostFeatures then reads
   frames[i] through a selection image and the kernel cache), and when
   tc->affineConsistencyCheck >= 0; with every > nframes - 1 it is
   KLTTrackSequence. */
void KLTTrackSequenceReplace(KLT_TrackingContext tc, KLT_PixelType **frames, int nframes, int ncols, int nrows,
                             KLT_FeatureList fl, KLT_FeatureTable ft, int ft_col, int every);

/* KLTTrackSequence for nseq independent sequences of one geometry (a stereo
   rig, a camera array, many clips) in one call:
     for (s = 0; s < nseq; s++)
       KLTTrackSequence(tc_s, frames[s], nframes, ncols, nrows, fl[s], ft ? ft[s] : NULL, ft_col);
   on nseq fresh copies tc_s of tc (its parameters and settings, no kept
   pyramid), with bit-identical lists and tables.  tc's own kept pyramid
   (sequential mode) is neither read nor changed.  The sequences are tracked
   together, one device launch per 16 frames serving all of them
   (klt_hip_track_frames_multi): frames go up group by group through pinned
   staging, the upload is not overlapped with the device work.  Where that
   call does not apply -- KLTTrackSequence itself would fall back to its loop
   (a kernel-cache corner case, internal images), the affine or the
   forward-backward check is on, more than KLT_HIP_MAX_SEQUENCES sequences, or
   a configuration the call refuses (another window, lighting-insensitive
   mode, fast sums, other pyramid parameters) -- it runs exactly the loop
   above, each sequence on a context of its own.  Argument checks are
   KLTTrackSequence's, per sequence; ft may be NULL, and so may any ft[s]. */
void KLTTrackSequences(KLT_TrackingContext tc, KLT_PixelType ***frames, int nseq, int nframes, int ncols, int nrows,
                       KLT_FeatureList *fl, KLT_FeatureTable *ft, int ft_col);

/* KLTTrackSequenceReplace for nseq independent sequences of one geometry:
     for (s = 0; s < nseq; s++)
       KLTTrackSequenceReplace(tc_s, frames[s], nframes, ncols, nrows, fl[s], ft ? ft[s] : NULL, ft_col, every);
   on nseq fresh copies tc_s of tc, with bit-identical lists (the aff_* fields
   of replaced slots included) and tables.  The sequences are tracked together
   as in KLTTrackSequences, and at every `every`-th tracked frame the lost
   features of every sequence are replaced inside the device call
   (klt_hip_track_frames_multi_replace, with the frames tracked so far as its
   count0: the groups of 16 frames do not show): one trackability-map launch
   serves all sequences that lost a feature, the selections run one sequence
   after the other.  every < 1 is a KLTError, raised before any device is
   touched; with every > nframes - 1 it is KLTTrackSequences.  A negative
   tc->mindist gets the reference's warning once (tc itself is left as it is:
   the loop changes its copies).  It runs exactly the loop above where
   KLTTrackSequences would fall back to its loop, and when tc->sequentialMode
   is off (KLTTrackSequenceReplace then runs its per-frame loop). */
void KLTTrackSequencesReplace(KLT_TrackingContext tc, KLT_PixelType ***frames, int nseq, int nframes, int ncols,
                              int nrows, KLT_FeatureList *fl, KLT_FeatureTable *ft, int ft_col, int every);

/* host side of the synthetic generator (include/klt_synth.h) */
void klt_synth_frame(uint64_t seed, int t, int ncols, int nrows, unsigned char *out);
/* the reference quicksort's permutation on {val, idx} pairs (test hook) */
void klt_sort_pairs_full(int *val, int *idx, int n);

#ifdef __cplusplus
}
#endif

#endif
