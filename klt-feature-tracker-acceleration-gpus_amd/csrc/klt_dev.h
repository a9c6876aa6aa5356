// klt_dev.h -- internal interface between the gfx950 kernel files and the host
// runtime of libklt_amd.so (not installed, not part of the C ABI).
//
//   pyramid.hip   k_pyr_l0 / k_pyr_l1 (fused default-parameter pyramid; k_pyr_l0_px
//                 from colour pixels), the generic one-pass kernels, k_to_gray,
//                 k_min_eigen, k_synth
//   track.hip     k_track_frames_g (the Newton loop for any window, one wave per
//                 feature; the _g is only a name), k_band_order
//   track7.hip    k_track7 (the Newton loop of the default configuration)
//                 both with forward-backward instances (k_*_fb), k_track7 with
//                 multi-sequence ones (k_track7_multi); the kernels' bodies
//                 are track_body.h / track7_body.h.  k_track7's templates and
//                 device code are track7_kernels.h, which track7_pred.hip and
//                 track7_mask.hip include as well for the motion-prior and
//                 region-mask instances, code objects of their own
//   affine.hip    k_affine (the affine consistency check, one frame pair per
//                 launch); its per-feature stage is affine_dev.h, which
//                 track.hip's k_track_frames_g_aff runs inside the batched launch
//   runtime*.hip  host side, the klt_hip_* C ABI (include/klt_hip.h); the
//                 units share runtime.h (the device context) and host_pool.h:
//                 runtime.hip contexts, exit hook, uploads, setters, selection;
//                 runtime_pyr.hip slots, banks and pyramid builds;
//                 runtime_track.hip tracker launches, per-call and affine
//                 entry points; runtime_frames.hip the batched calls;
//                 runtime_multi.hip the batched call over several sequences
//
// Kernels stay internal to their file; the runtime reaches them through the
// launch_* functions declared here, which return the launch's hipError_t.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "klt_hip.h"

namespace kltdev {

constexpr int kWave = 64;
constexpr int kBlock = 256;

// status codes (klt.h:28-33)
constexpr int kTracked = 0, kNotFound = -1, kSmallDet = -2, kMaxIter = -3, kOOB = -4, kLargeResidue = -5;

__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// taps reversed so that out[c] = sum_{m=0}^{w-1} in[c-r+m] * rk[m], the
// accumulation order of convolve.c:171-172 / :225-228.
struct RTaps {
  int w;
  float k[KLT_HIP_MAX_TAPS];
};

inline RTaps reverse_taps(const klt_hip_taps &t) {
  RTaps r;
  r.w = t.width;
  for (int m = 0; m < t.width; ++m) r.k[m] = t.k[t.width - 1 - m];
  for (int m = t.width; m < KLT_HIP_MAX_TAPS; ++m) r.k[m] = 0.0f;
  return r;
}

// default configuration of the fused path: sigma 0.7 / 1.0 / 3.6, subsampling 4
constexpr int kRS = 2, kRG = 3, kRP = 10, kSS = 4;
// centre of the 7-tap derivative: -0 * g / sum == +0 exactly (convolve.c:92),
// so a product with it can be left out of an ordered sum (pyramid.hip)
constexpr int kDC = 3;

struct DefTaps {
  float s[5];   // smoothing gauss, reversed
  float g[7];   // gradient gauss, reversed
  float d[7];   // gradient derivative, reversed
  float p[21];  // pyramid gauss, reversed
};

// hs (the level-0 rows pass of the pyramid smoothing, W1 = W/4 columns, H rows)
// is stored in column slabs 16 wide: slab X/16 holds rows 0..H-1 of its 16
// columns contiguously.  A 64-column level-0 tile owns exactly one slab, so
// its 32 rows are one contiguous 2 KB run of whole cache lines.
constexpr int kHsSlab = 16;
__host__ __device__ __forceinline__ long hs_at(int y, int X, int H) {
  return ((long)(X / kHsSlab) * H + y) * kHsSlab + (X % kHsSlab);
}
__host__ __device__ __forceinline__ long hs_size(int W1, int H) {
  return (long)((W1 + kHsSlab - 1) / kHsSlab) * kHsSlab * H;
}

// An interleaved level stores one 12-byte record per pixel, {gx, gy, img}:
// the gradient pair first, so that a kernel computing (gx, gy) as one packed
// f32 pair writes it and the image value with one 12-byte store from three
// consecutive registers (the pair is even-aligned), and a wave writes 64
// consecutive records as one contiguous 768-byte run.
constexpr int kRecGx = 0, kRecGy = 1, kRecImg = 2, kRec = 3;
// A level's layout (Level::il / TrkLevel::il): three planes, the interleaved
// records, or -- level 0 of a bank whose tracker computes its own windows'
// gradients from the image (klt_hip_set_lazy_grad) -- the img plane alone
constexpr int kLayoutPlanes = 0, kLayoutRec = 1, kLayoutImg = 2;

// Colour device frames (klt_hip_set_frame_format): interleaved 8-bit channels,
// 3 or 4 bytes a pixel.  gray = (4899 R + 9617 G + 1868 B + 8192) >> 14, the
// BT.601 weights in 14-bit fixed point (they sum to 1 << 14); alpha is ignored.
// One definition for the device kernels and klt_hip_gray_host.
constexpr uint32_t kGrayR = 4899, kGrayG = 9617, kGrayB = 1868, kGrayHalf = 8192;
constexpr int kGrayShift = 14;
static_assert(kGrayR + kGrayG + kGrayB == (1u << kGrayShift), "white stays 255");
// bytes per pixel of a KLT_HIP_FRAME_* format; -1: not a format
constexpr int frame_bpp(int fmt) {
  return fmt == KLT_HIP_FRAME_GRAY8                                 ? 1
         : (fmt == KLT_HIP_FRAME_RGB8 || fmt == KLT_HIP_FRAME_BGR8)   ? 3
         : (fmt == KLT_HIP_FRAME_RGBA8 || fmt == KLT_HIP_FRAME_BGRA8) ? 4
                                                                      : -1;
}
// the weights of a pixel's bytes 0 and 2 (byte 1 is green in every format)
constexpr bool frame_bgr(int fmt) { return fmt == KLT_HIP_FRAME_BGR8 || fmt == KLT_HIP_FRAME_BGRA8; }
__host__ __device__ __forceinline__ uint32_t gray_of(uint32_t c0, uint32_t c1, uint32_t c2, bool bgr) {
  return ((bgr ? kGrayB : kGrayR) * c0 + kGrayG * c1 + (bgr ? kGrayR : kGrayB) * c2 + kGrayHalf) >> kGrayShift;
}

// tile geometry the runtime needs for grids and band bookkeeping
namespace geom {
constexpr int L0_TW = 64, L0_TH = 32;  // k_pyr_l0 tile (level-0 pixels)
constexpr int L1_TW = 32, L1_TH = 32;  // k_pyr_l1 tile (level-1 pixels)
constexpr int L1_HR = kSS * (L1_TH + 2 * kRG - 1) + 2 * kRP + 1;  // hs rows an L1 tile reads: [4*y0-20, +HR)
}  // namespace geom

// grid.x for the XCD-aware tile order: a multiple of 8 covering `tiles`
inline unsigned xcd_grid(int tiles) { return (unsigned)(8 * ((tiles + 7) / 8)); }
inline unsigned blocks_for(long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// ---------------------------------------------------------------------------
// tracker arguments (track.hip)
// ---------------------------------------------------------------------------
struct TrkLevel {
  const float *img, *gx, *gy;  // il: img is the interleaved base ({gx, gy, img} per pixel), gx/gy null
  int w, h;
  int vlo = 0, vhi = 1 << 30;  // rows that hold valid data (a band-built pyramid: fewer)
  int il = 0;                  // kLayoutPlanes / kLayoutRec / kLayoutImg (img alone, gx/gy null)
};

struct TrkArgs {
  TrkLevel A[KLT_HIP_MAX_LEVELS];  // previous image (img1)
  TrkLevel B[KLT_HIP_MAX_LEVELS];  // current image (img2)
  int nlev;
  float ss;
  float ss_inv;       // 1/ss when ss is a power of two (x / ss == x * ss_inv bit for bit), else 0
  int ww, wh, max_it;
  float min_det, min_disp, max_res, step;
  int borderx, bordery, ncols, nrows;
  int li;
  int red_pitch;     // per-sum row pitch of the reduction staging area (floats)
  int merge_res;     // 1: defer the finest level's residue into the next frame's first pass
  int *escape;       // band mode: set when a window needs rows outside [vlo, vhi)
  int prio;          // 1: tracker waves raise their issue priority (s_setprio 3) over concurrent pyramid waves
  int aos;           // 1 (k_track7): a level's img is {gx, gy, img} interleaved per pixel (gx/gy unused)
  int fast;          // 1 (k_track7): KLT_HIP_FAST window sums (DPP tree), interleaved two-level pyramids only
  // k_track7 (set by launch_track7): per level, the bit pattern of the smallest
  // float x >= 3 with (float)w - (x + 3) < 1.001f (ooby: the same for h), so the
  // window bounds test is integer compares of x's and y's bit patterns
  int oobx[KLT_HIP_MAX_LEVELS], ooby[KLT_HIP_MAX_LEVELS];
  // k_track7's lazy-gradient instances: level 0 of B (and of A, when A[0].il
  // says so) is an img plane, and the kernel computes the gradients of the
  // pixels its windows touch with these taps (DefTaps::g / ::d, reversed)
  int lazy;
  float gg[7], gd[7];
};

// batched frames: frame j tracks pyramid j-1 -> j of a bank; row j of the
// optional feature table receives the list after frame j
struct TrkFramesArgs {
  long lfs[KLT_HIP_MAX_LEVELS];  // bank frame stride per level (floats)
  int nframes;
  const int *perm;   // processing order (slot -> feature), nullptr: identity
  const int *n_dev;  // non-null: number of slots to process (device value, <= n)
  int xcd_per;       // > 0: blockIdx -> XCD-major order, this many blocks per XCD
  unsigned long long *prof;  // per wave: phase cycle counts (instrumented build only)
  float *tx, *ty;
  int *tv;
  long tstride;  // table row stride (elements); tx == nullptr: no table
  unsigned long long *count;  // non-null: [kCountSlots] 2x2 systems formed, [kCountSlots] gather round trips
  // k_track7's lazy-gradient instances with HOOK only (launch_track7 picks them
  // when either pointer is set; the others never read these fields).
  // exits: every launched wave adds 1 as it leaves, the waves that return
  // before tracking too; the wave that brings the count to exit_thr writes
  // that value to exit_sig, signal memory a stream can wait on: "all but K
  // waves of this launch are gone" (klt_hip_set_frames_overlap's tail
  // schedule).  The count itself is in device memory: 5024 system-scope adds
  // to signal memory took 4.6 ms per launch.
  // wave_t: {0, 0, capacity, 0}, then `capacity` entry times and
  // `capacity` exit times (wall_clock64, the XCD in the top four bits), by
  // the wave's number in the grid and by its feature (klt_hip_set_wave_times)
  unsigned *exits, *exit_sig;
  unsigned exit_thr;
  unsigned long long *wave_t;
};
// forward-backward check (klt_hip_set_fb): the FB kernel instances take this
// beside TrkFramesArgs, so the FB-off instances keep their argument layout
struct TrkFbArgs {
  float t2;     // max_dist * max_dist, rounded to float on the host
  float *err;   // optional: row j receives frame j's squared return distance (-1: none); nullptr: no table
  long stride;  // its row stride (elements)
};
constexpr int kFbRejected = KLT_HIP_FB_REJECTED;
// motion prior (klt_hip_set_predict): the prediction instances of k_track7 take
// this beside TrkFramesArgs, so the others keep their argument layout
struct TrkPredArgs {
  float *vx, *vy;    // per feature: its displacement over the last tracked frame (in/out)
  float *tvx, *tvy;  // optional tables: row j receives the state after frame j; nullptr: none
  long tstride;      // their row stride (elements)
};
// region mask, tracking use (klt_hip_set_mask with KLT_HIP_MASK_TRACK): the
// mask instances of k_track7 take this beside TrkFramesArgs, so the others keep
// their argument layout
struct TrkMaskArgs {
  const unsigned char *mask;  // one byte per level-0 pixel, zero = masked
  long pitch;                 // bytes between rows
};
constexpr int kMasked = KLT_HIP_MASKED;
// several independent sequences in one launch (klt_hip_track_frames_multi):
// the multi instances take this beside TrkFramesArgs, so the others keep
// their argument layout.  Sequence s owns features [first[s], first[s + 1]) of
// the concatenated lists; the banks are frame-major -- frame j of sequence s
// is pyramid j * nseq + s of a.B, the pyramid its first frame starts from is
// pyramid s of a.A (the previous bank's last group, or the seed group) -- with
// TrkFramesArgs::lfs the stride of one pyramid.
constexpr int kMaxSeq = KLT_HIP_MAX_SEQUENCES;
struct TrkMultiArgs {
  int nseq;
  int first[kMaxSeq + 1];
};
// the trackability maps of several of those pyramids in one launch
// (k_min_eigen7_multi): map i is taken from pyramid seq[i] of the group, by
// value like TrkMultiArgs -- no device table, no upload
struct EigMultiArgs {
  int nsel;
  int seq[kMaxSeq];
};
constexpr int kCountSlots = 64;  // counter pairs (the host sums them)
constexpr int kProfN = 12;       // instrumented build: counters per wave

// ---------------------------------------------------------------------------
// affine consistency check arguments (affine.hip)
// ---------------------------------------------------------------------------
struct AffParams {
  int mode, ww, wh, max_it, li;
  float min_det, th, th_aff, max_res, mdd, step;
};

struct AffArgs {
  const float *ai, *agx, *agy;  // image 1, level 0
  const float *bi, *bgx, *bgy;  // image 2, level 0
  int aw, ah, bw, bh;
  const float *xp, *yp;  // positions before this frame's translation track
  const float *x, *y;    // after it
  int *v;                // status (in/out)
  float *xo, *yo;        // feature positions written back (lost: -1)
  float *aff;            // 6 per feature: aff_x, aff_y, Axx, Ayx, Axy, Ayy
  int *state;            // in: 1 window stored, 0 none; out: 0, 1, 2 = stored by this call
  float *store;          // 3*S floats per feature
  int n;
  AffParams p;
};

// the check inside the batched tracker launch (klt_hip_set_frames_affine): the
// affine instances take this beside TrkFramesArgs, so the others keep their
// argument layout
struct TrkAffArgs {
  AffParams p;
  float *aff;    // 6 per feature (in/out)
  int *state;    // in: nonzero = window held; out: 0, 1 held from before, 2 stored by this call
  float *store;  // 3*S floats per feature
  int fresh;     // 1: the call's first launch (a held window is state 1); 0: a later one (2 stays 2)
  int lds_wave;  // floats of dynamic LDS per wave: the staging and the solve's block
  float *tab_aff;  // optional tables: row j receives the values / states after frame j
  int *tab_state;
  long stride;     // features per table row (the affine row is 6 * stride floats)
};
// pixels per ordered-sum chunk of the affine stage inside the tracker launch
// ("The affine check in the batched launch")
#ifndef KLT_AFF_CH
#define KLT_AFF_CH 64
#endif
constexpr int kAffChunk = KLT_AFF_CH;

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// A launcher's choice among a kernel's instances yields one row of a table: the
// name klt_hip_track_kernel / klt_hip_eigen_kernel report (the instance as
// rocprofv3 names it; bench.py matches counter summaries on it) beside the
// kernel that is launched.  K: the pointer type of the kernels' argument list.
template <class K>
struct KernelRow {
  const char *name;
  K kernel;
};

// k_pyr_l0 over F frames (src + f*stride; outputs + f*fs0, hs + f*fsh), level-0
// tile rows [ty0, ty1) of 32-row tiles; only tile rows [py0, py1) store the
// level-0 planes (the others only the sigma-3.6 rows pass, hs)
// il: kLayoutPlanes, kLayoutRec, or kLayoutImg (img as a plane, no gradients)
hipError_t launch_pyr_l0(hipStream_t st, const uint8_t *src, int pitch, long stride, int W, int H, const DefTaps &T,
                         int vec_u8, int vec_out, float *img, float *gx, float *gy, float *hs, int W1, int do_hs,
                         long fs0, long fsh, int F, int ty0, int ty1, int py0 = 0, int py1 = 1 << 30, int il = 0,
                         int fmt = KLT_HIP_FRAME_GRAY8, int strips = 0);
// strips: the image-only level 0 of whole gray frames as k_pyr_l0s (one-wave
// strips) where the tile kernel's interior path qualifies (klt_hip_set_l0_strip)
// fmt: the source pixels' format (KLT_HIP_FRAME_*); pitch and stride are bytes.
// A colour format runs the k_pyr_l0_px instances, whose phase A stages the
// gray bytes of gray_of(); everything after phase A is k_pyr_l0's
// k_pyr_l1 over F frames, level-1 tile rows [ty0, ty1)
// il != 0 (both): the planes interleaved per pixel, {gx, gy, img} at img + 3*(y*w + x); gx/gy unused
// thin: 8-row tiles (ty0/ty1 in those), for a single frame; else geom::L1_TH rows
hipError_t launch_pyr_l1(hipStream_t st, const float *hs, int W1, int H, int H1, const DefTaps &T, int vec,
                         float *img1, float *gx1, float *gy1, long fsh, long fs1, int F, int ty0, int ty1, int il = 0,
                         int thin = 0);
constexpr int kL1ThinRows = 8;  // launch_pyr_l1's thin tiles
// generic one-pass kernels (any sigma / levels / subsampling)
hipError_t launch_u8_to_f32(hipStream_t st, const uint8_t *src, long pitch, int W, int H, float *out);
// the same from colour pixels: float(gray_of(pixel)) (fmt: a colour KLT_HIP_FRAME_* format)
hipError_t launch_px_to_f32(hipStream_t st, const uint8_t *src, long pitch, int W, int H, int fmt, float *out);
// n frames of fmt pixels (src + f*stride, row pitch in bytes) to gray bytes
// (dst + f*dstride, row pitch dpitch); gray frames are copied
hipError_t launch_to_gray(hipStream_t st, int fmt, const uint8_t *src, long pitch, long stride, int n, int W, int H,
                          uint8_t *dst, long dpitch, long dstride);
hipError_t launch_rows(hipStream_t st, const float *in, int W, int H, const RTaps &t, float *out);
hipError_t launch_cols(hipStream_t st, const float *in, int W, int H, const RTaps &t, float *out);
hipError_t launch_subsample(hipStream_t st, const float *in, int W, int ss, float *out, int W1, int H1);
// trackability map over the nx x ny grid from (bx, by), step apart; ps: the
// gradients' pixel stride (1 planes; 3 an interleaved level's {gx, gy, img}
// records, gx = base + kRecGx, gy = base + kRecGy); name: out, the kernel
// instance launched, as rocprofv3 names it
hipError_t launch_min_eigen(hipStream_t st, const float *gx, const float *gy, int W, int ps, int bx, int by, int step,
                            int nx, int ny, int hw, int hh, int *out, const char **name = nullptr);
// the same map (7x7 window, step 1 or 2) from a level-0 img plane alone, row
// stride W: k_min_eigen7_img forms the gradients of its tile with the 7-tap
// gradient kernels t (reversed, as k_rows / k_cols take them), bit for bit
// what launch_rows / launch_cols over the whole plane give
struct GradTaps {
  float g[2 * kRG + 1], d[2 * kRG + 1];  // gauss, derivative
};
hipError_t launch_min_eigen_img(hipStream_t st, const float *img, int W, int H, const GradTaps &t, int bx, int by,
                                int step, int nx, int ny, int *out, const char **name = nullptr);
// the same map (7x7 window, step 1 or 2, borders >= 3) of m.nsel frames of full
// {gx, gy, img} records, frame m.seq[i] at rec + m.seq[i] * frame_stride
// (floats), in one launch: map i at maps + i * nx * ny, each bit for bit
// launch_min_eigen's for that frame
hipError_t launch_min_eigen_multi(hipStream_t st, const float *rec, long frame_stride, const EigMultiArgs &m, int W,
                                  int bx, int by, int step, int nx, int ny, int *maps, const char **name = nullptr);
hipError_t launch_synth(hipStream_t st, unsigned long long seed, int t0, int n, int W, int H, int row0, uint8_t *out,
                        long pitch, long fstride);
hipError_t launch_selftest_sqrt(const double *in, double *out, int n);
// n pixels of an interleaved level into three planes
hipError_t launch_from_il(hipStream_t st, const float *il, float *img, float *gx, float *gy, long n);
// and back: n pixels of a plane into field kRecGx / kRecGy / kRecImg of {gx, gy, img} records
hipError_t launch_to_il(hipStream_t st, const float *plane, float *il, int field, long n);
// n 32-bit words, 16-byte aligned ends (device or mapped pinned host memory)
hipError_t launch_copy_words(hipStream_t st, const void *src, void *dst, long n);
hipError_t launch_selftest_div(const float *a, const float *b, float *out, int n);
hipError_t launch_selftest_solve2(const float *in, float step, float min_det, float *out, int *ok, int n);

// the tracker: one wave per feature; patch/win7 select the lane-patch gather
// and the compiled-in 7x7 window, npx the pixels-per-lane instance
// fb != nullptr: the forward-backward instances (exact sums, no band checks)
// af != nullptr: the affine-check instances (the same; not together with fb)
hipError_t launch_track_frames(hipStream_t st, bool exact, bool li, bool patch, bool win7, int npx,
                               const TrkArgs &a, const TrkFramesArgs &b, float *x, float *y, int *v, int n,
                               const TrkFbArgs *fb = nullptr, const TrkAffArgs *af = nullptr);
// dynamic LDS bytes a workgroup of the affine instances needs for `mode`
size_t track_affine_lds_bytes(int mode);
// track7.hip: the default configuration (7x7 window, exact sums, no gain/bias,
// one wave per feature) with the latency-lean pass; band: escape checks
// pr != nullptr: the motion-prior instances (exact sums, whole frames, not together with fb)
// mk != nullptr: the region-mask instances (the same; not together with fb or pr)
hipError_t launch_track7(hipStream_t st, bool band, const TrkArgs &a, const TrkFramesArgs &b, float *x, float *y,
                         int *v, int n, const char **name = nullptr, const TrkFbArgs *fb = nullptr,
                         const TrkPredArgs *pr = nullptr, const TrkMaskArgs *mk = nullptr);
// track7_pred.hip (track7_kernels.h's k_track7_pred instances), for launch_track7: a with the bounds thresholds, its
// grid and depth
hipError_t launch_track7_pred(hipStream_t st, const TrkArgs &a, const TrkFramesArgs &b, const TrkPredArgs &pr, float *x,
                              float *y, int *v, int n, int grid, bool two, const char **name);
// track7_mask.hip (the k_track7_mask and k_track7_mask_lazy instances), in the same way
hipError_t launch_track7_mask(hipStream_t st, const TrkArgs &a, const TrkFramesArgs &b, const TrkMaskArgs &mk, float *x,
                              float *y, int *v, int n, int grid, bool two, const char **name);
// the multi-sequence instances (whole-frame interleaved pyramids, exact sums)
hipError_t launch_track7_multi(hipStream_t st, const TrkArgs &a, const TrkFramesArgs &b, const TrkMultiArgs &m, float *x,
                               float *y, int *v, int n, const char **name = nullptr);
// The balanced layout of the processing order (k_band_order, klt_hip_order_slot).
// The trackers take blocks XCD-major, so XCD x processes the slots of segment
// x, [min(x S, n), min((x + 1) S, n)) with S = seg.  Live features keep their
// band order and fill the head of each segment in shares proportional to its
// capacity, lost features fill the rest: the waves that leave at once are
// spread over all eight XCDs instead of emptying the last ones.
constexpr int kXcds = 8;
// live[x]: live rank at which segment x starts, B_x = floor(n_live * min(x S, n) / n)
// lost[x]: lost rank at which it starts, the prefix sum of capacity - live share
__host__ __device__ __forceinline__ int order_seg_start(int n, int seg, int x) {
  const long e = (long)x * seg;
  return e < n ? (int)e : n;
}
__host__ __device__ __forceinline__ int order_live_start(int n, int seg, int n_live, int x) {
  return n > 0 ? (int)((unsigned long long)n_live * (unsigned)order_seg_start(n, seg, x) / (unsigned)n) : 0;
}
__host__ __device__ __forceinline__ int order_lost_start(int n, int seg, int n_live, int x) {
  return order_seg_start(n, seg, x) - order_live_start(n, seg, n_live, x);
}
// the slot of live rank `rank` (lost = false) or lost rank `rank` (true),
// given the eight segment starts of its kind and the live starts
__host__ __device__ __forceinline__ int order_slot_of(const int *live, const int *lost_st, int seg, int rank,
                                                      bool lost) {
  const int *st = lost ? lost_st : live;
  // the last segment that starts at or before the rank (the starts never
  // decrease, and an empty segment starts where the next one does); constant
  // indices only, so that the starts can live in registers
  int x = 0, start = st[0], head = live[1] - live[0];
#pragma unroll
  for (int k = 1; k < kXcds; ++k) {
    const bool in = rank >= st[k];
    x = in ? k : x;
    start = in ? st[k] : start;
    head = in ? live[k + 1] - live[k] : head;
  }
  return x * seg + (lost ? head : 0) + (rank - start);  // a segment's lost features follow its live ones
}

// band-sorted processing order (one workgroup); count != nullptr: keep only
// live features with own_lo <= y < own_hi and store how many.  seg > 0 (and
// count == nullptr): the balanced layout over segments of seg slots; 0: live
// features in band order, lost features last
hipError_t launch_band_order(hipStream_t st, const float *fy, const int *fv, int n, int nrows, int *perm,
                             float own_lo, float own_hi, int *count, int seg);

hipError_t launch_affine(hipStream_t st, const AffArgs &a);

// runtime.hip: record a failure in the context's error message (klt_hip_last_error); returns -1
int ctx_fail(klt_hip_ctx *c, const char *fmt, ...);
// runtime.hip: the exit hook has run (graphs released, sort pool joined): no
// new selection graphs may be built or launched
bool lib_exiting();

// select.hip: exact lazy selection (the reference's quicksort order) with the
// top-level partition steps on the device
struct SelEngine;
constexpr int kSelDefaultThreshold = 49152;  // map points: longer segments are split on the device (tools/exp/r04ah.sh)
SelEngine *sel_engine_create();
void sel_engine_destroy(SelEngine *e);
void sel_engine_release_graphs(SelEngine *e);  // exit hook: the captured graphs before the code object goes
void sel_pool_shutdown();                       // exit hook: join the host sort pool's workers
void sel_engine_set_threshold(SelEngine *e, int threshold);
int sel_default_threshold();
void sel_engine_stats(const SelEngine *e, long *downloaded, long *steps, long *visited, double *us);
int sel_engine_run(SelEngine *e, hipStream_t st, const int *dev_vals, int nx, int ny, int bx, int by, int step,
                   int W, int H, int mindist, int min_eigenvalue, int overwrite_all, float *x, float *y, int *val,
                   unsigned char *changed, int n, const uint8_t *mask, long mask_pitch, std::string *err);
int sel_engine_sort(SelEngine *e, hipStream_t st, const int *dev_vals, int n, int *out_val, int *out_idx,
                    std::string *err);
hipError_t launch_affine_move(hipStream_t st, int dir, const int *idx, int m, int s3, float *staging, float *store);

}  // namespace kltdev
