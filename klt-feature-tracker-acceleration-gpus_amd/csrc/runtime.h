// runtime.h -- what the units of the host runtime share (internal): the device
// context and what it is made of, the helpers every unit uses, and the
// functions one unit calls in another (klt_dev.h lists the units).
#pragma once

#include <sys/resource.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "host_pool.h"
#include "klt_dev.h"
#include "klt_hip.h"

#define KLT_API extern "C" __attribute__((visibility("default")))

// klt_hip_set_lazy_grad's default ("Level-0 gradients in the tracker")
#ifndef KLT_LAZY_GRAD_DEFAULT
#define KLT_LAZY_GRAD_DEFAULT 1
#endif

using namespace kltdev;

// runtime_track.hip (exported, as before the split)
int feat_stage_in(klt_hip_ctx *c, const float *x, const float *y, const int *val, int n);
int feat_unpack(klt_hip_ctx *c, float *x, float *y, int *val, int n);

// everything below is internal to the library: no dynamic symbols
#pragma GCC visibility push(hidden)

// A level's storage is one block of 3 * cap floats, img | gx | gy.  Built by
// the fused kernels it holds the level interleaved (il: {gx, gy, img} per
// pixel from img on, the form the default tracker reads); built by the
// generic one-pass kernels it holds the three planes at img, gx and gy.
struct Level {
  int w = 0, h = 0;
  float *img = nullptr, *gx = nullptr, *gy = nullptr;  // gx = img + cap, gy = img + 2 cap
  size_t cap = 0;  // floats per plane
  int il = 0;      // contents: kLayoutPlanes, kLayoutRec (interleaved) or kLayoutImg (the img plane alone)
};

// a slot's level, or frame f of a bank's (interleaved levels: img is the
// frame's interleaved base, gx/gy null)
inline TrkLevel level_view(const Level &L, long f = 0, int vlo = 0, int vhi = 1 << 30) {
  const long n = (long)L.w * L.h;
  if (L.il == kLayoutImg) return TrkLevel{L.img + f * n, nullptr, nullptr, L.w, L.h, vlo, vhi, kLayoutImg};
  if (L.il) return TrkLevel{L.img + 3 * f * n, nullptr, nullptr, L.w, L.h, vlo, vhi, 1};
  return TrkLevel{L.img + f * n, L.gx + f * n, L.gy + f * n, L.w, L.h, vlo, vhi, 0};
}

struct Slot {
  int nlev = 0;
  int ss = 1;
  int fused = -1;
  Level lv[KLT_HIP_MAX_LEVELS];
};

enum TimerClass { T_L0 = 0, T_L1, T_TRACK, T_EIG, T_GEN, T_N };

// a batch of same-size pyramids: plane l of frame f at lv[l].img + f * w*h
struct Bank {
  int frames = 0;  // capacity in frames
  int nlev = 0;
  int ss = 1;
  Level lv[KLT_HIP_MAX_LEVELS];
  float *hs = nullptr;  // per-frame row pass of the sigma-3.6 smoothing (fused path)
  size_t hs_cap = 0;
  int vlo[KLT_HIP_MAX_LEVELS] = {}, vhi[KLT_HIP_MAX_LEVELS] = {};  // rows built (band mode: a subset)

  // What the bank holds after a build, called by every build and by nothing
  // else: level 0 in layout il, the levels above interleaved under an
  // image-only level 0 and in il otherwise, and the valid rows of every level
  // (null: whole frames).  The only writer of a bank level's il and of vlo / vhi.
  void holds(int il, const int *lo = nullptr, const int *hi = nullptr) {
    for (int l = 0; l < nlev; ++l) {
      lv[l].il = l > 0 && il == kLayoutImg ? kLayoutRec : il;
      vlo[l] = lo ? lo[l] : 0;
      vhi[l] = hi ? hi[l] : 1 << 30;
    }
  }
  // frame f of level l with its valid rows
  TrkLevel level(int l, long f) const { return level_view(lv[l], f, vlo[l], vhi[l]); }
};

// a bank whose pyramids a band call built ahead, during its own tracking, for
// the next call (klt_hip_track_frames_band's next_frames); bank -1: none
struct BuiltAhead {
  int bank = -1, F = 0, row_lo = 0, row_hi = 0, il = 1;
  const unsigned char *src = nullptr;
  long stride = 0;
  bool same(const BuiltAhead &o) const {
    return F == o.F && row_lo == o.row_lo && row_hi == o.row_hi && il == o.il && src == o.src && stride == o.stride;
  }
};

// The three banks of the batched calls, taken in turn ("Banks").
// ensure_banks / free_banks (runtime_pyr.hip) lay them out; take, peek,
// built_ahead and drop_ahead are the only code that touches next and pre;
// Bank::holds records every build.
struct BankRing {
  Bank bank[3];  // views into arena
  void *arena = nullptr;
  size_t arena_bytes = 0;
  int next = 0;
  BuiltAhead pre;
  hipEvent_t ev_built[3] = {}, ev_free[3] = {};

  // the next bank in turn.  A build-ahead record for it goes: the bank is
  // taken as built (*prebuilt, when it holds what `want` describes) or is
  // about to be overwritten
  int take(const BuiltAhead *want = nullptr, bool *prebuilt = nullptr) {
    const int bi = next;
    next = (bi + 1) % 3;
    if (prebuilt) *prebuilt = want && pre.bank == bi && pre.same(*want);
    if (pre.bank == bi) pre.bank = -1;
    return bi;
  }
  int peek() const { return next; }  // the bank the next take() returns: a build-ahead's
  void built_ahead(const BuiltAhead &b) { pre = b; }
  bool drop_ahead() {  // the record goes (the banks are laid out again, or change hands); true: there was one
    const bool was = pre.bank >= 0;
    pre.bank = -1;
    return was;
  }
};

// where the pyramid preceding the next batch lives
struct PrevRef {
  int bank = -1;  // -1: pyramid slot `slot`
  int frame = 0;
  int slot = KLT_HIP_MAX_SLOTS;  // the batch seed slot unless klt_hip_frames_begin_slot
};

// klt_hip_set_frames_overlap's values
enum { kSchedOne = 0, kSchedAuto = 1, kSchedBeside = 2, kSchedTail = 3 };
// klt_hip_set_frames_tail's default: four of a SIMD's five lazy-gradient
// tracker waves (256 CUs x 4 SIMDs).  1080p / 5000, headline frames/s over
// one stream with the lost features last in the processing order: K = 512
// 1.00, 1024 1.03, 2048 1.05, 3072 and 3584 1.06; 4096 and 4608 1.07 in the
// median but with single runs back at one stream's speed
// (profiles/sched_tail_bound.txt).  With the balanced order every SIMD frees
// registers as features die, and over K = 3072: 2048 1.00, 3584 1.01-1.02,
// 4096 1.02-1.03 with its slowest run above 3072's fastest in both sweeps,
// 4608 1.02 with one low run, no wait at all 0.87
// (profiles/order_balance_headline_ab.txt)
constexpr int kTailLeftDefault = 4096;
// the exit counter is re-based (at a drained point) once it has passed this;
// past it, and for launches of this many features, no launch counts, so the
// count stays below 2^31 whatever the call's length
constexpr unsigned kExitsRebase = 1u << 29;

struct __attribute__((visibility("default"))) klt_hip_ctx {  // its constructor is a dynamic symbol, as before the split
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t pstream = nullptr;  // pyramid stream of the pipelined sequence
  hipEvent_t ev_built[KLT_HIP_MAX_SLOTS] = {};
  hipEvent_t ev_free[KLT_HIP_MAX_SLOTS] = {};
  hipEvent_t ev_start = nullptr;
  // a caller's stream (klt_hip_set_stream): ev_caller is recorded on it when
  // the context switches away from it, so a reset or destroy can wait for the
  // work queued there even after the caller has destroyed the stream
  hipEvent_t ev_caller = nullptr;
  bool caller_pending = false;
  Slot slot[KLT_HIP_MAX_SLOTS + 2];  // + the batch seed and scratch slots
  uint8_t *d_u8[2] = {nullptr, nullptr};
  uint8_t *h_u8[2] = {nullptr, nullptr};
  hipEvent_t u8_done[2] = {nullptr, nullptr};
  size_t u8_cap = 0;
  int u8_w[2] = {0, 0}, u8_h[2] = {0, 0};
  float *d_hs = nullptr;
  size_t hs_cap = 0;
  float *d_tmp[2] = {nullptr, nullptr};
  size_t tmp_cap[2] = {0, 0};
  // host-array tracking (klt.h calls): x | y | val in one device block and one
  // pinned host block, so a call moves its feature list in one copy each way
  float *d_fx = nullptr, *d_fy = nullptr;  // views into d_feat
  int *d_fv = nullptr;
  float *d_feat = nullptr, *h_feat = nullptr;
  // klt_hip_track on host lists: 2 (default) two copy kernels move the pinned
  // block h_feat to d_feat and back around the tracker (no copy engine, no
  // copy-to-kernel hand-off, and the tracker's gathers of x/y/val stay on the
  // device: 111 against 130 us per registered 1080p/5000 call); 1 the kernels
  // use h_feat in place over the bus; 0 copy-engine copies
  int feat_mode = 2;
  size_t f_cap = 0;
  int *d_eig = nullptr;
  size_t eig_cap = 0;
  SelEngine *sel = nullptr;  // select.hip: the lazy exact selection
  // caller buffers registered with klt_hip_register_host (page-locked): frame
  // uploads from inside one are one DMA from the caller's pages, no staging
  std::vector<std::pair<const unsigned char *, size_t>> registered;
  // affine consistency check: stored windows (3*aff_S floats per feature) and per-call arrays
  float *d_aff_store = nullptr;
  size_t aff_store_cap = 0;
  int aff_S = 0;
  float *d_aff = nullptr, *d_xp = nullptr, *d_yp = nullptr, *d_astage = nullptr;
  size_t aff_cap = 0, xp_cap = 0, yp_cap = 0, astage_cap = 0;
  int *d_astate = nullptr, *d_aidx = nullptr;
  size_t astate_cap = 0, aidx_cap = 0;
  std::string err;
  int force_generic = 0;
  // klt_hip_set_frame_format: the pixels of device frames (KLT_HIP_FRAME_*).
  // Read where a caller's device frame enters a pyramid build (build_pyramid_on
  // with a frame, build_fused_bank); the host-frame paths hold it at gray
  // for their own device copies (GrayFrames)
  int frame_format = KLT_HIP_FRAME_GRAY8;
  int track_order = 0;  // 0: band-sorted, XCD-major processing order; 1: input order
  int track_patch = 1;  // one-feature waves gather through a lane patch when the window fits
  int track_merge = 1;   // defer finest-level residues into the next frame's first pass (ResCarry)
  int l0_strip = 1;  // klt_hip_set_l0_strip: the image-only level 0 of whole frames as k_pyr_l0s
  int lazy_grad = KLT_LAZY_GRAD_DEFAULT;  // klt_hip_set_lazy_grad: image-only level 0 in the banks of plain batched calls
  RTaps lazy_gg, lazy_gd;  // the gradient taps of the last such call (a kept image-only frame is made whole with them)
  int track_prio = 1;    // tracker waves at issue priority 3 (klt_hip_set_track_prio)
  // planes of interleaved levels for the kernels that read planes (the generic
  // tracker, the affine check): [0] image 1, [1] image 2 (a batch of frames)
  float *pl_scr[2][KLT_HIP_MAX_LEVELS] = {};
  size_t pl_cap[2][KLT_HIP_MAX_LEVELS] = {};
  int track_impl = 0;    // 0: track7.hip for the default configuration, 1: the generic k_track_frames_g
  const char *track_kernel = nullptr;  // instance name of the last tracker launch (klt_hip_track_kernel)
  // forward-backward check (klt_hip_set_fb): off by default; the optional
  // device table of squared return distances (klt_hip_set_fb_table)
  int fb_on = 0;
  float fb_dist = 0.0f;
  float *fb_tab = nullptr;
  long fb_stride = 0;
  // motion prior (klt_hip_set_predict): off by default; the caller's device
  // state arrays, the optional device tables (klt_hip_set_predict_table), and
  // the staging of klt_hip_track_frames_host (vx | vy)
  int pred_on = 0;
  float *pred_vx = nullptr, *pred_vy = nullptr;
  float *pred_tvx = nullptr, *pred_tvy = nullptr;
  long pred_stride = 0;
  float *d_pred = nullptr;
  size_t pred_cap = 0;
  // region mask (klt_hip_set_mask): the caller's device bytes, their row
  // pitch and the uses switched on (KLT_HIP_MASK_*); null / 0: none
  const unsigned char *mask = nullptr;
  long mask_pitch = 0;
  int mask_flags = 0;
  // affine check inside the tracker launch (klt_hip_set_frames_affine): the
  // caller's device arrays, the optional tables (klt_hip_set_affine_table);
  // aff_fresh: the next tracker launch is the first of its API call (windows
  // held on entry are state 1), aff_depth: nesting of the entry points
  int aff_on = 0;
  AffParams aff_p{};
  float *aff_dev = nullptr;
  int *aff_state_dev = nullptr;
  float *aff_tab = nullptr;
  int *aff_stab = nullptr;
  long aff_tab_stride = 0;
  int aff_fresh = 1, aff_depth = 0;
  // replacement of lost features inside the batched calls
  // (klt_hip_set_frames_replace): the counters since it was turned on, the
  // slots a replacement has written, the map and the pinned list (x | y | val)
  int rep_on = 0;
  klt_hip_replace_desc rep{};
  long rep_frames = 0, rep_runs = 0, rep_filled = 0;
  std::vector<unsigned char> rep_changed;
  int *d_rep_map = nullptr;
  size_t rep_map_cap = 0;
  float *h_rep = nullptr;
  size_t h_rep_cap = 0;  // features
  hipEvent_t ev_rep = nullptr;
  const char *eig_kernel = nullptr;  // instance name of the last map launch (klt_hip_eigen_kernel)
  // band calls: 1 = the next chunk's frames are ready when the call is made
  // (not written by work still queued on the tracking stream), so its
  // build-ahead waits for its bank and for this chunk's processing order
  // (ev_go: the pyramids start with the tracker) -- not for whatever the
  // caller queues between two chunks (klt_hip_set_ahead_ready)
  int ahead_ready = 0;
  hipEvent_t ev_go = nullptr;
  // klt_hip_set_frames_overlap: the schedule of a plain batched call that spans
  // several chunks (kSchedOne .. kSchedTail; plan_frames states the rule
  // behind kSchedAuto)
  int frames_sched = 0;
  // the tail schedule: the next chunk's build is released when at most this
  // many waves of the running tracker are left (klt_hip_set_frames_tail)
  int tail_left = kTailLeftDefault;
  // the tracker waves that have left, all launches of this context that were
  // asked to count (TrkFramesArgs::exits, device memory), and the 8-byte signal
  // allocation the pyramid stream waits on, which receives the count each time
  // it reaches a launch's threshold; exits_base is the count once everything
  // enqueued so far has run
  unsigned *d_exits = nullptr, *d_exit_sig = nullptr;
  unsigned exits_base = 0;
  unsigned long long *wave_t = nullptr;  // klt_hip_set_wave_times: TrkFramesArgs::wave_t of k_track7 launches
  int *d_perm = nullptr;
  size_t perm_cap = 0;
  int perm_n = -1, perm_age = 0;  // features of the order in d_perm (-1: none), frames tracked with it
  int *d_count = nullptr;  // band mode: features owned in this chunk
  unsigned long long *d_trk_count = nullptr;  // klt_hip_set_track_count: {solves, passes}, null when off
  // klt_hip_track_frames_host: frames uploaded chunk by chunk.  Two slots per
  // stage: pinned staging (filled by the pool), the device ring (one DMA per
  // chunk on cstream), device table rows (written by the tracker) and pinned
  // table rows (one D2H per chunk on dstream, then handed to the caller)
  unsigned char *d_ring = nullptr, *h_stage = nullptr;
  float *d_rows = nullptr, *h_rows = nullptr;
  size_t ring_cap = 0, stage_cap = 0, drows_cap = 0, hrows_cap = 0;  // bytes
  hipStream_t cstream = nullptr, dstream = nullptr;
  hipEvent_t ev_ring_free[2] = {}, ev_dma[2] = {}, ev_tracked[2] = {}, ev_rows[2] = {};
  HostPool *pool = nullptr;
  int copy_threads = default_host_threads();  // pool workers besides the caller (0: the caller alone)
  unsigned long long *prof = nullptr;  // instrumented build: per-wave tracker phase counters
  BankRing banks;
  size_t bank_budget = 0;  // bytes the bank arena may take (klt_hip_set_bank_budget; 0: the default)
  size_t dev_total = 0;    // the device's memory (queried once, for the default budget)
  int chunk_used = 0;      // frames per bank of the last klt_hip_track_frames* call (budget-capped)
  PrevRef prev;            // the kept pyramid (prev_level, kept_* below), current while frames_ready
  bool frames_ready = false;
  bool timing = false;
  long frames_timed[T_N] = {};
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used[T_N];
};

constexpr auto fail = &kltdev::ctx_fail;

#define HIPCHK(c, expr)                                                                \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail((c), "%s: %s", #expr, hipGetErrorString(e_));    \
  } while (0)

inline double wall_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

inline int use_device(klt_hip_ctx *c) {
  HIPCHK(c, hipSetDevice(c->device));
  return 0;
}

template <class T>
int grow(klt_hip_ctx *c, T **p, size_t *cap, size_t n) {
  if (*cap >= n && *p) return 0;
  if (*p) HIPCHK(c, hipFree(*p));
  *p = nullptr;
  HIPCHK(c, hipMalloc((void **)p, sizeof(T) * (n ? n : 1)));
  *cap = n;
  return 0;
}

inline hipEvent_t take_event(klt_hip_ctx *c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

#ifdef KLT_HOST_PROF  // experiment builds: CLOCK_MONOTONIC marks through one call, printed to stderr
struct HostMarks {
  long t[32];
  const char *what[32];
  int n = 0;
  void mark(const char *w) {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    if (n < 32) {
      t[n] = ts.tv_sec * 1000000000L + ts.tv_nsec;
      what[n++] = w;
    }
  }
  HostMarks();
  ~HostMarks() {
    cur() = nullptr;
    for (int i = 1; i < n; ++i) fprintf(stderr, "hostmark %s %.2f us\n", what[i], (t[i] - t[i - 1]) * 1e-3);
    if (n) fprintf(stderr, "hostmark enter_ns %ld\n", t[0]);
  }
  static HostMarks *&cur() {
    static thread_local HostMarks *p = nullptr;
    return p;
  }
};
inline HostMarks::HostMarks() { cur() = this; }
#define HMARK(w) hm_.mark(w)
#define HMARK_IN(w) \
  if (HostMarks::cur()) HostMarks::cur()->mark(w)
#else
#define HMARK(w) (void)0
#define HMARK_IN(w) (void)0
#endif

// HIP events around one launch, recorded on the stream the kernel runs on
struct TimedScope {
  klt_hip_ctx *c;
  int cls;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  TimedScope(klt_hip_ctx *c_, int cls_, hipStream_t st_, int frames = 1) : c(c_), cls(cls_), st(st_) {
    if (!c->timing) return;
    c->frames_timed[cls] += frames;
    a = take_event(c);
    b = take_event(c);
    if (a) hipEventRecord(a, st);
  }
  ~TimedScope() {
    if (!c->timing || !a || !b) return;
    hipEventRecord(b, st);
    c->ev_used[cls].push_back({a, b});
  }
};

// the context's host pool, created on first use (thread creation can throw:
// no exception crosses an extern "C" entry; without a pool the caller works alone)
inline void ensure_pool(klt_hip_ctx *c) {
  if (c->pool || c->copy_threads <= 0) return;
  try {
    c->pool = new HostPool(c->copy_threads);
  } catch (...) {
    c->pool = nullptr;
    c->copy_threads = 0;
  }
}

template <class Fn>
int host_parallel(klt_hip_ctx *c, size_t n, Fn fn) {
  try {
    if (c->pool) {
      const std::function<void(size_t)> f = fn;
      c->pool->parallel(n, f);
    } else {
      for (size_t i = 0; i < n; ++i) fn(i);
    }
  } catch (...) {
    return fail(c, "track_frames_host: host task failed (out of memory?)");
  }
  return 0;
}

inline int launched(klt_hip_ctx *c, const char *what, hipError_t e) {
  if (e != hipSuccess) return fail(c, "launch %s: %s", what, hipGetErrorString(e));
  return 0;
}

// the pinned list of a replacement inside a batched call (x | y | val of n
// features at c->h_rep) and the event its download is waited for
inline int ensure_rep_host(klt_hip_ctx *c, int n, hipStream_t st) {
  if (c->h_rep_cap < (size_t)n || !c->h_rep) {
    if (c->h_rep) {
      HIPCHK(c, hipStreamSynchronize(st));  // no copy still uses the old block
      HIPCHK(c, hipHostFree(c->h_rep));
    }
    c->h_rep = nullptr;
    c->h_rep_cap = 0;
    HIPCHK(c, hipHostMalloc((void **)&c->h_rep, 3 * sizeof(float) * (size_t)n, hipHostMallocDefault));
    c->h_rep_cap = (size_t)n;
  }
  if (!c->ev_rep) HIPCHK(c, hipEventCreateWithFlags(&c->ev_rep, hipEventDisableTiming));
  return 0;
}

// an entry point that tracks: the first tracker launch inside the outermost
// one is the call's first (TrkAffArgs::fresh)
struct AffCall {
  klt_hip_ctx *c;
  explicit AffCall(klt_hip_ctx *ctx) : c(ctx) {
    if (c && c->aff_depth++ == 0) c->aff_fresh = 1;
  }
  ~AffCall() {
    if (c) --c->aff_depth;
  }
};

// a host-frame entry point: its device copies of the caller's frames are gray
// whatever klt_hip_set_frame_format says
struct GrayFrames {
  klt_hip_ctx *c;
  int saved;
  explicit GrayFrames(klt_hip_ctx *ctx) : c(ctx), saved(ctx ? ctx->frame_format : 0) {
    if (c) c->frame_format = KLT_HIP_FRAME_GRAY8;
  }
  ~GrayFrames() {
    if (c) c->frame_format = saved;
  }
};

// the fused level-0 kernels' vectorised loads: base, row pitch and frame stride
// (bytes) 4-byte aligned, and whole 4-pixel groups (any pixel size: 4 pixels
// are 4, 12 or 16 bytes)
inline int vec_u8_ok(const uint8_t *src, long pitch, long stride, int W) {
  return (W % 4 == 0 && W >= 16 && pitch % 4 == 0 && stride % 4 == 0 && ((uintptr_t)src & 3) == 0) ? 1 : 0;
}

// track_frames_launch: ordered: the caller ran order_features into b already;
// fb_row: the forward-backward / affine table row of this launch's first
// frame; tail: non-null asks for the exit count (the tail schedule)
struct TailRelease {
  unsigned left;  // in: the waves that may still be running at the release
  bool wait;      // out: the launch counts, and c->d_exit_sig reaches thr when only `left` of its waves remain
  unsigned thr;
};

// the region mask as the selection engine takes it (null unless the selection
// bit is on), and the check of the calls that learn the image width: a mask
// whose rows are shorter than the image's is refused before any launch
inline const unsigned char *sel_mask(const klt_hip_ctx *c) {
  return (c->mask_flags & KLT_HIP_MASK_SELECT) ? c->mask : nullptr;
}
inline bool mask_tracks(const klt_hip_ctx *c) { return (c->mask_flags & KLT_HIP_MASK_TRACK) != 0; }
inline int mask_refused(klt_hip_ctx *c, int ncols, const char *who) {
  if (!c->mask_flags || c->mask_pitch >= ncols) return 0;
  return fail(c, "%s: region mask pitch %ld < image width %d (klt_hip_set_mask)", who, c->mask_pitch, ncols);
}

// The kept pyramid: the one the next batched call starts from, in a slot or a
// frame of a bank (c->prev).  Level l, its depth and subsampling, and whether
// its level 0 is the img plane alone (klt_hip_set_lazy_grad).
inline TrkLevel prev_level(const klt_hip_ctx *c, int l) {
  return c->prev.bank < 0 ? level_view(c->slot[c->prev.slot].lv[l]) : c->banks.bank[c->prev.bank].level(l, c->prev.frame);
}
inline int kept_nlev(const klt_hip_ctx *c) {
  return c->prev.bank < 0 ? c->slot[c->prev.slot].nlev : c->banks.bank[c->prev.bank].nlev;
}
inline int kept_ss(const klt_hip_ctx *c) {
  return c->prev.bank < 0 ? c->slot[c->prev.slot].ss : c->banks.bank[c->prev.bank].ss;
}
inline bool kept_image_only(const klt_hip_ctx *c) { return prev_level(c, 0).il == kLayoutImg; }  // slots hold whole levels

// the selection grid over a w x h image: every step-th pixel inside the
// borders, and the window's half sizes
struct SelGrid {
  int nx, ny, step, hw, hh;
};
inline int sel_step(const klt_hip_select_desc &d) { return d.nSkippedPixels + 1; }
inline SelGrid sel_grid(const klt_hip_select_desc &d, int w, int h) {
  const int step = sel_step(d), cx = w - 2 * d.borderx, cy = h - 2 * d.bordery;
  const bool ok = step > 0;  // the callers refuse step < 1
  return SelGrid{ok && cx > 0 ? (cx + step - 1) / step : 0, ok && cy > 0 ? (cy + step - 1) / step : 0, step,
                 d.window_width / 2, d.window_height / 2};
}

// runtime.hip
int ensure_pipeline(klt_hip_ctx *c);
int forget_kept(klt_hip_ctx *c);  // no current pyramid and no build-ahead from here on
// runtime_pyr.hip
bool fused_ok(const klt_hip_pyr_desc *d);
int ensure_slot(klt_hip_ctx *c, int s, const klt_hip_pyr_desc *d);
int build_pyramid_on(klt_hip_ctx *c, int s, const klt_hip_pyr_desc *d, const unsigned char *frame, long pitch,
                     int buf, hipStream_t st);
size_t bank_arena_bytes(const klt_hip_pyr_desc *d, int frames);
void free_banks(klt_hip_ctx *c);
size_t bank_budget_of(klt_hip_ctx *c);
int budget_chunk(klt_hip_ctx *c, const klt_hip_pyr_desc *d);
bool banks_fit(const klt_hip_ctx *c, const klt_hip_pyr_desc *d, int frames);
int ensure_banks(klt_hip_ctx *c, const klt_hip_pyr_desc *d, int frames);
int build_fused_bank(klt_hip_ctx *c, Bank &K, const klt_hip_pyr_desc *d, const uint8_t *src, long pitch,
                     long stride, int F, hipStream_t st, int row_lo = 0, int row_hi = 1 << 30, int plane_lo = 0,
                     int plane_hi = 1 << 30, int il = 1, long first = 0, long step = 1);
// runtime_frames.hip
int tables_refused(klt_hip_ctx *c, const char *who, const float *tab_x, const float *tab_y, const int *tab_val,
                   long tab_stride, int n, long pitch, int ncols);  // the table arrays and the frames' pitch
int replace_desc_refused(klt_hip_ctx *c, const klt_hip_replace_desc *d, const char *who);  // klt_hip_set_frames_replace's checks
// runtime_track.hip
int check_window(klt_hip_ctx *c, const klt_hip_track_desc *d);
void fill_trk_args(const klt_hip_track_desc *d, int nlev, int ss, int ncols, int nrows, TrkArgs &a);
bool t7_tracks(const klt_hip_ctx *c, const klt_hip_track_desc *d);
int order_features(klt_hip_ctx *c, hipStream_t st, int nrows, const float *y, const int *v, int n, int nframes,
                   const float *own, TrkFramesArgs &bb);
int fb_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, const char *who);
int aff_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, int n, const char *who);
int pred_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, const char *who);
int mask_track_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, const char *who);
int track_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, int n, const char *who);
int track_frames_launch(klt_hip_ctx *c, hipStream_t st, const klt_hip_track_desc *d, const TrkArgs &a,
                        const TrkFramesArgs &b, float *x, float *y, int *v, int n, const float *own = nullptr,
                        bool ordered = false, long fb_row = 0, TailRelease *tail = nullptr);
#pragma GCC visibility pop
