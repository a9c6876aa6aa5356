// runtime_frames.hip -- host side of libklt_amd.so: the batched calls
// (klt_hip_track_frames, _host, _band), their schedule, and the pyramid kept
// from one call to the next (runtime.h).  No kernels here.
#include "replace_step.h"

// A/B in one tree: KLT_FRAMES_SCHED=0..3 replaces whatever
// klt_hip_set_frames_overlap was given, KLT_FRAMES_TAIL=K whatever
// klt_hip_set_frames_tail was (-1: not set)
static int env_frames_sched() {
  static const int v = [] {
    const char *e = getenv("KLT_FRAMES_SCHED");
    return e && *e >= '0' && *e <= '3' && !e[1] ? *e - '0' : -1;
  }();
  return v;
}
static int env_frames_tail() {
  static const int v = [] {
    const char *e = getenv("KLT_FRAMES_TAIL");
    const long x = e && *e ? atol(e) : -1;
    return (int)(x < 0 ? -1 : x > (1 << 30) ? (1 << 30) : x);
  }();
  return v;
}

namespace {
bool seq_trace() {
  static const bool t = getenv("KLT_SEQ_TRACE") && atoi(getenv("KLT_SEQ_TRACE")) != 0;
  return t;
}

// KLT_SEQ_TRACE's stage clock for klt_hip_track_frames_host: every interval
// between two marks is charged to the stage named by the later mark, so the
// stages add up to the whole call; each stage also gets the process's and the
// calling thread's minor page faults over its intervals (a call
// with 2 057 faults and 5.5 ms outside the four stages traced then)
struct SeqStages {
  enum { PRE, WAIT_DMA, COPY, LAUNCH, WAIT_ROWS, DELIVER, TAIL, N };
  bool on = false;
  double t = 0, t0 = 0, us[N] = {};
  long pf = 0, tf = 0, pfl[N] = {}, tfl[N] = {};
  static void faults(long &proc, long &thr) {
    rusage r{};
    getrusage(RUSAGE_SELF, &r);
    proc = r.ru_minflt;
    getrusage(RUSAGE_THREAD, &r);
    thr = r.ru_minflt;
  }
  void start(bool enabled) {
    on = enabled;
    if (!on) return;
    t = t0 = wall_us();
    faults(pf, tf);
  }
  void mark(int stage) {
    if (!on) return;
    const double now = wall_us();
    long p, q;
    faults(p, q);
    us[stage] += now - t;
    pfl[stage] += p - pf;
    tfl[stage] += q - tf;
    t = now;
    pf = p;
    tf = q;
  }
  void print(int nframes, int nchunks, int threads) const {
    if (!on) return;
    static const char *name[N] = {"pre", "wait_dma", "stage_copy", "launch", "wait_rows", "deliver", "tail"};
    char buf[1024];
    int k = snprintf(buf, sizeof buf, "seqtrace frames=%d chunks=%d threads=%d total_us=%.0f", nframes, nchunks,
                     threads, t - t0);
    for (int i = 0; i < N && k < (int)sizeof buf; ++i)
      k += snprintf(buf + k, sizeof buf - k, " %s_us=%.0f %s_pf=%ld %s_tf=%ld", name[i], us[i], name[i], pfl[i],
                    name[i], tfl[i]);
    fprintf(stderr, "%s\n", buf);
  }
};
}  // namespace

// ---------------------------------------------------------------------------
// batched frames: pyramids of `chunk` frames per pair of launches into one of
// three banks on the pyramid stream, one k_track_frames launch per chunk on
// the tracking stream.  Bank k is rebuilt only after the chunk that used its
// last frame as the previous pyramid has been tracked (banks.ev_free[k]).
// ---------------------------------------------------------------------------

namespace {
constexpr int kSeedSlot = KLT_HIP_MAX_SLOTS, kScratchSlot = KLT_HIP_MAX_SLOTS + 1;

// one level (a view: a slot's, or a bank frame's) into frame f of level `to`
// (a slot's: f = 0), in the view's layout; what `to` holds is its owner's to
// record (slot_level below, Bank::holds)
int copy_level(klt_hip_ctx *c, const TrkLevel &from, Level &to, long f, hipStream_t st) {
  const size_t n = (size_t)from.w * from.h, b = sizeof(float) * n;
  if (!b) return 0;
  if (from.il) {
    HIPCHK(c, hipMemcpyAsync(to.img + 3 * f * n, from.img, 3 * b, hipMemcpyDeviceToDevice, st));
  } else {
    HIPCHK(c, hipMemcpyAsync(to.img + f * n, from.img, b, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(to.gx + f * n, from.gx, b, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(to.gy + f * n, from.gy, b, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

// a level of the kept pyramid into a slot's, which holds it in that layout
int slot_level(klt_hip_ctx *c, const TrkLevel &from, Level &to, hipStream_t st) {
  to.il = from.il;
  return copy_level(c, from, to, 0, st);
}

// a klt_hip_pyr_desc shaped like the kept pyramid (the sizes ensure_slot
// reads); *ss: its subsampling as kept (1 for a single level)
klt_hip_pyr_desc prev_desc(klt_hip_ctx *c, int *ss) {
  const TrkLevel p0 = prev_level(c, 0);
  *ss = kept_ss(c);
  klt_hip_pyr_desc d;
  memset(&d, 0, sizeof d);
  d.ncols = p0.w;
  d.nrows = p0.h;
  d.nlevels = kept_nlev(c);
  d.subsampling = *ss > 1 ? *ss : 2;
  return d;
}

// the kept pyramid's levels from `from` up move out of their bank into the
// seed slot (sized by the caller: ensure_slot), which is the kept pyramid from
// here on
int prev_to_seed(klt_hip_ctx *c, int from, hipStream_t st) {
  Slot &S = c->slot[kSeedSlot];
  for (int l = from; l < S.nlev; ++l)
    if (slot_level(c, prev_level(c, l), S.lv[l], st)) return -1;
  c->prev = PrevRef{-1, 0, kSeedSlot};
  return 0;
}

// The kept pyramid made whole.  After a call whose banks hold level 0 as the
// img plane alone (klt_hip_set_lazy_grad) the previous pyramid has no level-0
// gradients; a reader that needs them -- a call in another layout, the copy
// into a slot, the selection map -- first gets that one frame as a full
// pyramid in the seed slot: level 0's gx / gy from its img with the generic
// row and column kernels (the same values as the fused kernels', bit for bit:
// tests/test_gpu_pyramid.py), interleaved into records like a fused slot's,
// the levels above copied.  On the tracking stream, which has already waited
// for the bank's build.
int prev_full(klt_hip_ctx *c) {
  if (!kept_image_only(c)) return 0;
  const TrkLevel p0 = prev_level(c, 0);
  int ss = 1;
  const klt_hip_pyr_desc d = prev_desc(c, &ss);
  if (ensure_slot(c, kSeedSlot, &d)) return -1;
  Slot &S = c->slot[kSeedSlot];
  S.ss = ss;
  S.fused = 1;
  hipStream_t st = c->stream;
  const long n0 = (long)p0.w * p0.h;
  if (n0 > 0) {
    if (grow(c, &c->d_tmp[0], &c->tmp_cap[0], (size_t)n0)) return -1;
    if (grow(c, &c->d_tmp[1], &c->tmp_cap[1], (size_t)n0)) return -1;
    float *t0 = c->d_tmp[0], *t1 = c->d_tmp[1], *rec = S.lv[0].img;
    if (launched(c, "k_to_il", launch_to_il(st, p0.img, rec, kRecImg, n0)) ||
        launched(c, "k_rows", launch_rows(st, p0.img, p0.w, p0.h, c->lazy_gd, t0)) ||
        launched(c, "k_cols", launch_cols(st, t0, p0.w, p0.h, c->lazy_gg, t1)) ||
        launched(c, "k_to_il", launch_to_il(st, t1, rec, kRecGx, n0)) ||
        launched(c, "k_rows", launch_rows(st, p0.img, p0.w, p0.h, c->lazy_gg, t0)) ||
        launched(c, "k_cols", launch_cols(st, t0, p0.w, p0.h, c->lazy_gd, t1)) ||
        launched(c, "k_to_il", launch_to_il(st, t1, rec, kRecGy, n0)))
      return -1;
  }
  S.lv[0].il = kLayoutRec;
  return prev_to_seed(c, 1, st);
}
}  // namespace

KLT_API int klt_hip_frames_begin(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const unsigned char *frame,
                                 long pitch) {
  if (!c || !pd || !frame) return fail(c, "frames_begin: null argument");
  if (use_device(c)) return -1;
  if (build_pyramid_on(c, kSeedSlot, pd, frame, pitch, 0, c->stream)) return -1;
  c->prev = PrevRef{-1, 0, kSeedSlot};
  c->frames_ready = true;
  return 0;
}

KLT_API int klt_hip_frames_begin_slot(klt_hip_ctx *c, int slot) {
  if (!c) return fail(c, "frames_begin_slot: null context");
  if (slot < 0 || slot >= KLT_HIP_MAX_SLOTS || c->slot[slot].nlev < 1)
    return fail(c, "frames_begin_slot: slot %d is not built", slot);
  c->prev = PrevRef{-1, 0, slot};
  c->frames_ready = true;
  return 0;
}

KLT_API int klt_hip_frames_end_slot(klt_hip_ctx *c, int slot) {
  if (!c) return fail(c, "frames_end_slot: null context");
  if (slot < 0 || slot >= KLT_HIP_MAX_SLOTS) return fail(c, "frames_end_slot: bad slot %d", slot);
  if (!c->frames_ready) return fail(c, "frames_end_slot: no current pyramid");
  if (c->prev.bank < 0 && c->prev.slot == slot) return 0;
  if (use_device(c)) return -1;
  if (prev_full(c)) return -1;  // an image-only bank frame: whole in the seed slot first
  int ss = 1;
  const klt_hip_pyr_desc d = prev_desc(c, &ss);
  const int nl = d.nlevels;
  if (ensure_slot(c, slot, &d)) return -1;
  Slot &S = c->slot[slot];
  S.ss = ss;
  S.fused = 1;
  for (int l = 0; l < nl; ++l) {
    const TrkLevel p = prev_level(c, l);
    if (p.w != S.lv[l].w || p.h != S.lv[l].h) return fail(c, "frames_end_slot: level %d size mismatch", l);
    if (slot_level(c, p, S.lv[l], c->stream)) return -1;
  }
  return 0;
}

int tables_refused(klt_hip_ctx *c, const char *who, const float *tab_x, const float *tab_y, const int *tab_val,
                   long tab_stride, int n, long pitch, int ncols) {
  const int ntab = (tab_x != nullptr) + (tab_y != nullptr) + (tab_val != nullptr);
  if (ntab != 0 && ntab != 3) return fail(c, "%s: give all three table arrays or none", who);
  if (ntab && tab_stride < n) return fail(c, "%s: table stride %ld < n %d", who, tab_stride, n);
  if (pitch < (long)ncols * frame_bpp(c->frame_format))
    return fail(c, "%s: pitch %ld < ncols %d * %d bytes per pixel", who, pitch, ncols, frame_bpp(c->frame_format));
  return 0;
}

namespace {
struct BandSpec {
  float own[2];        // features owned: own[0] <= y < own[1] (level-0 rows) at the chunk start
  int row_lo, row_hi;  // level-0 rows to build
  int *escape;         // device flag
  const unsigned char *next;  // optional: the next chunk's frames, built ahead on the pyramid stream
  int next_n;
};

// The rows of a band whose level-0 planes are built.  A feature owned by the
// band reads level-0 rows within a few of its own (its window and the chunk's
// motion) but level-1 rows whose sigma-3.6 support reaches 32 rows above and
// 40 below it, so the outer part of each margin -- all but its first 8 rows,
// at most 32 -- builds only the rows pass hs (k_pyr_l0 tiles without planes).
// The tracker's band test still guards level 0 with these rows.
void band_planes(const BandSpec &b, int &p0, int &p1) {
  constexpr int kKeep = 8, kSkip = 32;
  p0 = b.row_lo;
  p1 = b.row_hi;
  if (isfinite(b.own[0])) p0 = b.row_lo + clampi((int)b.own[0] - b.row_lo - kKeep, 0, kSkip);
  if (isfinite(b.own[1])) p1 = b.row_hi - clampi(b.row_hi - (int)ceilf(b.own[1]) - kKeep, 0, kSkip);
  if (p1 < p0) p1 = p0;
}

// track_frames_impl's arguments, as its steps take them (filled there, once)
struct FramesCall {
  const klt_hip_pyr_desc *pd;
  const klt_hip_track_desc *td;
  const unsigned char *frames;
  long pitch, stride;
  int nframes;
  float *x, *y;
  int *val;
  int n;
  float *tab_x, *tab_y;
  int *tab_val;
  long tab_stride;
  const BandSpec *band;
  long fb_row0;
};

// the arguments, the modes set on the context and the kept pyramid's shape
int frames_check(klt_hip_ctx *c, const FramesCall &q, int chunk) {
  const klt_hip_pyr_desc *pd = q.pd;
  const int n = q.n;
  if (!c || !pd || !q.td) return fail(c, "track_frames: null argument");
  if (!c->frames_ready) return fail(c, "track_frames: no previous pyramid (call klt_hip_frames_begin)");
  if (q.nframes < 0 || chunk < 1 || n < 0) return fail(c, "track_frames: bad nframes/chunk/n");
  if (q.nframes > 0 && !q.frames) return fail(c, "track_frames: null frames");
  if (n > 0 && (!q.x || !q.y || !q.val)) return fail(c, "track_frames: null feature arrays");
  if (q.band && c->frame_format != KLT_HIP_FRAME_GRAY8)  // (a band call has no tables)
    return fail(c, "track_frames_band: colour frames are not covered (klt_hip_set_frame_format %d); convert with "
                "klt_hip_to_gray", c->frame_format);
  if (tables_refused(c, "track_frames", q.tab_x, q.tab_y, q.tab_val, q.tab_stride, n, q.pitch, pd->ncols)) return -1;
  if (check_window(c, q.td)) return -1;
  if (c->rep_on && c->aff_on)
    return fail(c, "track_frames: the affine check does not combine with the replacement of lost features "
                "(klt_hip_set_frames_affine, klt_hip_set_frames_replace)");
  if (track_refused(c, q.td, q.band != nullptr, n, q.band ? "track_frames_band" : "track_frames")) return -1;
  if (mask_refused(c, pd->ncols, q.band ? "track_frames_band" : "track_frames")) return -1;
  const TrkLevel p0 = prev_level(c, 0);
  const int nl = kept_nlev(c);
  if (p0.w != pd->ncols || p0.h != pd->nrows || nl != pd->nlevels)
    return fail(c, "track_frames: frames are %dx%d/%d levels, previous pyramid %dx%d/%d", pd->ncols, pd->nrows,
                pd->nlevels, p0.w, p0.h, nl);
  return 0;
}

// every decision of one batched call
struct FramesPlan {
  bool fz;             // the fused pyramid kernels build the banks
  bool lazy;           // level 0 of the banks is the img plane alone (klt_hip_set_lazy_grad)
  int bil;             // the banks' layout
  int chunk, F;        // frames per bank (budget-capped) and per launch
  int sched;           // kSchedOne, kSchedBeside or kSchedTail
  bool serial;         // builds and trackers on the tracking stream
  bool tail;           // builds held until the running tracker's tail
  unsigned tail_left;  // ... of this many waves
  bool ahead;          // a band call whose next frames are ready (klt_hip_set_ahead_ready)
};

// the pyramids' path and layout: decided first, a call that is not lazy makes
// an image-only kept frame whole before anything else
FramesPlan plan_layout(klt_hip_ctx *c, const FramesCall &q) {
  const klt_hip_pyr_desc *pd = q.pd;
  const bool band = q.band != nullptr, t7 = t7_tracks(c, q.td);
  FramesPlan p{};
  p.fz = fused_ok(pd) && !c->force_generic;
  // level 0 of the banks as the img plane alone, its gradients computed by the
  // tracker for the windows it reads (klt_hip_set_lazy_grad): whole-frame fused
  // pyramids tracked by k_track7 (its fast-sum instance: two levels) without
  // the forward-backward check or the motion prior (the region mask's tracking
  // use has lazy instances: exact sums only, which it insists on), from a previous pyramid that is interleaved
  // or image-only itself.  Any other call first makes an image-only previous
  // pyramid whole.
  p.lazy = c->lazy_grad && p.fz && t7 && !band && !c->fb_on && !c->aff_on && !c->pred_on &&
           (q.td->reduction == KLT_HIP_EXACT || pd->nlevels == 2) && prev_level(c, 0).il != kLayoutPlanes;
  // the banks' layout follows their reader: interleaved for k_track7 (level 0
  // the img plane alone for its lazy-gradient instance), planes for the
  // generic tracker (no per-chunk conversion)
  p.bil = p.lazy ? kLayoutImg : t7 ? kLayoutRec : kLayoutPlanes;
  return p;
}

// the chunk and the schedule, once the pyramid stream exists
int plan_frames(klt_hip_ctx *c, const FramesCall &q, int chunk, FramesPlan &p) {
  const klt_hip_pyr_desc *pd = q.pd;
  const bool band = q.band != nullptr;
  // the banks' byte budget caps the chunk: a plain call runs shorter launches
  // (results do not depend on the chunk), a band call -- whose chunk is the
  // caller's exchange span -- fails before allocating anything
  const int fit = budget_chunk(c, pd);
  if (fit < 1)
    return fail(c, "track_frames: one %dx%d pyramid per bank exceeds the bank budget of %zu bytes", pd->ncols,
                pd->nrows, bank_budget_of(c));
  if (chunk > fit) {
    if (band)
      return fail(c, "track_frames_band: %d frames per chunk of %dx%d need %zu bytes of banks, over the budget of "
                  "%zu (klt_hip_set_bank_budget); at most %d frames fit", chunk, pd->ncols, pd->nrows,
                  bank_arena_bytes(pd, chunk), bank_budget_of(c), fit);
    chunk = fit;
  }
  p.chunk = chunk;
  p.F = chunk < q.nframes ? chunk : q.nframes;
  // band calls always use both streams: the next chunk's band pyramids are
  // built on the pyramid stream while this chunk is tracked and exchanged
  // A call that fits one chunk has nothing to overlap (its one pyramid build
  // must finish before its tracker starts), so it stays on the tracking
  // stream: the cross-queue event hand-off would only add its latency
  // (~12 us measured between k_pyr_l1's end and k_track7's start).  The next
  // call's pyramid stream still starts behind it (ev_start, track_frames_impl).
  //
  // The schedule of a plain call over several chunks (klt_hip_set_frames_overlap):
  //   one stream: build, track, build, track, no kernel shares the CUs;
  //   beside:     the pyramid stream builds chunk c+1 as soon as its bank is free,
  //               so for the whole of chunk c's tracker;
  //   tail:       the same, but the build is also held until at most tail_left
  //               waves of chunk c's tracker are still to leave (its exit count
  //               in c->d_exits), so it fills the CUs the tracker's last waves
  //               leave empty and does not run beside a full tracker.
  // Results are the same in all three.  The rule behind "automatic":
  // A lazy-gradient call's tracker is held to 96 VGPRs for five waves per SIMD;
  // 5 x 96 leaves 32 of a SIMD's 512 registers per lane and a pyramid wave needs
  // 64, so beside a full tracker the build only gets the slots that open here
  // and there, both kernels run slower for the tracker's whole length and the
  // next tracker waits for the slow build.  A quarter of the tracker's wave
  // slots stand empty over its launch, though, nearly all of them in its last
  // third, so those calls take "tail".  1080p / 5000, six alternating runs
  // each: one stream 84.6 k frames/s, beside 75.7 k, tail 89.8 k (its slowest run
  // above one stream's fastest).  4K / 20 000, whose waves never all reside at
  // once: one stream 22.3 k, beside 23.0 k, tail 23.0 k for every K from 2048 to
  // 8192 -- nothing to tell tail from beside, so the rule does not look at the
  // launch's size ("The schedule after lazy gradients";
  // profiles/sched_tail_bound.txt).  A launch of no more waves than tail_left
  // is not waited for, which is "beside" for a tracker that leaves room anyway.
  // The other trackers (full records, the forward-backward and affine checks,
  // fast sums on other depths, the generic kernel) leave room beside them, and
  // "beside" measured 2-3 % faster there: they keep it.
  constexpr int kAutoLazy = kSchedTail;
  p.sched = env_frames_sched() >= 0 ? env_frames_sched() : c->frames_sched;
  if (p.sched == kSchedAuto) p.sched = p.lazy ? kAutoLazy : kSchedBeside;
  if (c->rep_on) p.sched = kSchedOne;  // replacement inside the call: the context's stream alone
  p.serial = band ? false : (p.sched == kSchedOne || q.nframes <= chunk);
  p.tail = !band && !p.serial && p.sched == kSchedTail;
  p.tail_left = (unsigned)(env_frames_tail() >= 0 ? env_frames_tail() : c->tail_left);
  p.ahead = band && c->ahead_ready;
  return 0;
}

// what the plan needs of the context: the banks, the tail schedule's counters
int frames_resources(klt_hip_ctx *c, const FramesCall &q, const FramesPlan &p) {
  const klt_hip_pyr_desc *pd = q.pd;
  c->chunk_used = p.chunk;
  // banks hold `chunk` frames whatever this call's length, so a short first
  // call does not force a reallocation (and a drain) in the next one
  if (!banks_fit(c, pd, p.chunk)) {
    // they are laid out again: a previous pyramid living in a bank moves to
    // the seed slot first (an image-only frame: whole), on the tracking stream,
    // which has waited for that bank's build and is drained with the rest
    if (prev_full(c)) return -1;
    if (c->prev.bank >= 0 && (ensure_slot(c, kSeedSlot, pd) || prev_to_seed(c, 0, c->stream))) return -1;
  }
  if (ensure_banks(c, pd, p.chunk)) return -1;
  if (p.tail) {
    const bool fresh = !c->d_exits || !c->d_exit_sig;
    if (!c->d_exits) HIPCHK(c, hipMalloc((void **)&c->d_exits, sizeof(unsigned long long)));
    if (!c->d_exit_sig)
      HIPCHK(c, hipExtMallocWithFlags((void **)&c->d_exit_sig, sizeof(unsigned long long), hipMallocSignalMemory));
    if (fresh || c->exits_base > kExitsRebase) {
      // re-based long before the 32-bit count wraps, with nothing running or waiting
      HIPCHK(c, hipStreamSynchronize(c->stream));
      HIPCHK(c, hipStreamSynchronize(c->pstream));
      HIPCHK(c, hipMemsetAsync(c->d_exits, 0, sizeof(unsigned long long), c->stream));
      HIPCHK(c, hipMemsetAsync(c->d_exit_sig, 0, sizeof(unsigned long long), c->stream));
      c->exits_base = 0;
    }
  }
  return 0;
}

// the pyramid stream starts behind everything already queued on the
// tracking stream -- except a band call's build-ahead when the caller has
// said its frames are ready (klt_hip_set_ahead_ready): that waits for its
// bank and starts with this chunk's tracker (ev_go), so the short kernels
// between two trackers (the processing order; the caller's exchange before
// the call) run without pyramid waves beside them -- each of them is on the
// chain, and measured 3-10x slower with k_pyr_l0 filling the CUs
// (profiles/r05_rank_timeline_*.txt)
// Every event record and cross-stream wait is a packet the tracking queue
// processes between two trackers (several us each), so the ahead-ready
// band call records ev_start only when a build needs it, and no banks.ev_free
// (its build-ahead waits for ev_go, which follows the previous tracker)
struct PstreamBehind {
  bool serial, ahead;
  bool pwait = false;  // the pyramid stream waits for ev_start already
  int operator()(klt_hip_ctx *c) {
    if (serial || pwait) return 0;
    pwait = true;
    if (ahead) HIPCHK(c, hipEventRecord(c->ev_start, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->pstream, c->ev_start, 0));
    return 0;
  }
};

// One chunk of the call is F frames from src into bank bi, built on ps;
// prebuilt (band mode): the previous call built it ahead.
// The chunk's pyramids into its bank.  rel: the tail release of the previous
// chunk's tracker launch, taken here
int build_chunk(klt_hip_ctx *c, const FramesCall &q, const FramesPlan &p, int bi, int F, const unsigned char *src,
                hipStream_t ps, bool prebuilt, PstreamBehind &behind, TailRelease &rel) {
  const BandSpec *band = q.band;
  Bank &K = c->banks.bank[bi];
  // one stream: stream order is the dependency (an event wait would add a queue barrier)
  if (!p.serial && !prebuilt && behind(c)) return -1;  // this chunk's own frames: behind the caller's work
  if (!p.serial && !prebuilt && !p.ahead) HIPCHK(c, hipStreamWaitEvent(ps, c->banks.ev_free[bi], 0));
  // tail: a hint on top of banks.ev_free / banks.ev_built, which stay the dependencies.
  // The tracker that raises the count to rel.thr was enqueued for the
  // previous chunk and reaches it by completing.
  if (rel.wait) HIPCHK(c, hipStreamWaitValue32(ps, c->d_exit_sig, rel.thr, hipStreamWaitValueGte, 0xFFFFFFFFu));
  rel.wait = false;
  if (prebuilt) {
    // banks.ev_built[bi] was recorded after that build: the driver's wait orders it
  } else if (p.fz) {
    int p0 = 0, p1 = 1 << 30;
    if (band) band_planes(*band, p0, p1);
    if (build_fused_bank(c, K, q.pd, src, q.pitch, q.stride, F, ps, band ? band->row_lo : 0,
                         band ? band->row_hi : 1 << 30, p0, p1, p.bil))
      return -1;
  } else {
    for (int f = 0; f < F; ++f) {
      if (build_pyramid_on(c, kScratchSlot, q.pd, src + (long)f * q.stride, q.pitch, 0, ps)) return -1;
      for (int l = 0; l < q.pd->nlevels; ++l)  // generic levels: planes
        if (copy_level(c, level_view(c->slot[kScratchSlot].lv[l]), K.lv[l], f, ps)) return -1;
    }
    K.holds(kLayoutPlanes);  // whole frames: every row is valid
  }
  return 0;
}

// the chunk's tracker launch (b: its processing order, already queued); the
// chunk's last frame is the kept pyramid from here on.  rel: out, the exit
// count at which the pyramid stream may start the next build.
// f0 > 0 (replacement inside the call): a sub-launch over the bank's frames
// [f0, f0 + F), the call's frames from j0 on; the kept pyramid it starts from
// is the bank's frame f0 - 1, where the sub-launch before it ended
int launch_chunk(klt_hip_ctx *c, const FramesCall &q, const FramesPlan &p, int bi, int j0, int F, TrkArgs &a,
                 TrkFramesArgs &b, TailRelease &rel, int f0 = 0) {
  const BandSpec *band = q.band;
  const Bank &K = c->banks.bank[bi];
  for (int l = 0; l < q.pd->nlevels; ++l) {
    a.A[l] = prev_level(c, l);
    a.B[l] = K.level(l, f0);
    b.lfs[l] = (long)K.lv[l].w * K.lv[l].h * (K.lv[l].il == kLayoutRec ? 3 : 1);
  }
  b.nframes = F;
  if (q.tab_x) {
    b.tx = q.tab_x + (long)j0 * q.tab_stride;
    b.ty = q.tab_y + (long)j0 * q.tab_stride;
    b.tv = q.tab_val + (long)j0 * q.tab_stride;
    b.tstride = q.tab_stride;
  }
  if (p.ahead) {
    if (!c->ev_go) HIPCHK(c, hipEventCreateWithFlags(&c->ev_go, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_go, c->stream));
  }
  rel = TailRelease{p.tail_left, false, 0};
  const bool count = p.tail && c->exits_base <= kExitsRebase && (unsigned)q.n < kExitsRebase;
  if (q.n > 0 && track_frames_launch(c, c->stream, q.td, a, b, q.x, q.y, q.val, q.n, band ? band->own : nullptr, true,
                                     q.fb_row0 + j0, count ? &rel : nullptr))
    return -1;
  HMARK_IN("track");
  if (!p.serial && !p.ahead && c->prev.bank >= 0) HIPCHK(c, hipEventRecord(c->banks.ev_free[c->prev.bank], c->stream));
  c->prev = PrevRef{bi, f0 + F - 1};
  return 0;
}

// a band call's next chunk, into the bank it will take, on the pyramid
// stream: its pyramids depend on frames only, not on this chunk's result
int build_ahead(klt_hip_ctx *c, const FramesCall &q, const FramesPlan &p, const PstreamBehind &behind) {
  const BandSpec *band = q.band;
  if (!(band && band->next && band->next_n > 0 && p.fz)) return 0;
  const int bj = c->banks.peek();
  const int Fn = band->next_n < p.chunk ? band->next_n : p.chunk;
  if (c->ahead_ready) {  // with this chunk's tracker, so after the previous one: bank bj is free
    if (!behind.pwait) HIPCHK(c, hipStreamWaitEvent(c->pstream, c->ev_go, 0));
  } else {
    HIPCHK(c, hipStreamWaitEvent(c->pstream, c->banks.ev_free[bj], 0));
  }
  int p0 = 0, p1 = 1 << 30;
  band_planes(*band, p0, p1);
  if (build_fused_bank(c, c->banks.bank[bj], q.pd, band->next, q.pitch, q.stride, Fn, c->pstream, band->row_lo,
                       band->row_hi, p0, p1, p.bil))
    return -1;
  HIPCHK(c, hipEventRecord(c->banks.ev_built[bj], c->pstream));
  c->banks.built_ahead(BuiltAhead{bj, Fn, band->row_lo, band->row_hi, p.bil, band->next, q.stride});
  return 0;
}

// One replacement of lost features (klt_hip_set_frames_replace): the kept
// pyramid is the frame just tracked, `row` its table row.  Its trackability
// map is taken where the frame lies -- an image-only level 0 by
// k_min_eigen7_img when the window and step are its own, anything else as
// klt_hip_min_eigen_rows does it (which completes an image-only frame first).
// The counters are the context's.
template <class Ahead>
int replace_lost(klt_hip_ctx *c, const FramesCall &q, long row, Ahead ahead) {
  const int first[2] = {0, q.n};
  const RepLists lists{1, q.n, first, q.x, q.y, q.val, q.tab_x, q.tab_y, q.tab_val, q.tab_stride};
  const klt_hip_select_desc &sd = c->rep.sel;
  const auto maps = [&](const EigMultiArgs &, const SelGrid &g) -> long {
    const TrkLevel L = prev_level(c, 0);
    const long np = (long)g.nx * g.ny;
    if (L.il == kLayoutImg && g.hw == kRG && g.hh == kRG && g.step <= 2 && c->lazy_gg.w == 2 * kRG + 1 &&
        c->lazy_gd.w == 2 * kRG + 1) {
      GradTaps t;
      for (int m = 0; m < 2 * kRG + 1; ++m) {
        t.g[m] = c->lazy_gg.k[m];
        t.d[m] = c->lazy_gd.k[m];
      }
      TimedScope ts(c, T_EIG, c->stream);
      return launched(c, "k_min_eigen7_img", launch_min_eigen_img(c->stream, L.img, L.w, L.h, t, sd.borderx, sd.bordery,
                                                                  g.step, g.nx, g.ny, c->d_rep_map, &c->eig_kernel))
                 ? -1 : np;
    }
    int nx = 0, ny = 0, r0 = 0, r1 = 0;
    const int rc = klt_hip_min_eigen_rows(c, &sd, 0, L.h, c->d_rep_map, &nx, &ny, &r0, &r1);
    if (rc < 0) return -1;
    if (rc > 0 || r0 != 0 || r1 != ny) return fail(c, "track_frames: the tracked frame does not hold every row of the map");
    return np;
  };
  if (c->rep_changed.size() < (size_t)q.n) c->rep_changed.resize((size_t)q.n, 0);
  const TrkLevel L = prev_level(c, 0);
  long filled = 0;
  if (replace_step(c, lists, c->rep, L.w, L.h, row, RepCounters{c->rep_changed.data(), &c->rep_runs, &c->rep_filled},
                   ahead, maps, &filled))
    return -1;
  // results never depend on the cached processing order, but new features
  // would sit in the lost features' places
  if (filled) c->perm_n = -1;
  return 0;
}

// The chunks of a call that replaces lost features: the pyramid launches keep
// the chunk, the tracker launch is cut where the frame count since the setting
// was turned on reaches a multiple of `every`, and each cut runs the
// replacement.  All on the tracking stream; the next chunk's pyramids are
// queued before the host waits for the list of a chunk's last frame.
int track_frames_replacing(klt_hip_ctx *c, const FramesCall &q, const FramesPlan &p, TrkArgs &a,
                           PstreamBehind &behind) {
  const int every = c->rep.every;
  TailRelease rel{p.tail_left, false, 0};
  int bi = -1, ahead_bank = -1;
  for (int j0 = 0; j0 < q.nframes; j0 += p.F) {
    const int F = p.F < q.nframes - j0 ? p.F : q.nframes - j0;
    if (ahead_bank >= 0) {
      bi = ahead_bank;
    } else {
      bi = c->banks.take();
      if (build_chunk(c, q, p, bi, F, q.frames + (long)j0 * q.stride, c->stream, false, behind, rel)) return -1;
    }
    ahead_bank = -1;
    const int jn = j0 + F, Fn = p.F < q.nframes - jn ? p.F : q.nframes - jn;
    for (int f0 = 0; f0 < F;) {
      const int f1 = next_cut(c->rep_frames, every, f0, F);
      TrkFramesArgs b;
      memset(&b, 0, sizeof b);
      if (q.n > 0 && order_features(c, c->stream, q.pd->nrows, q.y, q.val, q.n, f1 - f0, nullptr, b)) return -1;
      if (launch_chunk(c, q, p, bi, j0 + f0, f1 - f0, a, b, rel, f0)) return -1;
      c->rep_frames += f1 - f0;
      if (c->rep_frames % every == 0) {
        const auto ahead = [&]() -> int {
          if (f1 < F || Fn <= 0) return 0;
          ahead_bank = c->banks.take();
          return build_chunk(c, q, p, ahead_bank, Fn, q.frames + (long)jn * q.stride, c->stream, false, behind, rel);
        };
        if (replace_lost(c, q, j0 + f1 - 1, ahead)) return -1;
      }
      f0 = f1;
    }
  }
  return 0;
}

int track_frames_impl(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                      const unsigned char *frames, long pitch, long stride, int nframes, int chunk, float *x,
                      float *y, int *val, int n, float *tab_x, float *tab_y, int *tab_val, long tab_stride,
                      const BandSpec *band, long fb_row0 = 0) {
#ifdef KLT_HOST_PROF
  HostMarks hm_;
#endif
  HMARK("enter");
  const FramesCall q{pd, td, frames, pitch, stride, nframes, x, y, val, n, tab_x, tab_y, tab_val, tab_stride, band,
                     fb_row0};
  if (frames_check(c, q, chunk)) return -1;
  if (nframes == 0) return 0;
  HMARK("checks");
  if (use_device(c)) return -1;
  HMARK("set_device");
  FramesPlan p = plan_layout(c, q);
  if (!p.lazy && prev_full(c)) return -1;
  if (ensure_pipeline(c)) return -1;
  if (!c->banks.ev_built[0])
    for (int k = 0; k < 3; ++k) {
      HIPCHK(c, hipEventCreateWithFlags(&c->banks.ev_built[k], hipEventDisableTiming));
      HIPCHK(c, hipEventCreateWithFlags(&c->banks.ev_free[k], hipEventDisableTiming));
    }
  if (plan_frames(c, q, chunk, p)) return -1;
  HMARK("budget");
  if (frames_resources(c, q, p)) return -1;
  PstreamBehind behind{p.serial, p.ahead};
  if (!p.serial && !p.ahead) HIPCHK(c, hipEventRecord(c->ev_start, c->stream));
  if (!p.ahead && behind(c)) return -1;
  if (band && !p.fz) return fail(c, "track_frames_band: needs the fused (default-parameter) pyramid path");
  TrkArgs a;
  fill_trk_args(td, pd->nlevels, pd->nlevels > 1 ? pd->subsampling : 1, pd->ncols, pd->nrows, a);
  if (p.lazy) {
    c->lazy_gg = reverse_taps(pd->grad_gauss);
    c->lazy_gd = reverse_taps(pd->grad_deriv);
    a.lazy = 1;
    for (int m = 0; m < 2 * kRG + 1; ++m) {
      a.gg[m] = c->lazy_gg.k[m];
      a.gd[m] = c->lazy_gd.k[m];
    }
  }
  if (band) a.escape = band->escape;
  if (c->rep_on) return track_frames_replacing(c, q, p, a, behind);
  TailRelease rel{p.tail_left, false, 0};
  for (int j0 = 0; j0 < nframes; j0 += p.F) {
    const int F = p.F < nframes - j0 ? p.F : nframes - j0;
    const unsigned char *src = frames + (long)j0 * stride;
    // overlapped: the pyramid stream builds chunk c+1 while chunk c is tracked;
    // serial: both on the tracking stream (no two kernels share the CUs)
    hipStream_t ps = p.serial ? c->stream : c->pstream;
    // the processing order reads the positions this chunk starts from: queued
    // on the tracking stream ahead of its wait for the chunk's pyramids (and,
    // serial, ahead of the build), so the sort is off the chain
    TrkFramesArgs b;
    memset(&b, 0, sizeof b);
    HMARK("chunk_top");
    if (n > 0 && order_features(c, c->stream, pd->nrows, y, val, n, F, band ? band->own : nullptr, b)) return -1;
    HMARK("order");
    // a band call takes the bank the previous call built ahead, when it holds these frames
    const BuiltAhead want{-1, F, band ? band->row_lo : 0, band ? band->row_hi : 0, p.bil, src, stride};
    bool prebuilt = false;
    const int bi = c->banks.take(band ? &want : nullptr, &prebuilt);
    if (build_chunk(c, q, p, bi, F, src, ps, prebuilt, behind, rel)) return -1;
    HMARK("pyramids");
    if (!p.serial) {  // the built bank to the tracking stream
      if (!prebuilt) HIPCHK(c, hipEventRecord(c->banks.ev_built[bi], ps));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->banks.ev_built[bi], 0));
    }
    if (launch_chunk(c, q, p, bi, j0, F, a, b, rel)) return -1;
  }
  return build_ahead(c, q, p, behind);
}
}  // namespace

KLT_API int klt_hip_track_frames(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                                 const unsigned char *frames, long pitch, long stride, int nframes, int chunk,
                                 float *x, float *y, int *val, int n, float *tab_x, float *tab_y, int *tab_val,
                                 long tab_stride) {
  AffCall aff_call(c);
  return track_frames_impl(c, pd, td, frames, pitch, stride, nframes, chunk, x, y, val, n, tab_x, tab_y, tab_val,
                           tab_stride, nullptr);
}

// Host frames (klt_hip_track_frames_host): the caller's pageable frames go up
// chunk by chunk.  Per chunk: the pool copies the frames into a pinned staging
// slot, one DMA moves the slot into a device ring slot (copy stream), the
// batched pyramids + tracker run on the context stream and write the chunk's
// table rows into a device rows slot, one D2H brings the rows into a pinned
// host slot (a third stream), and the pool hands them to the caller's
// callback.  Two slots of each: the upload of chunk c+1 and the delivery of
// chunk c-1 run on the host while chunk c is on the device.
// the copy streams of the host pipeline (KLTTrackSequence)
static int copy_streams(klt_hip_ctx *c) {
  for (hipStream_t *st : {&c->cstream, &c->dstream})
    if (!*st) HIPCHK(c, hipStreamCreateWithFlags(st, hipStreamNonBlocking));
  return 0;
}

namespace {
int host_pipeline_prepare(klt_hip_ctx *c, size_t stage_bytes, size_t rows_bytes) {
  if (copy_streams(c)) return -1;
  for (int k = 0; k < 2; ++k)
    for (hipEvent_t *e : {&c->ev_ring_free[k], &c->ev_dma[k], &c->ev_tracked[k], &c->ev_rows[k]})
      if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
  if (c->stage_cap < stage_bytes || c->hrows_cap < rows_bytes) {
    HIPCHK(c, hipDeviceSynchronize());  // no copy still reads the old pinned buffers
    if (c->stage_cap < stage_bytes) {
      if (c->h_stage) HIPCHK(c, hipHostFree(c->h_stage));
      c->h_stage = nullptr;
      c->stage_cap = 0;
      HIPCHK(c, hipHostMalloc((void **)&c->h_stage, stage_bytes, hipHostMallocDefault));
      c->stage_cap = stage_bytes;
    }
    if (c->hrows_cap < rows_bytes) {
      if (c->h_rows) HIPCHK(c, hipHostFree(c->h_rows));
      c->h_rows = nullptr;
      c->hrows_cap = 0;
      HIPCHK(c, hipHostMalloc((void **)&c->h_rows, rows_bytes, hipHostMallocDefault));
      c->hrows_cap = rows_bytes;
    }
  }
  if (c->ring_cap < stage_bytes) {
    HIPCHK(c, hipDeviceSynchronize());
    hipFree(c->d_ring);
    c->d_ring = nullptr;
    c->ring_cap = 0;
    HIPCHK(c, hipMalloc((void **)&c->d_ring, stage_bytes));
    c->ring_cap = stage_bytes;
  }
  if (c->drows_cap < rows_bytes) {
    HIPCHK(c, hipDeviceSynchronize());
    hipFree(c->d_rows);
    c->d_rows = nullptr;
    c->drows_cap = 0;
    HIPCHK(c, hipMalloc((void **)&c->d_rows, rows_bytes));
    c->drows_cap = rows_bytes;
  }
  ensure_pool(c);
  return 0;
}
}  // namespace

namespace {
// klt_hip_track_frames_host with the motion prior on: the launches read and
// write the context's own device block (vx | vy), filled from the caller's
// arrays before the first one and copied back to them after the last; the
// setting points at the caller's arrays again however the call ends
struct PredStage {
  klt_hip_ctx *c;
  int n;
  float *vx, *vy;  // the caller's arrays; null: the setting is off, or no features
  PredStage(klt_hip_ctx *c_, int n_) : c(c_), n(n_), vx(nullptr), vy(nullptr) {
    if (c->pred_on && n > 0) vx = c->pred_vx, vy = c->pred_vy;
  }
  ~PredStage() {
    if (vx) c->pred_vx = vx, c->pred_vy = vy;
  }
  PredStage(const PredStage &) = delete;
  PredStage &operator=(const PredStage &) = delete;
  int up() const {
    if (!vx) return 0;
    if (grow(c, &c->d_pred, &c->pred_cap, 2 * (size_t)n)) return -1;
    const size_t nb = sizeof(float) * (size_t)n;
    HIPCHK(c, hipMemcpyAsync(c->d_pred, vx, nb, hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_pred + n, vy, nb, hipMemcpyDefault, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's arrays may be pageable: read by now
    c->pred_vx = c->d_pred;
    c->pred_vy = c->d_pred + n;
    return 0;
  }
  int down() const {
    if (!vx) return 0;
    const size_t nb = sizeof(float) * (size_t)n;
    HIPCHK(c, hipMemcpyAsync(vx, c->d_pred, nb, hipMemcpyDefault, c->stream));
    HIPCHK(c, hipMemcpyAsync(vy, c->d_pred + n, nb, hipMemcpyDefault, c->stream));
    return 0;  // feat_unpack waits for the stream
  }
};
}  // namespace

KLT_API int klt_hip_track_frames_host(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                                      const unsigned char *const *frames, int nframes, int seed_first, int chunk,
                                      float *x, float *y, int *val, int n, klt_hip_rows_fn rows, void *user) {
  if (!c || !pd || !td || (nframes > 0 && !frames)) return fail(c, "track_frames_host: null argument");
  if (chunk < 1 || nframes < 0 || n < 0) return fail(c, "track_frames_host: bad nframes/chunk/n");
  const GrayFrames gray_ring(c);  // host frames are gray: so is the upload ring the calls below read
  if (mask_track_refused(c, td, false, "track_frames_host") || mask_refused(c, pd->ncols, "track_frames_host")) return -1;
  if (pred_refused(c, td, false, "track_frames_host")) return -1;
  if (fb_refused(c, td, false, "track_frames_host")) return -1;
  if (aff_refused(c, td, false, n, "track_frames_host")) return -1;
  if (c->rep_on && c->aff_on)
    return fail(c, "track_frames_host: the affine check does not combine with the replacement of lost features "
                "(klt_hip_set_frames_affine, klt_hip_set_frames_replace)");
  AffCall aff_call(c);
  if (n > 0 && (!x || !y || !val)) return fail(c, "track_frames_host: null feature arrays");
  for (int f = 0; f < nframes; ++f)
    if (!frames[f]) return fail(c, "track_frames_host: frame %d is NULL", f);
  if (nframes - (seed_first ? 1 : 0) <= 0) return 0;
  if (use_device(c)) return -1;
  // KLT_SEQ_TRACE=1: one stderr line per call -- wall time and minor page
  // faults per stage (SeqStages: host_pipeline_prepare and the feature
  // staging, waits for a staging slot's previous DMA, copies into staging,
  // launches, waits for the table rows, handing them out, the final list)
  SeqStages tr;
  tr.start(seq_trace());
  const size_t fb = (size_t)pd->ncols * pd->nrows;
  const int F = chunk < nframes ? chunk : nframes;
  const size_t rows_slot = (size_t)3 * F * (n > 0 ? n : 1);  // floats: x | y | val rows of one chunk
  if (host_pipeline_prepare(c, 2 * F * fb, 2 * rows_slot * sizeof(float))) return -1;
  if (n > 0 && feat_stage_in(c, x, y, val, n)) return -1;
  float *dx = c->d_fx, *dy = c->d_fy;
  int *dv = c->d_fv;
  // the motion prior's state goes up with the list and comes back with it
  // (the caller's arrays may be host arrays here, as x, y and val are)
  const PredStage pred_stage(c, n);
  if (pred_stage.up()) return -1;
  // the ring and the rows slots may still be read by earlier work on the context stream
  for (int k = 0; k < 2; ++k) {
    HIPCHK(c, hipEventRecord(c->ev_ring_free[k], c->stream));
    HIPCHK(c, hipEventRecord(c->ev_rows[k], c->stream));
  }
  const int nchunks = (nframes + F - 1) / F;
  tr.mark(SeqStages::PRE);
  auto upload = [&](int ci) -> int {
    const int k = ci & 1, f0 = ci * F, nf = F < nframes - f0 ? F : nframes - f0;
    unsigned char *stage = c->h_stage + (size_t)k * F * fb;
    tr.mark(SeqStages::LAUNCH);
    HIPCHK(c, hipEventSynchronize(c->ev_dma[k]));  // the slot's previous DMA is done
    tr.mark(SeqStages::WAIT_DMA);
    const size_t piece = 512 << 10, per = (fb + piece - 1) / piece;
    if (host_parallel(c, (size_t)nf * per, [&](size_t t) {
          const size_t f = t / per, o = (t - f * per) * piece;
          copy_stream(stage + f * fb + o, frames[f0 + f] + o, fb - o < piece ? fb - o : piece);
        }))
      return -1;
    tr.mark(SeqStages::COPY);
    HIPCHK(c, hipStreamWaitEvent(c->cstream, c->ev_ring_free[k], 0));
    HIPCHK(c, hipMemcpyAsync(c->d_ring + (size_t)k * F * fb, stage, (size_t)nf * fb, hipMemcpyHostToDevice,
                             c->cstream));
    HIPCHK(c, hipEventRecord(c->ev_dma[k], c->cstream));
    return 0;
  };
  auto ring_ready = [&](int k) -> int {
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_dma[k], 0));
    return 0;
  };
  // tracked frames of chunk ci: input frames [f0+skip, f0+nf), table rows from t0
  auto span = [&](int ci, int &t0, int &nt, int &skip) {
    const int f0 = ci * F, nf = F < nframes - f0 ? F : nframes - f0;
    skip = (ci == 0 && seed_first) ? 1 : 0;
    nt = nf - skip;
    t0 = f0 + skip - (seed_first ? 1 : 0);
  };
  auto deliver = [&](int ci) -> int {
    int t0, nt, skip;
    span(ci, t0, nt, skip);
    if (!rows || nt <= 0 || n <= 0) return 0;
    const int k = ci & 1;
    tr.mark(SeqStages::LAUNCH);
    HIPCHK(c, hipEventSynchronize(c->ev_rows[k]));
    tr.mark(SeqStages::WAIT_ROWS);
    const float *hx = c->h_rows + k * rows_slot, *hy = hx + (size_t)F * n;
    const int *hv = reinterpret_cast<const int *>(hy + (size_t)F * n);
    const int per = 256;
    const int rc = host_parallel(c, (size_t)(n + per - 1) / per, [&](size_t t) {
      const int a = (int)t * per, b = a + per < n ? a + per : n;
      rows(user, t0, nt, a, b, hx, hy, hv, n);
    });
    tr.mark(SeqStages::DELIVER);
    return rc;
  };
  if (upload(0)) return -1;
  if (seed_first) {  // frames[0]'s pyramid, built from its uploaded copy
    if (ring_ready(0)) return -1;
    if (klt_hip_frames_begin(c, pd, c->d_ring, pd->ncols)) return -1;
  }
  for (int ci = 0; ci < nchunks; ++ci) {
    const int k = ci & 1;
    int t0, nt, skip;
    span(ci, t0, nt, skip);
    float *rx = c->d_rows + k * rows_slot, *ry = rx + (size_t)F * n;
    int *rv = reinterpret_cast<int *>(ry + (size_t)F * n);
    if (ring_ready(k)) return -1;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_rows[k], 0));  // the rows slot's last D2H is done
    // a call that replaces lost features blocks on the list inside the chunk:
    // the next chunk's upload does not depend on it and goes first
    const bool up_first = c->rep_on && ci + 1 < nchunks;
    if (up_first && upload(ci + 1)) return -1;
    if (nt > 0 && track_frames_impl(c, pd, td, c->d_ring + (size_t)k * F * fb + skip * fb, pd->ncols, fb, nt, F,
                                    dx, dy, dv, n, rows ? rx : nullptr, rows ? ry : nullptr, rows ? rv : nullptr,
                                    n, nullptr, t0))
      return -1;
    HIPCHK(c, hipEventRecord(c->ev_ring_free[k], c->stream));
    if (rows && n > 0 && nt > 0) {
      HIPCHK(c, hipEventRecord(c->ev_tracked[k], c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->dstream, c->ev_tracked[k], 0));
      float *hx = c->h_rows + k * rows_slot;
      const size_t b = sizeof(float) * (size_t)nt * n;
      HIPCHK(c, hipMemcpyAsync(hx, rx, b, hipMemcpyDeviceToHost, c->dstream));
      HIPCHK(c, hipMemcpyAsync(hx + (size_t)F * n, ry, b, hipMemcpyDeviceToHost, c->dstream));
      HIPCHK(c, hipMemcpyAsync(hx + (size_t)2 * F * n, rv, b, hipMemcpyDeviceToHost, c->dstream));
      HIPCHK(c, hipEventRecord(c->ev_rows[k], c->dstream));
    }
    if (!up_first && ci + 1 < nchunks && upload(ci + 1)) return -1;  // overlaps chunk ci on the device
    if (ci >= 1 && deliver(ci - 1)) return -1;          // and the rows of chunk ci-1
  }
  if (deliver(nchunks - 1)) return -1;
  tr.mark(SeqStages::LAUNCH);
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(c->h_feat, c->d_feat, 3 * sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (pred_stage.down()) return -1;
    if (feat_unpack(c, x, y, val, n)) return -1;
  }
  tr.mark(SeqStages::TAIL);
  tr.print(nframes, nchunks, c->copy_threads);
  return 0;
}

KLT_API int klt_hip_track_frames_band(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                                      const unsigned char *frames, long pitch, long stride, int nframes,
                                      float *x, float *y, int *val, int n, float own_lo, float own_hi,
                                      int row_lo, int row_hi, int *escape, const unsigned char *next_frames,
                                      int next_nframes) {
  if (c && c->rep_on)
    return fail(c, "track_frames_band: not covered while lost features are replaced (klt_hip_set_frames_replace)");
  if (!escape) return fail(c, "track_frames_band: null escape flag");
  BandSpec bs{{own_lo, own_hi}, row_lo, row_hi, escape, next_frames, next_nframes};
  return track_frames_impl(c, pd, td, frames, pitch, stride, nframes, nframes > 0 ? nframes : 1, x, y, val, n,
                           nullptr, nullptr, nullptr, 0, &bs);
}

KLT_API int klt_hip_min_eigen_rows(klt_hip_ctx *c, const klt_hip_select_desc *d, int row_lo, int row_hi,
                                   int *dev_map, int *nx, int *ny, int *r0, int *r1) {
  if (!c || !d || !nx || !ny || !r0 || !r1) return fail(c, "min_eigen_rows: null argument");
  if (!c->frames_ready) return fail(c, "min_eigen_rows: no tracked frame (call klt_hip_frames_begin)");
  if (kept_image_only(c) && (use_device(c) || prev_full(c))) return -1;  // the map reads level-0 gradients
  const TrkLevel L = prev_level(c, 0);
  const SelGrid g = sel_grid(*d, L.w, L.h);
  const int hw = g.hw, hh = g.hh, step = g.step, gx = g.nx, gy = g.ny;
  if (step < 1) return fail(c, "min_eigen_rows: bad nSkippedPixels");
  const int bx = d->borderx, by = d->bordery;
  if (bx < hw || by < hh) return fail(c, "min_eigen_rows: border smaller than window half size");
  // grid rows j with by + j*step in [row_lo, row_hi)
  auto first_at = [&](int y) { return clampi(y <= by ? 0 : (y - by + step - 1) / step, 0, gy); };
  const int j0 = first_at(row_lo), j1 = first_at(row_hi) > j0 ? first_at(row_hi) : j0;
  *nx = gx;
  *ny = gy;
  *r0 = j0;
  *r1 = j1;
  if (!dev_map || j1 == j0 || gx == 0) return 0;
  // the window's gradient rows must have been built (a band pyramid holds [vlo, vhi))
  const int ylo = by + j0 * step - hh, yhi = by + (j1 - 1) * step + hh + 1;
  if (ylo < L.vlo || (yhi > L.vhi && L.vhi < L.h)) return 1;
  if (use_device(c)) return -1;
  TimedScope ts(c, T_EIG, c->stream);
  return launched(c, "k_min_eigen", launch_min_eigen(c->stream, L.il ? L.img + kRecGx : L.gx, L.il ? L.img + kRecGy : L.gy,
                                                     L.w, L.il ? 3 : 1, bx, by + j0 * step, step, gx, j1 - j0, hw,
                                                     hh, dev_map + (long)j0 * gx, &c->eig_kernel));
}

// the reference's gradient kernels for sigma 1.0 (klt_api.c: taps_make, the C
// arithmetic of convolve.c:60-114)
extern "C" void klt_default_grad_taps(klt_hip_taps *gauss, klt_hip_taps *deriv);

KLT_API int klt_hip_min_eigen_plane(klt_hip_ctx *c, const float *dev_img, int ncols, int nrows,
                                    const klt_hip_select_desc *d, int *dev_map) {
  if (!c || !dev_img || !d || !dev_map || ncols < 1 || nrows < 1) return fail(c, "min_eigen_plane: bad argument");
  const SelGrid g = sel_grid(*d, ncols, nrows);
  const int step = g.step, nx = g.nx, ny = g.ny;
  if (d->window_width != 2 * kRG + 1 || d->window_height != 2 * kRG + 1)
    return fail(c, "min_eigen_plane: window %dx%d, the kernel covers 7x7 only", d->window_width, d->window_height);
  if (step < 1 || step > 2) return fail(c, "min_eigen_plane: step %d, the kernel covers 1 and 2", step);
  if (d->borderx < kRG || d->bordery < kRG) return fail(c, "min_eigen_plane: border smaller than window half size");
  if ((long)nx * ny == 0) return 0;
  if (use_device(c)) return -1;
  klt_hip_taps gg, gd;
  klt_default_grad_taps(&gg, &gd);
  if (gg.width != 2 * kRG + 1 || gd.width != 2 * kRG + 1) return fail(c, "min_eigen_plane: default taps are not 7 wide");
  const RTaps rg = reverse_taps(gg), rd = reverse_taps(gd);
  GradTaps t;
  for (int m = 0; m < 2 * kRG + 1; ++m) {
    t.g[m] = rg.k[m];
    t.d[m] = rd.k[m];
  }
  {
    TimedScope ts(c, T_EIG, c->stream);
    if (launched(c, "k_min_eigen7_img", launch_min_eigen_img(c->stream, dev_img, ncols, nrows, t, d->borderx, d->bordery,
                                                             step, nx, ny, dev_map, &c->eig_kernel)))
      return -1;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int replace_desc_refused(klt_hip_ctx *c, const klt_hip_replace_desc *d, const char *who) {
  if (d->every < 1) return fail(c, "%s: every %d < 1", who, d->every);
  if (d->sel.window_width < 1 || d->sel.window_height < 1)
    return fail(c, "%s: window %dx%d", who, d->sel.window_width, d->sel.window_height);
  if (d->sel.borderx < d->sel.window_width / 2 || d->sel.bordery < d->sel.window_height / 2)
    return fail(c, "%s: border smaller than window half size", who);
  if (d->sel.nSkippedPixels < 0) return fail(c, "%s: bad nSkippedPixels", who);
  return 0;
}

KLT_API int klt_hip_set_frames_replace(klt_hip_ctx *c, const klt_hip_replace_desc *d) {
  if (!c) return -1;
  if (!d) {
    c->rep_on = 0;
    return 0;
  }
  if (replace_desc_refused(c, d, "set_frames_replace")) return -1;
  c->rep = *d;
  c->rep_on = 1;
  c->rep_frames = c->rep_runs = c->rep_filled = 0;
  c->rep_changed.clear();
  return 0;
}

KLT_API int klt_hip_get_frames_replace(klt_hip_ctx *c, int *on, long *frames, long *replacements, long *filled) {
  if (!c) return -1;
  if (on) *on = c->rep_on;
  if (frames) *frames = c->rep_frames;
  if (replacements) *replacements = c->rep_runs;
  if (filled) *filled = c->rep_filled;
  return 0;
}

KLT_API int klt_hip_frames_replace_changed(klt_hip_ctx *c, unsigned char *changed, int n) {
  if (!c || n < 0 || (n > 0 && !changed)) return fail(c, "frames_replace_changed: bad argument");
  for (int k = 0; k < n; ++k) changed[k] = (size_t)k < c->rep_changed.size() ? c->rep_changed[k] : 0;
  return 0;
}
