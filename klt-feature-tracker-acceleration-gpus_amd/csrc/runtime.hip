// runtime.hip -- host side of libklt_amd.so: device contexts and their streams,
// the exit hook, frame uploads, the setters and getters, selection, timing and
// the self-tests of the klt_hip_* C ABI declared in include/klt_hip.h.  The
// pyramid, tracking and batched entry points are runtime_pyr.hip,
// runtime_track.hip and runtime_frames.hip (runtime.h).  No kernels here.
#include "runtime.h"

int kltdev::ctx_fail(klt_hip_ctx *c, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return -1;
}

namespace {
// the pyramid stream: normal priority, or the lowest (KLT_PSTREAM_PRIO=low:
// the tracking stream's short kernels between two chunks -- the exchange, the
// processing order -- are then dispatched ahead of queued pyramid workgroups)
hipError_t make_pstream(klt_hip_ctx *c) {
  static const bool low = [] {
    const char *v = getenv("KLT_PSTREAM_PRIO");
    return v && strcmp(v, "low") == 0;
  }();
  if (!low) return hipStreamCreateWithFlags(&c->pstream, hipStreamNonBlocking);
  int least = 0, greatest = 0;
  const hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) return e;
  return hipStreamCreateWithPriority(&c->pstream, hipStreamNonBlocking, least);
}
}  // namespace

// the pyramid stream and the events of the two-stream pipelines (the slot
// rotation of klt_hip_track_sequence, the banks of the batched calls), once
int ensure_pipeline(klt_hip_ctx *c) {
  if (c->pstream) return 0;
  HIPCHK(c, make_pstream(c));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_start, hipEventDisableTiming));
  for (int k = 0; k < 3; ++k) {
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_built[k], hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_free[k], hipEventDisableTiming));
  }
  return 0;
}

namespace {
// ---------------------------------------------------------------------------
// Process exit.  hipcc's module constructor of each translation unit with
// kernels registers the code object at load time and an atexit handler that
// unregisters it (the runtime*.hip units have no kernels and register none); the
// HIP runtime (and a profiler's tool library, e.g. rocprofv3) tear down in
// their own exit handlers.  Anything of ours still holding the code object's
// kernels or HIP state at that point -- the selection engine's instantiated
// graphs of every live or parked context, the host sort pool's threads --
// is released by exit_hook, which atexit() runs BEFORE those handlers because
// it is registered after them (at the first context's creation).
// ---------------------------------------------------------------------------
std::mutex g_live_m;
std::set<klt_hip_ctx *> *g_live = new std::set<klt_hip_ctx *>();  // never destroyed: exit_hook reads it
std::atomic<bool> g_exiting{false};

// a live (or parked) context's host side of the upload pipelines, released
// at exit after the device is drained: its copy-pool threads (idle between
// calls, blocked on a condition variable inside this library) are joined, the
// copy streams destroyed, the caller's page-locked buffers unregistered and
// the pinned staging freed, so none of it is left to the HIP runtime's own
// exit-time teardown.  Everything is re-created on demand, should a later
// exit handler still call in.
void exit_release_host(klt_hip_ctx *c) {
  delete c->pool;
  c->pool = nullptr;
  for (hipStream_t *st : {&c->cstream, &c->dstream})
    if (*st) {
      (void)hipStreamDestroy(*st);
      *st = nullptr;
    }
  for (auto &r : c->registered) (void)hipHostUnregister(const_cast<unsigned char *>(r.first));
  c->registered.clear();
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  if (c->h_rows) (void)hipHostFree(c->h_rows);
  c->h_stage = nullptr;
  c->h_rows = nullptr;
  c->stage_cap = c->hrows_cap = 0;
  for (unsigned **p : {&c->d_exits, &c->d_exit_sig}) {  // the device is drained, nothing waits on the signal
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  c->exits_base = 0;
}

void exit_hook() {
  g_exiting.store(true, std::memory_order_release);
  std::lock_guard<std::mutex> lk(g_live_m);
  std::set<int> devs;
  for (klt_hip_ctx *c : *g_live) devs.insert(c->device);
  for (int d : devs)  // a look-ahead refinement's graph, a copy stream's last DMA may still be in flight
    if (hipSetDevice(d) == hipSuccess) (void)hipDeviceSynchronize();
  static const bool release_host = [] {  // KLT_EXIT_RELEASE=0 (A/B): the round-5 hook
    const char *e = getenv("KLT_EXIT_RELEASE");
    return !(e && *e == '0');
  }();
  for (klt_hip_ctx *c : *g_live) {
    sel_engine_release_graphs(c->sel);
    if (release_host && hipSetDevice(c->device) == hipSuccess) exit_release_host(c);
  }
  sel_pool_shutdown();
}
}  // namespace

bool kltdev::lib_exiting() { return g_exiting.load(std::memory_order_acquire); }

namespace {
void live_add(klt_hip_ctx *c) {
  static std::once_flag once;
  std::call_once(once, [] { atexit(exit_hook); });
  std::lock_guard<std::mutex> lk(g_live_m);
  g_live->insert(c);
}

void live_remove(klt_hip_ctx *c) {
  std::lock_guard<std::mutex> lk(g_live_m);
  g_live->erase(c);
}

// wait for what a caller's stream holds of this context's work: the event
// recorded when the context left it, and the stream still set (which must be
// valid until klt_hip_set_stream(c, NULL), the reset or the destroy)
int drain_caller(klt_hip_ctx *c) {
  if (c->stream && c->stream != c->own) {
    // an earlier caller stream's record (A -> own -> B) is waited for before
    // the event is re-recorded on the current one, which would overwrite it
    if (c->caller_pending) {
      HIPCHK(c, hipEventSynchronize(c->ev_caller));
      c->caller_pending = false;
    }
    if (!c->ev_caller) HIPCHK(c, hipEventCreateWithFlags(&c->ev_caller, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_caller, c->stream));
    c->caller_pending = true;
  }
  if (c->caller_pending) {
    HIPCHK(c, hipEventSynchronize(c->ev_caller));
    c->caller_pending = false;
  }
  return 0;
}
}  // namespace

KLT_API int klt_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

KLT_API klt_hip_ctx *klt_hip_ctx_create(int device) {
  klt_hip_ctx *c = new klt_hip_ctx();
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  c->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return nullptr;
  }
  c->stream = c->own;
  for (int i = 0; i < 2; ++i) hipEventCreateWithFlags(&c->u8_done[i], hipEventDisableTiming);
  live_add(c);
  return c;
}

KLT_API void klt_hip_ctx_destroy(klt_hip_ctx *c) {
  if (!c) return;
  live_remove(c);
  hipSetDevice(c->device);
  (void)drain_caller(c);
  if (c->own) hipStreamSynchronize(c->own);
  if (c->pstream) hipStreamSynchronize(c->pstream);
  for (auto &S : c->slot)
    for (auto &L : S.lv) hipFree(L.img);  // one block per level
  for (int i = 0; i < 2; ++i) {
    hipFree(c->d_u8[i]);
    if (c->h_u8[i]) hipHostFree(c->h_u8[i]);
    if (c->u8_done[i]) hipEventDestroy(c->u8_done[i]);
    hipFree(c->d_tmp[i]);
  }
  free_banks(c);
  for (int k = 0; k < 3; ++k) {
    if (c->banks.ev_built[k]) hipEventDestroy(c->banks.ev_built[k]);
    if (c->banks.ev_free[k]) hipEventDestroy(c->banks.ev_free[k]);
  }
  hipFree(c->d_perm);
  hipFree(c->d_count);
  hipFree(c->d_trk_count);
  for (hipStream_t st : {c->cstream, c->dstream})
    if (st) {
      hipStreamSynchronize(st);
      hipStreamDestroy(st);
    }
  for (int k = 0; k < 2; ++k)
    for (hipEvent_t e : {c->ev_ring_free[k], c->ev_dma[k], c->ev_tracked[k], c->ev_rows[k]})
      if (e) hipEventDestroy(e);
  hipFree(c->d_ring);
  hipFree(c->d_rows);
  delete c->pool;
  if (c->h_stage) hipHostFree(c->h_stage);
  if (c->h_rows) hipHostFree(c->h_rows);
  hipFree(c->d_hs);
  hipFree(c->d_feat);
  if (c->h_feat) hipHostFree(c->h_feat);
  hipFree(c->d_eig);
  hipFree(c->d_rep_map);
  hipFree(c->d_pred);
  if (c->h_rep) hipHostFree(c->h_rep);
  if (c->ev_rep) hipEventDestroy(c->ev_rep);
  sel_engine_destroy(c->sel);
  for (auto &r : c->registered) (void)hipHostUnregister(const_cast<unsigned char *>(r.first));
  for (void *p : {(void *)c->d_aff_store, (void *)c->d_aff, (void *)c->d_xp, (void *)c->d_yp, (void *)c->d_astage,
                  (void *)c->d_astate, (void *)c->d_aidx})
    hipFree(p);
  for (auto e : c->ev_pool) hipEventDestroy(e);
  for (auto &v : c->ev_used)
    for (auto &p : v) {
      hipEventDestroy(p.first);
      hipEventDestroy(p.second);
    }
  if (c->pstream) {
    hipStreamSynchronize(c->pstream);
    hipStreamDestroy(c->pstream);
  }
  for (int k = 0; k < KLT_HIP_MAX_SLOTS; ++k) {
    if (c->ev_built[k]) hipEventDestroy(c->ev_built[k]);
    if (c->ev_free[k]) hipEventDestroy(c->ev_free[k]);
  }
  if (c->ev_start) hipEventDestroy(c->ev_start);
  if (c->ev_caller) hipEventDestroy(c->ev_caller);
  if (c->ev_go) hipEventDestroy(c->ev_go);
  hipFree(c->d_exits);
  hipFree(c->d_exit_sig);
  if (c->own) hipStreamDestroy(c->own);
  delete c;
}

int forget_kept(klt_hip_ctx *c) {
  if (c->banks.drop_ahead() && c->pstream) HIPCHK(c, hipStreamSynchronize(c->pstream));  // a band call's build-ahead
  c->frames_ready = false;
  c->prev = PrevRef{};
  return 0;
}

KLT_API int klt_hip_current_device(void) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) return -1;
  return d;
}

KLT_API int klt_hip_ctx_device(klt_hip_ctx *c) { return c ? c->device : -1; }

// Device bytes a cached context keeps at most (klt_hip_ctx_reset): larger
// bank arenas, upload rings and staging are freed when it is parked.
constexpr size_t kKeepBytes = (size_t)2 << 30;

KLT_API size_t klt_hip_ctx_footprint(klt_hip_ctx *c) {
  if (!c) return 0;
  size_t b = c->banks.arena_bytes + c->ring_cap + c->drows_cap + c->hs_cap * sizeof(float) +
             c->eig_cap * sizeof(int) + c->u8_cap * 2 + (c->tmp_cap[0] + c->tmp_cap[1]) * sizeof(float);
  for (const auto &S : c->slot)
    for (const auto &L : S.lv) b += 3 * L.cap * sizeof(float);
  if (!c->banks.arena)
    for (const auto &K : c->banks.bank) {
      for (const auto &L : K.lv) b += 3 * L.cap * sizeof(float);
      b += K.hs_cap * sizeof(float);
    }
  return b;
}

KLT_API int klt_hip_ctx_reset(klt_hip_ctx *c) {
  if (!c) return -1;
  if (use_device(c)) return -1;
  // nothing of the previous owner is still running: the context's own streams,
  // and a caller's stream through drain_caller (an event recorded on it, so a
  // stream the caller has switched away from and destroyed is never touched)
  if (drain_caller(c)) return -1;
  for (hipStream_t st : {c->own, c->pstream, c->cstream, c->dstream})
    if (st) HIPCHK(c, hipStreamSynchronize(st));
  if (klt_hip_ctx_footprint(c) > kKeepBytes) {
    free_banks(c);
    hipFree(c->d_ring);
    hipFree(c->d_rows);
    c->d_ring = nullptr;
    c->d_rows = nullptr;
    c->ring_cap = c->drows_cap = 0;
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->h_rows) hipHostFree(c->h_rows);
    c->h_stage = nullptr;
    c->h_rows = nullptr;
    c->stage_cap = c->hrows_cap = 0;
  }
  if (c->copy_threads != default_host_threads()) {
    delete c->pool;  // idle between calls; joined here
    c->pool = nullptr;
    c->copy_threads = default_host_threads();
  }
  c->feat_mode = 2;
  for (auto &r : c->registered) (void)hipHostUnregister(const_cast<unsigned char *>(r.first));
  c->registered.clear();
  if (c->sel) sel_engine_set_threshold(c->sel, sel_default_threshold());
  c->bank_budget = 0;
  c->chunk_used = 0;
  c->stream = c->own;
  c->force_generic = 0;
  c->frame_format = KLT_HIP_FRAME_GRAY8;
  c->track_order = 0;
  c->track_patch = 1;
  c->track_merge = 1;
  c->lazy_grad = KLT_LAZY_GRAD_DEFAULT;
  c->l0_strip = 1;
  c->track_prio = 1;
  c->track_impl = 0;
  c->track_kernel = nullptr;  // klt_hip_track_kernel: "" before the next owner's first launch
  c->fb_on = 0;
  c->fb_dist = 0.0f;
  c->mask = nullptr;
  c->mask_pitch = 0;
  c->mask_flags = 0;
  c->fb_tab = nullptr;
  c->fb_stride = 0;
  c->pred_on = 0;
  c->pred_vx = c->pred_vy = nullptr;
  c->pred_tvx = c->pred_tvy = nullptr;
  c->pred_stride = 0;
  c->aff_on = 0;
  c->aff_dev = nullptr;
  c->aff_state_dev = nullptr;
  c->aff_tab = nullptr;
  c->aff_stab = nullptr;
  c->aff_tab_stride = 0;
  c->aff_fresh = 1;
  c->aff_depth = 0;
  c->rep_on = 0;
  c->rep_frames = c->rep_runs = c->rep_filled = 0;
  c->rep_changed.clear();
  c->eig_kernel = nullptr;
  c->frames_sched = kSchedOne;
  c->tail_left = kTailLeftDefault;
  c->wave_t = nullptr;
  c->ahead_ready = 0;
  c->prof = nullptr;
  if (forget_kept(c)) return -1;
  c->timing = false;
  for (int k = 0; k < T_N; ++k) {
    for (auto &p : c->ev_used[k]) {
      c->ev_pool.push_back(p.first);
      c->ev_pool.push_back(p.second);
    }
    c->ev_used[k].clear();
    c->frames_timed[k] = 0;
  }
  hipFree(c->d_trk_count);
  c->d_trk_count = nullptr;
  c->perm_n = -1;
  for (auto &S : c->slot) S.fused = -1;
  c->err.clear();
  return 0;
}

KLT_API const char *klt_hip_last_error(klt_hip_ctx *c) { return c ? c->err.c_str() : "null context"; }

KLT_API const char *klt_hip_track_kernel(klt_hip_ctx *c) { return c && c->track_kernel ? c->track_kernel : ""; }

KLT_API const char *klt_hip_eigen_kernel(klt_hip_ctx *c) { return c && c->eig_kernel ? c->eig_kernel : ""; }

KLT_API int klt_hip_set_stream(klt_hip_ctx *c, void *stream) {
  if (!c) return -1;
  const hipStream_t next = stream ? (hipStream_t)stream : c->own;
  if (next != c->stream && c->stream != c->own) {
    // leaving a caller's stream: remember its last work (drain_caller)
    if (use_device(c)) return -1;
    if (c->caller_pending) HIPCHK(c, hipEventSynchronize(c->ev_caller));
    if (!c->ev_caller) HIPCHK(c, hipEventCreateWithFlags(&c->ev_caller, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->ev_caller, c->stream));
    c->caller_pending = true;
  }
  c->stream = next;
  return 0;
}

KLT_API void *klt_hip_get_stream(klt_hip_ctx *c) { return c ? (void *)c->stream : nullptr; }

KLT_API int klt_hip_sync(klt_hip_ctx *c) {
  if (use_device(c)) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

KLT_API int klt_hip_upload_frame(klt_hip_ctx *c, int buf, const unsigned char *host, int ncols,
                                 int nrows) {
  if (buf < 0 || buf > 1 || !host || ncols < 0 || nrows < 0) return fail(c, "upload: bad arguments");
  if (use_device(c)) return -1;
  const size_t n = (size_t)ncols * nrows;
  if (n > c->u8_cap) {
    for (int i = 0; i < 2; ++i) {
      HIPCHK(c, hipStreamSynchronize(c->stream));
      hipFree(c->d_u8[i]);
      if (c->h_u8[i]) hipHostFree(c->h_u8[i]);
      c->d_u8[i] = nullptr;
      c->h_u8[i] = nullptr;
      HIPCHK(c, hipMalloc((void **)&c->d_u8[i], n));
      HIPCHK(c, hipHostMalloc((void **)&c->h_u8[i], n, hipHostMallocDefault));
    }
    c->u8_cap = n;
  }
  // a frame inside a registered caller buffer: one DMA straight from it.
  // Measured slower (round 4, per registered call): k_pyr_l0 reading the
  // caller's mapped pages over the bus, no copy at all, 120-122 against
  // 107-108 us (tools/exp/r04q.sh); a copy kernel on the tracking stream
  // reading them (no copy-engine hand-off), 116-117 against 106 us
  // (tools/exp/r04t.sh).
  for (size_t i = 0; i < c->registered.size(); ++i) {
    const auto &r = c->registered[i];
    if (host >= r.first && n <= r.second && (size_t)(host - r.first) <= r.second - n) {
      HIPCHK(c, hipMemcpyAsync(c->d_u8[buf], host, n, hipMemcpyHostToDevice, c->stream));
      // no u8_done record: it guards the pinned bounce buffer, which this DMA
      // does not touch, and a marker between the DMA and level 0 cost the
      // call 2 us (100.8 against 102.8 us, tools/exp/r06_regevent_ab.sh)
      c->u8_w[buf] = ncols;
      c->u8_h[buf] = nrows;
      return 0;
    }
  }
  // the previous copy out of this bounce buffer must have finished
  HIPCHK(c, hipEventSynchronize(c->u8_done[buf]));
  // in groups: the host pool copies group g+1 into pinned memory while group
  // g's DMA runs
  ensure_pool(c);
  const size_t G = upload_groups(), piece = copy_piece();
  const size_t group = n >= (1u << 20) ? (((n + G - 1) / G + 63) & ~(size_t)63) : n;
  // KLT_UPLOAD_TRACE=1: per group, the host copy and the DMA's enqueue (us) on stderr
  static const bool trace = [] {
    const char *e = getenv("KLT_UPLOAD_TRACE");
    return e && *e == '1';
  }();
  char tl[512];
  int tn = 0, nq = 0;
  double t0 = trace ? wall_us() : 0.0;
  const auto enqueue = [&](size_t o, size_t m) -> int {
    ++nq;
    const double t1 = trace ? wall_us() : 0.0;
    HIPCHK(c, hipMemcpyAsync(c->d_u8[buf] + o, c->h_u8[buf] + o, m, hipMemcpyHostToDevice, c->stream));
    if (trace) {
      const double t2 = wall_us();
      if (tn < (int)sizeof tl - 40) tn += snprintf(tl + tn, sizeof tl - tn, " copy=%.1f enq=%.1f", t1 - t0, t2 - t1);
      t0 = t2;
    }
    return 0;
  };
  if (c->pool && upload_pipelined()) {
    // one generation of the pool over every piece; each group (whole pieces)
    // is DMAed as soon as its pieces are in pinned memory.  Each DMA costs
    // ~10 us besides its bytes (tools/exp/r06_upload_pipe_ab.sh: 16 groups
    // ~120 us slower than 4), so few groups, the first one short: its DMA
    // starts early and the rest's copy runs beside it
    const size_t np = (n + piece - 1) / piece;
    size_t end[64], ng = 0;
    if (n < (1u << 20) || G == 1 || np < G) {
      end[ng++] = np;
    } else {
      const double f = upload_first();
      size_t e0 = f > 0 ? (size_t)(f * (double)np + 0.5) : (np + G - 1) / G;
      e0 = e0 < 1 ? 1 : e0 > np - (G - 1) ? np - (G - 1) : e0;
      end[ng++] = e0;
      for (size_t g = 1; g < G; ++g) end[ng++] = e0 + ((np - e0) * g + (G - 2)) / (G - 1);
      end[ng - 1] = np;
    }
    try {
      if (c->pool->parallel_groups(
              end, ng,
              [&](size_t t) {
                const size_t q = t * piece;
                copy_stream(c->h_u8[buf] + q, host + q, n - q < piece ? n - q : piece);
              },
              [&](size_t g) {
                const size_t o = (g ? end[g - 1] : 0) * piece, e = end[g] * piece < n ? end[g] * piece : n;
                return enqueue(o, e - o);
              }))
        return -1;
    } catch (...) {
      return fail(c, "upload: host task failed (out of memory?)");
    }
  } else {
    for (size_t o = 0; o < n; o += group) {
      const size_t m = n - o < group ? n - o : group;
      unsigned char *dst = c->h_u8[buf] + o;
      const unsigned char *src = host + o;
      if (host_parallel(c, (m + piece - 1) / piece, [&](size_t t) {
            const size_t q = t * piece;
            copy_stream(dst + q, src + q, m - q < piece ? m - q : piece);
          }))
        return -1;
      if (enqueue(o, m)) return -1;
    }
  }
  if (trace) fprintf(stderr, "uptrace groups=%d%s\n", nq, tn ? tl : "");
  HIPCHK(c, hipEventRecord(c->u8_done[buf], c->stream));
  c->u8_w[buf] = ncols;
  c->u8_h[buf] = nrows;
  return 0;
}

KLT_API int klt_hip_set_path(klt_hip_ctx *c, int force_generic) {
  if (!c) return -1;
  c->force_generic = force_generic != 0;
  return 0;
}



KLT_API int klt_hip_set_prof(klt_hip_ctx *c, void *dev) {
  if (!c) return fail(c, "set_prof: null context");
  c->prof = (unsigned long long *)dev;  // written by the instrumented tracker only (KLT_TRACK_PROF)
  return 0;
}

KLT_API int klt_hip_set_host_threads(klt_hip_ctx *c, int workers) {
  if (!c) return fail(c, "set_host_threads: null context");
  if (workers < 0 || workers > kMaxCopyThreads)
    return fail(c, "set_host_threads: %d workers (0..%d)", workers, kMaxCopyThreads);
  if (workers != c->copy_threads) {
    delete c->pool;  // its workers are idle between calls; joined here
    c->pool = nullptr;
    c->copy_threads = workers;
  }
  return 0;
}

KLT_API int klt_hip_register_host(klt_hip_ctx *c, const void *ptr, size_t bytes) {
  if (!c || !ptr || !bytes) return fail(c, "register_host: bad argument");
  const unsigned char *p = static_cast<const unsigned char *>(ptr);
  for (const auto &r : c->registered)
    if (p < r.first + r.second && r.first < p + bytes)
      return fail(c, "register_host: [%p, +%zu) overlaps a registered buffer", ptr, bytes);
  if (use_device(c)) return -1;
  HIPCHK(c, hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterMapped));
  c->registered.push_back({p, bytes});
  return 0;
}

KLT_API int klt_hip_unregister_host(klt_hip_ctx *c, const void *ptr) {
  if (!c || !ptr) return fail(c, "unregister_host: bad argument");
  for (size_t i = 0; i < c->registered.size(); ++i)
    if (c->registered[i].first == ptr) {
      if (use_device(c)) return -1;
      // no upload still reads it: the context's streams drain first
      for (hipStream_t st : {c->stream, c->own, c->pstream, c->cstream})
        if (st) HIPCHK(c, hipStreamSynchronize(st));
      HIPCHK(c, hipHostUnregister(const_cast<void *>(ptr)));
      c->registered.erase(c->registered.begin() + (long)i);
      return 0;
    }
  return fail(c, "unregister_host: %p is not registered", ptr);
}

KLT_API int klt_hip_set_bank_budget(klt_hip_ctx *c, size_t bytes) {
  if (!c) return fail(c, "set_bank_budget: null context");
  c->bank_budget = bytes;
  return 0;
}

KLT_API size_t klt_hip_get_bank_budget(klt_hip_ctx *c) { return c ? bank_budget_of(c) : 0; }

KLT_API int klt_hip_frames_chunk(klt_hip_ctx *c) { return c ? c->chunk_used : -1; }

KLT_API int klt_hip_get_host_threads(klt_hip_ctx *c) { return c ? c->copy_threads : -1; }

KLT_API int klt_hip_set_ahead_ready(klt_hip_ctx *c, int ready) {
  if (!c) return -1;
  c->ahead_ready = ready != 0;
  return 0;
}

KLT_API int klt_hip_set_frames_overlap(klt_hip_ctx *c, int overlap) {
  if (!c) return fail(c, "set_frames_overlap: null context");
  if (overlap < kSchedOne || overlap > kSchedTail)
    return fail(c, "set_frames_overlap: schedule %d (0 one stream, 1 automatic, 2 beside, 3 tail)", overlap);
  c->frames_sched = overlap;
  return 0;
}

KLT_API int klt_hip_set_frames_tail(klt_hip_ctx *c, int waves_left) {
  if (!c) return fail(c, "set_frames_tail: null context");
  if (waves_left < 0) return fail(c, "set_frames_tail: %d waves left", waves_left);
  c->tail_left = waves_left;
  return 0;
}

// base + launched - waves_left, the counter value at which at most waves_left
// of the `launched` waves counted on top of `base` are still to leave; 0 (no
// wait) when that many may be left from the start.  1 <= *threshold - base <=
// launched: reached by the launch's own completion at the latest, never before
// its first wave has left.
KLT_API int klt_hip_tail_threshold(unsigned base, unsigned launched, unsigned waves_left, unsigned *threshold) {
  if (launched == 0 || launched <= waves_left) return 0;
  if (threshold) *threshold = base + (launched - waves_left);
  return 1;
}

KLT_API int klt_hip_set_wave_times(klt_hip_ctx *c, void *dev) {
  if (!c) return fail(c, "set_wave_times: null context");
  c->wave_t = (unsigned long long *)dev;
  return 0;
}

KLT_API int klt_hip_set_track_patch(klt_hip_ctx *c, int on) {
  if (!c) return fail(c, "set_track_patch: null context");
  c->track_patch = on ? 1 : 0;
  return 0;
}


KLT_API int klt_hip_set_lazy_grad(klt_hip_ctx *c, int on) {
  if (!c) return fail(c, "set_lazy_grad: null context");
  c->lazy_grad = on ? 1 : 0;
  return 0;
}

KLT_API int klt_hip_set_l0_strip(klt_hip_ctx *c, int on) {
  if (!c) return fail(c, "set_l0_strip: null context");
  c->l0_strip = on ? 1 : 0;
  return 0;
}

KLT_API int klt_hip_set_track_merge(klt_hip_ctx *c, int on) {
  if (!c) return fail(c, "set_track_merge: null context");
  c->track_merge = on ? 1 : 0;
  return 0;
}

KLT_API int klt_hip_set_track_prio(klt_hip_ctx *c, int on) {
  if (!c) return fail(c, "set_track_prio: null context");
  c->track_prio = on ? 1 : 0;
  return 0;
}

KLT_API int klt_hip_set_track_impl(klt_hip_ctx *c, int impl) {
  if (!c || impl < 0 || impl > 1) return fail(c, "set_track_impl: 0 (default kernel) or 1 (generic)");
  c->track_impl = impl;
  return 0;
}

KLT_API int klt_hip_set_fb(klt_hip_ctx *c, int on, float max_dist) {
  if (!c) return fail(c, "set_fb: null context");
  if (!(max_dist >= 0.0f) || !isfinite(max_dist))
    return fail(c, "set_fb: max_dist %g must be finite and >= 0", (double)max_dist);
  c->fb_on = on ? 1 : 0;
  c->fb_dist = max_dist;
  return 0;
}

KLT_API int klt_hip_get_fb(klt_hip_ctx *c, int *on, float *max_dist) {
  if (!c) return fail(c, "get_fb: null context");
  if (on) *on = c->fb_on;
  if (max_dist) *max_dist = c->fb_dist;
  return 0;
}

KLT_API int klt_hip_set_fb_table(klt_hip_ctx *c, float *dev_err, long stride) {
  if (!c) return fail(c, "set_fb_table: null context");
  if (dev_err && stride < 1) return fail(c, "set_fb_table: stride %ld < 1", stride);
  c->fb_tab = dev_err;
  c->fb_stride = dev_err ? stride : 0;
  return 0;
}

KLT_API int klt_hip_set_predict(klt_hip_ctx *c, int on, float *dev_vx, float *dev_vy) {
  if (!c) return fail(c, "set_predict: null context");
  if (on && (!dev_vx || !dev_vy)) return fail(c, "set_predict: null state array");
  c->pred_on = on ? 1 : 0;
  c->pred_vx = on ? dev_vx : nullptr;
  c->pred_vy = on ? dev_vy : nullptr;
  return 0;
}

KLT_API int klt_hip_get_predict(klt_hip_ctx *c, int *on, float **dev_vx, float **dev_vy) {
  if (!c) return fail(c, "get_predict: null context");
  if (on) *on = c->pred_on;
  if (dev_vx) *dev_vx = c->pred_vx;
  if (dev_vy) *dev_vy = c->pred_vy;
  return 0;
}

KLT_API int klt_hip_set_predict_table(klt_hip_ctx *c, float *dev_tab_vx, float *dev_tab_vy, long stride) {
  if (!c) return fail(c, "set_predict_table: null context");
  if ((dev_tab_vx != nullptr) != (dev_tab_vy != nullptr)) return fail(c, "set_predict_table: give both tables or none");
  if (dev_tab_vx && stride < 1) return fail(c, "set_predict_table: stride %ld < 1", stride);
  c->pred_tvx = dev_tab_vx;
  c->pred_tvy = dev_tab_vy;
  c->pred_stride = dev_tab_vx ? stride : 0;
  return 0;
}

KLT_API int klt_hip_set_mask(klt_hip_ctx *c, const unsigned char *dev_mask, long pitch, int flags) {
  if (!c) return fail(c, "set_mask: null context");
  if (flags & ~(KLT_HIP_MASK_SELECT | KLT_HIP_MASK_TRACK))
    return fail(c, "set_mask: flags %#x (KLT_HIP_MASK_SELECT | KLT_HIP_MASK_TRACK)", (unsigned)flags);
  if (dev_mask && flags && pitch < 1) return fail(c, "set_mask: pitch %ld < 1", pitch);
  const bool on = dev_mask && flags;
  c->mask = on ? dev_mask : nullptr;
  c->mask_pitch = on ? pitch : 0;
  c->mask_flags = on ? flags : 0;
  return 0;
}

KLT_API int klt_hip_get_mask(klt_hip_ctx *c, const unsigned char **dev_mask, long *pitch, int *flags) {
  if (!c) return fail(c, "get_mask: null context");
  if (dev_mask) *dev_mask = c->mask;
  if (pitch) *pitch = c->mask_pitch;
  if (flags) *flags = c->mask_flags;
  return 0;
}

KLT_API int klt_hip_set_track_count(klt_hip_ctx *c, int on) {
  if (!c) return fail(c, "set_track_count: null context");
  if (use_device(c)) return -1;
  HIPCHK(c, hipDeviceSynchronize());  // no tracker launch still holds the old pointer
  if (!on) {
    hipFree(c->d_trk_count);
    c->d_trk_count = nullptr;
    return 0;
  }
  const size_t bytes = 2 * kCountSlots * sizeof(unsigned long long);
  if (!c->d_trk_count) HIPCHK(c, hipMalloc((void **)&c->d_trk_count, bytes));
  HIPCHK(c, hipMemset(c->d_trk_count, 0, bytes));
  return 0;
}

KLT_API int klt_hip_get_track_count(klt_hip_ctx *c, unsigned long long *solves, unsigned long long *passes,
                                    int reset) {
  if (!c || !solves || !passes) return fail(c, "get_track_count: null argument");
  if (!c->d_trk_count) return fail(c, "get_track_count: counting is off (klt_hip_set_track_count)");
  if (use_device(c)) return -1;
  unsigned long long h[2 * kCountSlots];
  HIPCHK(c, hipDeviceSynchronize());  // every stream the tracker may have run on
  HIPCHK(c, hipMemcpy(h, c->d_trk_count, sizeof h, hipMemcpyDeviceToHost));
  *solves = *passes = 0;
  for (int k = 0; k < kCountSlots; ++k) {
    *solves += h[k];
    *passes += h[kCountSlots + k];
  }
  if (reset) HIPCHK(c, hipMemset(c->d_trk_count, 0, sizeof h));
  return 0;
}

KLT_API int klt_hip_set_track_order(klt_hip_ctx *c, int input_order) {
  if (!c) return fail(c, "set_track_order: null context");
  c->track_order = input_order ? 1 : 0;
  c->perm_n = -1;  // the cached processing order is dropped: the next call sorts afresh
  c->perm_age = 0;
  return 0;
}

KLT_API int klt_hip_min_eigen(klt_hip_ctx *c, int s, const klt_hip_select_desc *d, int *vals, int *nx,
                              int *ny) {
  if (!c || !d) return fail(c, "min_eigen: null argument");
  if (s < 0 || s >= KLT_HIP_MAX_SLOTS || c->slot[s].nlev < 1) return fail(c, "min_eigen: bad slot");
  const Level &L = c->slot[s].lv[0];
  const SelGrid g = sel_grid(*d, L.w, L.h);
  const int hw = g.hw, hh = g.hh, step = g.step, gx = g.nx, gy = g.ny;
  if (step < 1) return fail(c, "min_eigen: bad nSkippedPixels");
  const int bx = d->borderx, by = d->bordery;
  if (bx < hw || by < hh) return fail(c, "min_eigen: border smaller than window half size");
  *nx = gx;
  *ny = gy;
  if (!vals) return 0;
  const long np = (long)gx * gy;
  if (np == 0) return 0;
  if (use_device(c)) return -1;
  if (grow(c, &c->d_eig, &c->eig_cap, (size_t)np)) return -1;
  {
    TimedScope ts(c, T_EIG, c->stream);
    if (launched(c, "k_min_eigen", launch_min_eigen(c->stream, L.il ? L.img + kRecGx : L.gx, L.il ? L.img + kRecGy : L.gy,
                                                    L.w, L.il ? 3 : 1, bx, by, step, gx, gy, hw, hh, c->d_eig,
                                                    &c->eig_kernel)))
      return -1;
  }
  HIPCHK(c, hipMemcpyAsync(vals, c->d_eig, sizeof(int) * np, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// the trackability map of slot s into d_eig (k_min_eigen), grid nx x ny
static int eigen_to_dev(klt_hip_ctx *c, int s, const klt_hip_select_desc *d, int *nx, int *ny) {
  if (klt_hip_min_eigen(c, s, d, nullptr, nx, ny)) return -1;
  const long np = (long)*nx * *ny;
  if (np == 0) return 0;
  const Level &L = c->slot[s].lv[0];
  const SelGrid g = sel_grid(*d, L.w, L.h);
  if (grow(c, &c->d_eig, &c->eig_cap, (size_t)np)) return -1;
  TimedScope ts(c, T_EIG, c->stream);
  return launched(c, "k_min_eigen", launch_min_eigen(c->stream, L.il ? L.img + kRecGx : L.gx, L.il ? L.img + kRecGy : L.gy,
                                                     L.w, L.il ? 3 : 1, d->borderx, d->bordery, g.step, g.nx, g.ny, g.hw,
                                                     g.hh, c->d_eig, &c->eig_kernel));
}

static SelEngine *sel_of(klt_hip_ctx *c) {
  if (!c->sel) c->sel = sel_engine_create();
  return c->sel;
}


KLT_API int klt_hip_select(klt_hip_ctx *c, int s, const klt_hip_select_desc *d, int ncols, int nrows, int mindist,
                           int min_eigenvalue, int overwrite_all, float *x, float *y, int *val,
                           unsigned char *changed, int n) {
  if (!c || !d || (n > 0 && (!x || !y || !val || !changed))) return fail(c, "select: null argument");
  if (s < 0 || s >= KLT_HIP_MAX_SLOTS || c->slot[s].nlev < 1) return fail(c, "select: bad slot");
  if (c->slot[s].lv[0].w != ncols || c->slot[s].lv[0].h != nrows)
    return fail(c, "select: slot %d is %dx%d, image %dx%d", s, c->slot[s].lv[0].w, c->slot[s].lv[0].h, ncols, nrows);
  if (mask_refused(c, ncols, "select")) return -1;
  if (use_device(c)) return -1;
  int nx = 0, ny = 0;
  if (eigen_to_dev(c, s, d, &nx, &ny)) return -1;
  std::string e;
  if (sel_engine_run(sel_of(c), c->stream, c->d_eig, nx, ny, d->borderx, d->bordery, sel_step(*d), ncols, nrows, mindist < 0 ? 0 : mindist, min_eigenvalue, overwrite_all, x, y, val, changed, n, sel_mask(c),
                     c->mask_pitch, &e))
    return fail(c, "select: %s", e.c_str());
  return 0;
}

KLT_API int klt_hip_select_dev_map(klt_hip_ctx *c, const int *dev_map, int nx, int ny,
                                   const klt_hip_select_desc *d, int ncols, int nrows, int mindist,
                                   int min_eigenvalue, int overwrite_all, float *x, float *y, int *val,
                                   unsigned char *changed, int n) {
  if (!c || !d || (nx * ny > 0 && !dev_map) || (n > 0 && (!x || !y || !val || !changed)))
    return fail(c, "select_dev_map: null argument");
  if (mask_refused(c, ncols, "select_dev_map")) return -1;
  if (use_device(c)) return -1;
  std::string e;
  if (sel_engine_run(sel_of(c), c->stream, dev_map, nx, ny, d->borderx, d->bordery, sel_step(*d), ncols, nrows, mindist < 0 ? 0 : mindist, min_eigenvalue, overwrite_all, x, y, val, changed, n, sel_mask(c),
                     c->mask_pitch, &e))
    return fail(c, "select: %s", e.c_str());
  return 0;
}

KLT_API int klt_hip_select_tune(klt_hip_ctx *c, int threshold) {
  if (!c) return fail(c, "select_tune: null context");
  sel_engine_set_threshold(sel_of(c), threshold);
  return 0;
}

KLT_API int klt_hip_select_stats(klt_hip_ctx *c, long *downloaded, long *device_steps, long *visited,
                                 double *host_us) {
  if (!c || !downloaded || !device_steps || !visited) return fail(c, "select_stats: null argument");
  sel_engine_stats(sel_of(c), downloaded, device_steps, visited, host_us);
  return 0;
}

KLT_API int klt_hip_select_sort_test(klt_hip_ctx *c, const int *vals, int n, int *out_val, int *out_idx) {
  if (!c || n < 0 || (n > 0 && (!vals || !out_val || !out_idx))) return fail(c, "select_sort_test: bad argument");
  if (use_device(c)) return -1;
  if (n == 0) return 0;
  if (grow(c, &c->d_eig, &c->eig_cap, (size_t)n)) return -1;
  HIPCHK(c, hipMemcpyAsync(c->d_eig, vals, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
  std::string e;
  if (sel_engine_sort(sel_of(c), c->stream, c->d_eig, n, out_val, out_idx, &e))
    return fail(c, "select_sort_test: %s", e.c_str());
  return 0;
}

KLT_API int klt_hip_synth_frames(klt_hip_ctx *c, unsigned long long seed, int t0, int n, int ncols, int nrows,
                                 unsigned char *dev, long pitch, long fstride) {
  if (!c || !dev || n < 0 || pitch < ncols) return fail(c, "synth: bad arguments");
  if (use_device(c)) return -1;
  const long np = (long)ncols * nrows;
  if (np == 0 || n == 0) return 0;
  return launched(c, "k_synth", launch_synth(c->stream, seed, t0, n, ncols, nrows, 0, dev, pitch, fstride));
}

KLT_API int klt_hip_synth_rows(klt_hip_ctx *c, unsigned long long seed, int t0, int n, int ncols, int row0,
                               int nrows, unsigned char *dev, long pitch, long fstride) {
  if (!c || !dev || n < 0 || pitch < ncols || row0 < 0 || nrows < 0) return fail(c, "synth_rows: bad arguments");
  if (use_device(c)) return -1;
  if ((long)ncols * nrows == 0 || n == 0) return 0;
  return launched(c, "k_synth", launch_synth(c->stream, seed, t0, n, ncols, nrows, row0, dev, pitch, fstride));
}

KLT_API void *klt_hip_malloc(klt_hip_ctx *c, size_t bytes) {
  void *p = nullptr;
  if (!c || use_device(c)) return nullptr;
  if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
    fail(c, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return p;
}

KLT_API void klt_hip_free(klt_hip_ctx *c, void *p) {
  if (!c || !p) return;
  use_device(c);
  hipFree(p);
}

KLT_API int klt_hip_memcpy(klt_hip_ctx *c, void *dst, const void *src, size_t bytes, int kind) {
  if (use_device(c)) return -1;
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, (hipMemcpyKind)kind, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

KLT_API int klt_hip_set_timing(klt_hip_ctx *c, int on) {
  if (!c) return -1;
  c->timing = on != 0;
  return 0;
}

KLT_API int klt_hip_get_timing(klt_hip_ctx *c, klt_hip_timing *out) {
  if (!c || !out) return -1;
  if (klt_hip_sync(c)) return -1;
  double ms[T_N] = {0, 0, 0, 0, 0};
  int cnt[T_N] = {0, 0, 0, 0, 0};
  for (int k = 0; k < T_N; ++k) {
    for (auto &p : c->ev_used[k]) {
      float t = 0.0f;
      if (hipEventElapsedTime(&t, p.first, p.second) == hipSuccess) {
        ms[k] += t;
        cnt[k]++;
      }
      c->ev_pool.push_back(p.first);
      c->ev_pool.push_back(p.second);
    }
    c->ev_used[k].clear();
  }
  out->n_pyr_l0 = cnt[T_L0];
  out->ms_pyr_l0 = ms[T_L0];
  out->n_pyr_l1 = cnt[T_L1];
  out->ms_pyr_l1 = ms[T_L1];
  out->n_track = cnt[T_TRACK];
  out->ms_track = ms[T_TRACK];
  out->n_eigen = cnt[T_EIG];
  out->ms_eigen = ms[T_EIG];
  out->n_generic = cnt[T_GEN];
  out->ms_generic = ms[T_GEN];
  out->frames_pyr_l0 = c->frames_timed[T_L0];
  out->frames_pyr_l1 = c->frames_timed[T_L1];
  out->frames_track = c->frames_timed[T_TRACK];
  for (auto &f : c->frames_timed) f = 0;
  return 0;
}

KLT_API int klt_hip_selftest_sqrt(klt_hip_ctx *c, const double *in, double *out, int n) {
  if (use_device(c)) return -1;
  double *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, sizeof(double) * 2 * (n ? n : 1)));
  hipMemcpy(d, in, sizeof(double) * n, hipMemcpyHostToDevice);
  hipError_t e = launch_selftest_sqrt(d, d + n, n);
  if (e == hipSuccess) e = hipMemcpy(out, d + n, sizeof(double) * n, hipMemcpyDeviceToHost);
  hipFree(d);
  if (e != hipSuccess) return fail(c, "selftest_sqrt: %s", hipGetErrorString(e));
  return 0;
}

KLT_API int klt_hip_selftest_copy_pool(int workers, int rounds, size_t max_bytes) {
  if (workers < 0 || rounds < 0 || max_bytes < 1) return -1;
  std::vector<unsigned char> src(max_bytes), dst(max_bytes);
  HostPool pool(workers);
  unsigned long long r64 = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() {
    r64 ^= r64 << 13;
    r64 ^= r64 >> 7;
    r64 ^= r64 << 17;
    return r64;
  };
  for (int r = 0; r < rounds; ++r) {
    const size_t n = 1 + rnd() % max_bytes;
    const size_t piece = 1 + rnd() % (n < 65536 ? n : 65536);
    for (size_t i = 0; i < n; ++i) src[i] = (unsigned char)(rnd() >> 29);
    memset(dst.data(), 0, n);
    const std::function<void(size_t)> copy = [&](size_t t) {
      const size_t o = t * piece;
      memcpy(dst.data() + o, src.data() + o, n - o < piece ? n - o : piece);
    };
    pool.parallel((n + piece - 1) / piece, copy);
    if (memcmp(dst.data(), src.data(), n) != 0) return r + 1;
  }
  return 0;
}

KLT_API int klt_hip_selftest_div(klt_hip_ctx *c, const float *a, const float *b, float *out, int n) {
  if (use_device(c)) return -1;
  float *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, sizeof(float) * 3 * (n ? n : 1)));
  hipMemcpy(d, a, sizeof(float) * n, hipMemcpyHostToDevice);
  hipMemcpy(d + n, b, sizeof(float) * n, hipMemcpyHostToDevice);
  hipError_t e = launch_selftest_div(d, d + n, d + 2 * n, n);
  if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, sizeof(float) * n, hipMemcpyDeviceToHost);
  hipFree(d);
  if (e != hipSuccess) return fail(c, "selftest_div: %s", hipGetErrorString(e));
  return 0;
}

KLT_API int klt_hip_selftest_solve2(klt_hip_ctx *c, const float *sums, float step, float min_det, float *out, int *ok,
                                    int n) {
  if (use_device(c)) return -1;
  if (n < 0) return fail(c, "selftest_solve2: n < 0");
  const size_t m = n ? n : 1;
  float *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, sizeof(float) * 12 * m));  // 5 n sums, 6 n results, n flags
  float *dout = d + 5 * m;
  int *dok = reinterpret_cast<int *>(d + 11 * m);
  hipError_t e = hipMemcpy(d, sums, sizeof(float) * 5 * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_selftest_solve2(d, step, min_det, dout, dok, n);
  if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(float) * 6 * n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ok, dok, sizeof(int) * n, hipMemcpyDeviceToHost);
  hipFree(d);
  if (e != hipSuccess) return fail(c, "selftest_solve2: %s", hipGetErrorString(e));
  return 0;
}
