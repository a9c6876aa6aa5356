// host_pool.h -- the host copy pool of a device context (internal): the worker
// threads that copy pageable frames into pinned staging and hand table rows
// out, the non-temporal copy they run, and the environment knobs of the
// upload schedules.  No HIP in here (tools/hostcheck/copy_pool_tsan.sh).
#pragma once

#include <emmintrin.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// Host-side parallel work of klt_hip_track_frames_host: copies of the
// caller's pageable frames into pinned staging and the delivery of table rows
// to the caller's callback.  A few worker threads and the calling thread pull
// task indices of one generation; parallel() returns only when every worker
// has finished the generation, so no worker still runs the task function when
// the caller moves on to the next one.
struct HostPool {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv;
  const std::function<void(size_t)> *fn = nullptr;
  size_t ntasks = 0;
  std::atomic<size_t> next{0};
  std::atomic<int> finished{0};
  unsigned gen = 0;
  bool stop = false;

  explicit HostPool(int workers) {
    for (int i = 0; i < workers; ++i) th.emplace_back([this] { worker(); });
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> l(m);
      stop = true;
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
  void run() {
    for (size_t i; (i = next.fetch_add(1)) < ntasks;) (*fn)(i);
  }
  void worker() {
    unsigned seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
      }
      run();
      finished.fetch_add(1);
    }
  }
  // fn(0) .. fn(n-1) on the workers in one generation, the tasks taken in
  // index order; group g is tasks [end[g-1], end[g]) (end[ng-1] == n), and
  // on_group(g) runs on the calling thread, in group order, as soon as it
  // sees every task of group g done (one wake-up of the workers per call, not
  // one per group: a generation's wake-ups and its wait for the last worker
  // cost ~10 us, measured per group on the box, tools/exp/r06_upload_ab.sh).
  // The caller copies too while the tasks being claimed are its next
  // group's.  Returns the first non-zero on_group result (the remaining tasks
  // still run).
  template <class Fn, class OnGroup>
  int parallel_groups(const size_t *end, size_t ng, const Fn &f, const OnGroup &on_group) {
    constexpr size_t kMaxGroups = 64;
    if (ng == 0 || ng > kMaxGroups || end[ng - 1] == 0) return -1;
    const size_t n = end[ng - 1];
    std::atomic<unsigned> gd[kMaxGroups];
    for (size_t g = 0; g < ng; ++g) gd[g].store(0, std::memory_order_relaxed);
    const auto group_of = [&](size_t i) {
      size_t g = 0;
      while (i >= end[g]) ++g;
      return g;
    };
    const std::function<void(size_t)> task = [&](size_t i) {
      f(i);
      gd[group_of(i)].fetch_add(1, std::memory_order_release);
    };
    {
      std::lock_guard<std::mutex> l(m);
      fn = &task;
      ntasks = n;
      next = 0;
      finished = 0;
      ++gen;
    }
    cv.notify_all();
    int rc = 0;
    for (size_t g = 0; g < ng && rc == 0;) {
      const unsigned want = (unsigned)(end[g] - (g ? end[g - 1] : 0));
      if (gd[g].load(std::memory_order_acquire) == want) {
        rc = on_group(g);
        ++g;
        continue;
      }
      if (next.load(std::memory_order_relaxed) < end[g]) {
        const size_t i = next.fetch_add(1);
        if (i < n) task(i);
      } else {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
    }
    for (size_t i; (i = next.fetch_add(1)) < n;) task(i);  // an early error: finish the tasks here too
    while (finished.load() < (int)th.size()) std::this_thread::yield();
    return rc;
  }
  // fn(0) .. fn(n-1), on the workers and the calling thread
  void parallel(size_t n, const std::function<void(size_t)> &f) {
    {
      std::lock_guard<std::mutex> l(m);
      fn = &f;
      ntasks = n;
      next = 0;
      finished = 0;
      ++gen;
    }
    cv.notify_all();
    run();
    while (finished.load() < (int)th.size()) std::this_thread::yield();
  }
};

#pragma GCC visibility push(hidden)
constexpr int kMaxCopyThreads = 16;  // copy-pool workers per device context, at most

// host copy workers of a new context (KLT_AMD_HOST_THREADS; default 7) and
// the piece a worker copies at a time (KLT_AMD_COPY_PIECE bytes; default 64 KiB):
// tuning hooks, any value gives the same results
inline int default_host_threads() {
  static const int n = [] {
    const char *v = getenv("KLT_AMD_HOST_THREADS");
    const int x = v && *v ? atoi(v) : 7;
    return x < 0 ? 0 : x > kMaxCopyThreads ? kMaxCopyThreads : x;  // klt_hip_set_host_threads' range
  }();
  return n;
}
// DMAs a large per-call frame upload is split into (KLT_AMD_UPLOAD_GROUPS, A/B;
// default 2, round 5: 4): the host copies group g+1 into pinned memory while
// group g's DMA runs
inline size_t upload_groups() {
  static const size_t g = [] {
    const char *e = getenv("KLT_AMD_UPLOAD_GROUPS");
    const long v = e && *e ? atol(e) : 2;
    return (size_t)(v < 1 ? 1 : v > 64 ? 64 : v);
  }();
  return g;
}

// the per-call upload's groups in one pool generation (round 6; KLT_AMD_UPLOAD_PIPE=0:
// one generation per group, the round-5 schedule)
inline bool upload_pipelined() {
  static const bool v = [] {
    const char *e = getenv("KLT_AMD_UPLOAD_PIPE");
    return !(e && *e == '0');
  }();
  return v;
}

// the first DMA group's share of a pipelined per-call upload
// (KLT_AMD_UPLOAD_FIRST, a fraction, default 0.25; 0: equal groups)
inline double upload_first() {
  static const double v = [] {
    const char *e = getenv("KLT_AMD_UPLOAD_FIRST");
    const double x = e && *e ? atof(e) : 0.25;
    return x > 0 && x < 1 ? x : 0.0;
  }();
  return v;
}

inline size_t copy_piece() {
  static const size_t n = [] {
    const char *v = getenv("KLT_AMD_COPY_PIECE");
    const long x = v && *v ? atol(v) : 64L << 10;
    return (size_t)(x < 4096 ? 4096 : x);
  }();
  return n;
}

// copy into pinned staging with non-temporal stores: the destination is read
// only by the DMA engine, so its lines need not be fetched (no read-for-
// ownership) nor kept in the CPU caches
inline void copy_stream(unsigned char *dst, const unsigned char *src, size_t n) {
  size_t i = 0;
  const size_t head = (16 - ((uintptr_t)dst & 15)) & 15;
  if (head) {
    memcpy(dst, src, head < n ? head : n);
    i = head < n ? head : n;
  }
  for (; i + 64 <= n; i += 64) {
    const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i));
    const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i + 16));
    const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i + 32));
    const __m128i d = _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i + 48));
    _mm_stream_si128(reinterpret_cast<__m128i *>(dst + i), a);
    _mm_stream_si128(reinterpret_cast<__m128i *>(dst + i + 16), b);
    _mm_stream_si128(reinterpret_cast<__m128i *>(dst + i + 32), c);
    _mm_stream_si128(reinterpret_cast<__m128i *>(dst + i + 48), d);
  }
  if (i < n) memcpy(dst + i, src + i, n - i);
  _mm_sfence();  // the stores are globally visible before the DMA is queued
}
#pragma GCC visibility pop
