// replace_step.h -- the replacement of lost features inside the batched calls
// (internal): one step for the single-sequence calls (runtime_frames.hip) and
// the multi-sequence call (runtime_multi.hip), and the frame at which their
// tracker launch is cut for it.
#pragma once

#include "runtime.h"

#pragma GCC visibility push(hidden)

// the device lists of a batched call -- nseq sequences' features one after the
// other, sequence s at [first[s], first[s + 1]) of n -- and its device tables
struct RepLists {
  int nseq, n;
  const int *first;
  float *x, *y;
  int *val;
  float *tab_x, *tab_y;
  int *tab_val;
  long tab_stride;
};

// where a step counts: per feature `changed`, per sequence `runs` and
// `filled`; any may be null
struct RepCounters {
  unsigned char *changed;
  long *runs, *filled;
};

// the last frame (exclusive, at most F) of a tracker launch that starts at
// frame f0 of its bank with `count` frames tracked so far: cut where the count
// reaches a multiple of `every` (0: no replacement, no cut)
inline int next_cut(long count, int every, int f0, int F) {
  const long due = every > 0 ? every - count % every : F;
  return f0 + due < F ? (int)(f0 + due) : F;
}

// n features of x | y | val between the device lists and the pinned block:
// one transfer where the caller keeps the three arrays in one block
inline int move_lists(klt_hip_ctx *c, const RepLists &q, float *h, hipMemcpyKind kind, hipStream_t st) {
  const size_t nb = sizeof(float) * (size_t)q.n;
  const bool down = kind == hipMemcpyDeviceToHost;
  if (q.y == q.x + q.n && reinterpret_cast<float *>(q.val) == q.y + q.n) {
    HIPCHK(c, hipMemcpyAsync(down ? (void *)h : (void *)q.x, down ? (const void *)q.x : (const void *)h, 3 * nb, kind, st));
    return 0;
  }
  void *dev[3] = {q.x, q.y, q.val};
  for (int k = 0; k < 3; ++k) {
    float *hk = h + (size_t)k * q.n;
    HIPCHK(c, hipMemcpyAsync(down ? (void *)hk : dev[k], down ? (const void *)dev[k] : (const void *)hk, nb, kind, st));
  }
  return 0;
}

// One replacement for every sequence (KLTReplaceLostFeatures in sequential
// mode, each on its own list and its own frame) after the frame whose table
// row is `row`; the frames are w x h.  The lists come to the pinned block
// (x | y | val); `ahead()` queues whatever does not depend on them before the
// host waits.  The sequences with a lost slot -- the others are left alone --
// get their trackability maps from `maps(m, g)`, which fills c->d_rep_map
// where the frames lie and returns the ints from one map to the next
// (negative: failed); the selection engine fills each one's slots from its own
// map, one sequence after the other, and the lists and their table row go back
// to the device.  *filled_all: the slots filled in all sequences.
template <class Ahead, class Maps>
int replace_step(klt_hip_ctx *c, const RepLists &q, const klt_hip_replace_desc &d, int w, int h, long row,
                 const RepCounters &cnt, Ahead ahead, Maps maps, long *filled_all = nullptr) {
  const int n = q.n;
  if (n <= 0) return ahead();
  hipStream_t st = c->stream;
  if (ensure_rep_host(c, n, st)) return -1;
  float *hx = c->h_rep, *hy = hx + n;
  int *hv = reinterpret_cast<int *>(hy + n);
  if (move_lists(c, q, hx, hipMemcpyDeviceToHost, st)) return -1;
  HIPCHK(c, hipEventRecord(c->ev_rep, st));
  if (ahead()) return -1;
  HIPCHK(c, hipEventSynchronize(c->ev_rep));
  EigMultiArgs m;
  memset(&m, 0, sizeof m);
  for (int s = 0; s < q.nseq; ++s) {
    int lost = 0;
    for (int k = q.first[s]; k < q.first[s + 1]; ++k) lost += hv[k] < 0;
    if (lost) m.seq[m.nsel++] = s;
  }
  if (!m.nsel) return 0;  // KLTReplaceLostFeatures: nothing to replace
  const SelGrid g = sel_grid(d.sel, w, h);
  if (grow(c, &c->d_rep_map, &c->rep_map_cap, (size_t)g.nx * g.ny * m.nsel)) return -1;
  const long np = (long)g.nx * g.ny > 0 ? maps(m, g) : 0;
  if (np < 0) return -1;
  std::vector<unsigned char> changed((size_t)n, 0);
  long written = 0;
  for (int i = 0; i < m.nsel; ++i) {
    const int s = m.seq[i], a = q.first[s], ns = q.first[s + 1] - a;
    if (klt_hip_select_dev_map(c, c->d_rep_map + i * np, g.nx, g.ny, &d.sel, w, h, d.mindist, d.min_eigenvalue, 0, hx + a,
                               hy + a, hv + a, changed.data() + a, ns))
      return -1;
    long filled = 0;
    for (int k = a; k < a + ns; ++k) {
      if (!changed[k]) continue;
      if (cnt.changed) cnt.changed[k] |= 1;
      ++written;
      filled += hv[k] >= 0;
    }
    if (cnt.runs) ++cnt.runs[s];
    if (cnt.filled) cnt.filled[s] += filled;
    if (filled_all) *filled_all += filled;
  }
  if (!written) return 0;
  if (move_lists(c, q, hx, hipMemcpyHostToDevice, st)) return -1;
  if (q.tab_x) {  // the row carries every list after the replacement
    const size_t nb = sizeof(float) * (size_t)n;
    HIPCHK(c, hipMemcpyAsync(q.tab_x + row * q.tab_stride, q.x, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(q.tab_y + row * q.tab_stride, q.y, nb, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(q.tab_val + row * q.tab_stride, q.val, nb, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}
#pragma GCC visibility pop
