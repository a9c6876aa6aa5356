// runtime_multi.hip -- host side of libklt_amd.so: the batched calls over
// several independent sequences (klt_hip_track_frames_multi,
// klt_hip_track_frames_multi_replace; runtime.h).  No kernels here.
//
// One context, one stream.  The three banks of the plain batched calls are
// laid out for nseq * chunk pyramids each and filled frame-major: pyramid
// j * nseq + s of a bank is frame j of sequence s, so the nseq pyramids a
// chunk starts from -- the previous bank's last group, or for the first chunk
// the start images' group, built into the bank the third chunk reuses -- are
// contiguous and one pointer per level (TrkArgs::A) serves every sequence.
// Per chunk: the pyramids (one pair of launches over nseq * F frames when the
// caller's frames are frame-major too, else one pair per sequence), then one
// k_track7_multi launch over the concatenated lists.  Stream order is the
// only dependency; the banks rotate all the same, so that a chunk never
// overwrites the group it starts from.
//
// With a replacement description the tracker launch alone is cut, for all
// sequences at once, after every frame at which a replacement is due: a
// sub-launch over frames [f0, f1) of a bank starts from the group at f0 - 1.
// At a cut the lists come to the host, the next chunk's pyramids are queued
// before the host waits, the sequences with a lost slot get their maps from
// one k_min_eigen7_multi launch over the adjacent pyramids of that frame, and
// the selection engine fills each one's slots from its own map, one sequence
// after the other.
#include "replace_step.h"

namespace {
// what the multi instances cover: the default configuration
int multi_refused(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td, const char *who) {
  if (c->fb_on) return fail(c, "%s: the forward-backward check is not covered (klt_hip_set_fb)", who);
  if (c->aff_on) return fail(c, "%s: the affine check is not covered (klt_hip_set_frames_affine)", who);
  if (c->pred_on) return fail(c, "%s: the motion prior is not covered (klt_hip_set_predict)", who);
  if (mask_tracks(c)) return fail(c, "%s: the region mask's tracking use is not covered (klt_hip_set_mask)", who);
  if (td->reduction != KLT_HIP_EXACT) return fail(c, "%s: needs KLT_HIP_EXACT sums", who);
  if (td->window_width != 7 || td->window_height != 7)
    return fail(c, "%s: window %dx%d is not covered (7x7 only)", who, td->window_width, td->window_height);
  if (td->lighting_insensitive) return fail(c, "%s: lighting-insensitive mode is not covered", who);
  if (pd->nlevels < 1 || pd->nlevels > KLT_HIP_MAX_LEVELS) return fail(c, "%s: bad nlevels %d", who, pd->nlevels);
  if (!fused_ok(pd) || c->force_generic)
    return fail(c, "%s: needs the fused (default-parameter) pyramid path (klt_hip_fused_path)", who);
  if (!t7_tracks(c, td))
    return fail(c, "%s: needs the default tracker kernel (klt_hip_set_track_impl 0, klt_hip_set_track_patch 1, "
                "no klt_hip_set_prof buffer)", who);
  return 0;
}

// the replacement of klt_hip_track_frames_multi_replace: its description, the
// frames tracked before the call and the caller's host arrays (optional)
struct MultiReplace {
  const klt_hip_replace_desc *d;
  long count0;
  unsigned char *changed;
  long *runs, *filled;
};

// One replacement for every sequence: the frame just tracked is group `group`
// of bank K, whose nseq adjacent pyramids one k_min_eigen7_multi launch reads
// (a description with another window or step: a launch per sequence)
template <class Ahead>
int replace_lost_multi(klt_hip_ctx *c, const RepLists &q, const MultiReplace &r, const Bank &K, long group, long row,
                       Ahead ahead) {
  const Level &L0 = K.lv[0];
  const klt_hip_select_desc &sd = r.d->sel;
  const auto maps = [&](const EigMultiArgs &m, const SelGrid &g) -> long {
    const long np = (long)g.nx * g.ny, lfs = (long)L0.w * L0.h * kRec;
    const float *rec = L0.img + group * q.nseq * lfs;
    hipStream_t st = c->stream;
    TimedScope ts(c, T_EIG, st);
    if (g.hw == kRG && g.hh == kRG && g.step <= 2)
      return launched(c, "k_min_eigen7_multi", launch_min_eigen_multi(st, rec, lfs, m, L0.w, sd.borderx, sd.bordery, g.step,
                                                                      g.nx, g.ny, c->d_rep_map, &c->eig_kernel))
                 ? -1 : np;
    for (int i = 0; i < m.nsel; ++i) {
      const float *f = rec + m.seq[i] * lfs;
      if (launched(c, "k_min_eigen", launch_min_eigen(st, f + kRecGx, f + kRecGy, L0.w, kRec, sd.borderx, sd.bordery, g.step,
                                                      g.nx, g.ny, g.hw, g.hh, c->d_rep_map + i * np, &c->eig_kernel)))
        return -1;
    }
    return np;
  };
  return replace_step(c, q, *r.d, L0.w, L0.h, row, RepCounters{r.changed, r.runs, r.filled}, ahead, maps);
}

// both calls; rep == nullptr: klt_hip_track_frames_multi
int track_multi(klt_hip_ctx *c, const char *who, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                const MultiReplace *rep, const unsigned char *frames, long pitch, long stride, long seq_stride, int nseq,
                int nframes, int chunk, const int *n_seq, float *x, float *y, int *val, float *tab_x, float *tab_y,
                int *tab_val, long tab_stride) {
  if (!c || !pd || !td || !n_seq) return fail(c, "%s: null argument", who);
  if (rep && !rep->d) return fail(c, "%s: null replacement description", who);
  if (c->rep_on)
    return rep ? fail(c, "%s: the context's own replacement setting is on; it belongs to the single-sequence calls "
                      "(klt_hip_set_frames_replace)", who)
               : fail(c, "%s: not covered while lost features are replaced (klt_hip_set_frames_replace)", who);
  if (rep && replace_desc_refused(c, rep->d, who)) return -1;
  if (mask_refused(c, pd->ncols, who)) return -1;
  if (rep && rep->count0 < 0) return fail(c, "%s: count0 %ld < 0", who, rep->count0);
  if (nseq < 1 || nseq > KLT_HIP_MAX_SEQUENCES)
    return fail(c, "%s: nseq %d is not in 1..%d", who, nseq, KLT_HIP_MAX_SEQUENCES);
  if (nframes < 0 || chunk < 1) return fail(c, "%s: bad nframes/chunk", who);
  TrkMultiArgs ms;
  memset(&ms, 0, sizeof ms);
  ms.nseq = nseq;
  long total = 0;
  for (int s = 0; s < nseq; ++s) {
    if (n_seq[s] < 0) return fail(c, "%s: sequence %d has %d features", who, s, n_seq[s]);
    total += n_seq[s];
    if (total > (1L << 30)) return fail(c, "%s: too many features", who);
    ms.first[s + 1] = (int)total;
  }
  for (int s = nseq + 1; s <= kMaxSeq; ++s) ms.first[s] = (int)total;
  const int n = (int)total;
  if (!frames) return fail(c, "%s: null frames", who);
  if (n > 0 && (!x || !y || !val)) return fail(c, "%s: null feature arrays", who);
  if (tables_refused(c, who, tab_x, tab_y, tab_val, tab_stride, n, pitch, pd->ncols)) return -1;
  if (multi_refused(c, pd, td, who)) return -1;
  if (nframes == 0) return 0;
  if (use_device(c)) return -1;

  // the chunk: three banks of nseq * chunk pyramids within the budget
  const int fit = budget_chunk(c, pd) / nseq;
  if (fit < 1)
    return fail(c, "%s: %d %dx%d pyramids per bank exceed the bank budget of %zu bytes", who, nseq, pd->ncols,
                pd->nrows, bank_budget_of(c));
  if (chunk > fit) chunk = fit;
  const int F0 = chunk < nframes ? chunk : nframes;

  // from here on the context has no current pyramid: the banks are this call's
  if (forget_kept(c)) return -1;
  c->chunk_used = chunk;
  if (ensure_banks(c, pd, nseq * chunk)) return -1;  // pyramids per bank

  TrkArgs a;
  fill_trk_args(td, pd->nlevels, pd->nlevels > 1 ? pd->subsampling : 1, pd->ncols, pd->nrows, a);
  a.merge_res = c->track_merge;
  a.prio = c->track_prio;
  a.aos = 1;
  hipStream_t st = c->stream;
  const bool frame_major = stride == (long)nseq * seq_stride;
  const RepLists q{nseq, n, ms.first, x, y, val, tab_x, tab_y, tab_val, tab_stride};

  // a chunk's pyramids: F frames of every sequence from call frame j0 + 1 into bank K
  const auto build = [&](Bank &K, int j0, int F) -> int {
    const unsigned char *src = frames + (long)(j0 + 1) * stride;
    if (frame_major)
      return build_fused_bank(c, K, pd, src, pitch, seq_stride, nseq * F, st, 0, 1 << 30, 0, 1 << 30, kLayoutRec);
    for (int s = 0; s < nseq; ++s)
      if (build_fused_bank(c, K, pd, src + (long)s * seq_stride, pitch, stride, F, st, 0, 1 << 30, 0, 1 << 30,
                           kLayoutRec, s, nseq))
        return -1;
    return 0;
  };

  // the start images' group: pyramids 0 .. nseq-1 of a bank
  int bi = c->banks.take();
  if (build_fused_bank(c, c->banks.bank[bi], pd, frames, pitch, seq_stride, nseq, st, 0, 1 << 30, 0, 1 << 30, kLayoutRec))
    return -1;
  long prev_first = 0;  // the group this chunk starts from: pyramids prev_first .. +nseq of bank bi
  int ahead_bank = -1;  // >= 0: this chunk's pyramids were queued there at the previous chunk's last cut
  for (int j0 = 0; j0 < nframes; j0 += F0) {
    const int F = F0 < nframes - j0 ? F0 : nframes - j0, pb = bi;
    bi = ahead_bank >= 0 ? ahead_bank : c->banks.take();
    Bank &K = c->banks.bank[bi];
    if (ahead_bank < 0 && build(K, j0, F)) return -1;
    ahead_bank = -1;
    const int jn = j0 + F, Fn = F0 < nframes - jn ? F0 : nframes - jn;
    for (int f0 = 0; f0 < F;) {
      // up to the next frame at which a replacement is due
      const int f1 = rep ? next_cut(rep->count0 + j0 + f0, rep->d->every, f0, F) : F;
      TrkFramesArgs b;
      memset(&b, 0, sizeof b);
      for (int l = 0; l < pd->nlevels; ++l) {
        a.A[l] = f0 ? K.level(l, (long)(f0 - 1) * nseq) : c->banks.bank[pb].level(l, prev_first);
        a.B[l] = K.level(l, (long)f0 * nseq);
        b.lfs[l] = (long)K.lv[l].w * K.lv[l].h * 3;
      }
      b.nframes = f1 - f0;
      if (tab_x) {
        b.tx = tab_x + (long)(j0 + f0) * tab_stride;
        b.ty = tab_y + (long)(j0 + f0) * tab_stride;
        b.tv = tab_val + (long)(j0 + f0) * tab_stride;
        b.tstride = tab_stride;
      }
      b.count = c->d_trk_count;
      if (n > 0) {
        TimedScope ts(c, T_TRACK, st, f1 - f0);
        if (launched(c, "k_track7_multi", launch_track7_multi(st, a, b, ms, x, y, val, n, &c->track_kernel))) return -1;
      }
      if (rep && (rep->count0 + j0 + f1) % rep->d->every == 0) {
        const auto ahead = [&]() -> int {
          if (f1 < F || Fn <= 0) return 0;
          ahead_bank = c->banks.take();
          return build(c->banks.bank[ahead_bank], jn, Fn);
        };
        if (replace_lost_multi(c, q, *rep, K, f1 - 1, j0 + f1 - 1, ahead)) return -1;
      }
      f0 = f1;
    }
    prev_first = (long)(F - 1) * nseq;
  }
  return 0;
}
}  // namespace

KLT_API int klt_hip_multi_covers(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td) {
  if (!c || !pd || !td) return fail(c, "multi_covers: null argument");
  if (c->pred_on) return fail(c, "track_frames_multi: the motion prior is not covered (klt_hip_set_predict)");
  if (mask_tracks(c))
    return fail(c, "track_frames_multi: the region mask's tracking use is not covered (klt_hip_set_mask)");
  return multi_refused(c, pd, td, "track_frames_multi") ? 0 : 1;
}

KLT_API int klt_hip_track_frames_multi(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                                       const unsigned char *frames, long pitch, long stride, long seq_stride,
                                       int nseq, int nframes, int chunk, const int *n_seq, float *x, float *y,
                                       int *val, float *tab_x, float *tab_y, int *tab_val, long tab_stride) {
  return track_multi(c, "track_frames_multi", pd, td, nullptr, frames, pitch, stride, seq_stride, nseq, nframes, chunk,
                     n_seq, x, y, val, tab_x, tab_y, tab_val, tab_stride);
}

KLT_API int klt_hip_track_frames_multi_replace(klt_hip_ctx *c, const klt_hip_pyr_desc *pd,
                                               const klt_hip_track_desc *td, const klt_hip_replace_desc *rep,
                                               long count0, const unsigned char *frames, long pitch, long stride,
                                               long seq_stride, int nseq, int nframes, int chunk, const int *n_seq,
                                               float *x, float *y, int *val, float *tab_x, float *tab_y, int *tab_val,
                                               long tab_stride, unsigned char *changed, long *runs, long *filled) {
  const MultiReplace r{rep, count0, changed, runs, filled};
  return track_multi(c, "track_frames_multi_replace", pd, td, &r, frames, pitch, stride, seq_stride, nseq, nframes,
                     chunk, n_seq, x, y, val, tab_x, tab_y, tab_val, tab_stride);
}

KLT_API int klt_hip_min_eigen_records(klt_hip_ctx *c, const float *dev_rec, long frame_stride, const int *which,
                                      int nsel, int ncols, int nrows, const klt_hip_select_desc *d, int *dev_maps) {
  if (!c || !dev_rec || !which || !d || !dev_maps || ncols < 1 || nrows < 1)
    return fail(c, "min_eigen_records: bad argument");
  if (nsel < 1 || nsel > kMaxSeq) return fail(c, "min_eigen_records: nsel %d is not in 1..%d", nsel, kMaxSeq);
  const SelGrid g = sel_grid(*d, ncols, nrows);
  const int step = g.step, nx = g.nx, ny = g.ny;
  if (d->window_width != 2 * kRG + 1 || d->window_height != 2 * kRG + 1)
    return fail(c, "min_eigen_records: window %dx%d, the kernel covers 7x7 only", d->window_width, d->window_height);
  if (step < 1 || step > 2) return fail(c, "min_eigen_records: step %d, the kernel covers 1 and 2", step);
  if (d->borderx < kRG || d->bordery < kRG) return fail(c, "min_eigen_records: border smaller than window half size");
  if (frame_stride < (long)ncols * nrows * kRec) return fail(c, "min_eigen_records: frame stride %ld too small", frame_stride);
  EigMultiArgs m;
  memset(&m, 0, sizeof m);
  m.nsel = nsel;
  for (int i = 0; i < nsel; ++i) {
    if (which[i] < 0) return fail(c, "min_eigen_records: frame index %d", which[i]);
    m.seq[i] = which[i];
  }
  if ((long)nx * ny == 0) return 0;
  if (use_device(c)) return -1;
  {
    TimedScope ts(c, T_EIG, c->stream);
    if (launched(c, "k_min_eigen7_multi", launch_min_eigen_multi(c->stream, dev_rec, frame_stride, m, ncols, d->borderx,
                                                                 d->bordery, step, nx, ny, dev_maps, &c->eig_kernel)))
      return -1;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
