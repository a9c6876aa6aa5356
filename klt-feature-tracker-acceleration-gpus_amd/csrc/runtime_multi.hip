// runtime_multi.hip -- host side of libklt_amd.so: the batched call over
// several independent sequences (klt_hip_track_frames_multi; runtime.h).  No
// kernels here.
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
#include "runtime.h"

namespace {
// what the multi instances cover: the default configuration
int multi_refused(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td) {
  const char *who = "track_frames_multi";
  if (c->fb_on) return fail(c, "%s: the forward-backward check is not covered (klt_hip_set_fb)", who);
  if (c->aff_on) return fail(c, "%s: the affine check is not covered (klt_hip_set_frames_affine)", who);
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
}  // namespace

KLT_API int klt_hip_multi_covers(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td) {
  if (!c || !pd || !td) return fail(c, "multi_covers: null argument");
  return multi_refused(c, pd, td) ? 0 : 1;
}

KLT_API int klt_hip_track_frames_multi(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                                       const unsigned char *frames, long pitch, long stride, long seq_stride,
                                       int nseq, int nframes, int chunk, const int *n_seq, float *x, float *y,
                                       int *val, float *tab_x, float *tab_y, int *tab_val, long tab_stride) {
  const char *who = "track_frames_multi";
  if (!c || !pd || !td || !n_seq) return fail(c, "%s: null argument", who);
  if (c->rep_on) return fail(c, "%s: not covered while lost features are replaced (klt_hip_set_frames_replace)", who);
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
  const int ntab = (tab_x != nullptr) + (tab_y != nullptr) + (tab_val != nullptr);
  if (ntab != 0 && ntab != 3) return fail(c, "%s: give all three table arrays or none", who);
  if (ntab && tab_stride < n) return fail(c, "%s: table stride %ld < n %d", who, tab_stride, n);
  if (pitch < (long)pd->ncols * frame_bpp(c->frame_format))
    return fail(c, "%s: pitch %ld < ncols %d * %d bytes per pixel", who, pitch, pd->ncols, frame_bpp(c->frame_format));
  if (multi_refused(c, pd, td)) return -1;
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
  c->frames_ready = false;
  c->prev = PrevRef{};
  if (c->pstream && c->pre.bank >= 0) HIPCHK(c, hipStreamSynchronize(c->pstream));  // a band call's build-ahead
  c->pre.bank = -1;
  c->chunk_used = chunk;
  const int P = nseq * chunk;  // pyramids per bank
  if (!(bank_fits(c->bank[0], pd, P) && bank_fits(c->bank[1], pd, P) && bank_fits(c->bank[2], pd, P))) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->pstream) HIPCHK(c, hipStreamSynchronize(c->pstream));
    if (ensure_banks(c, pd, P)) return -1;
  }

  TrkArgs a;
  fill_trk_args(td, pd->nlevels, pd->nlevels > 1 ? pd->subsampling : 1, pd->ncols, pd->nrows, a);
  a.merge_res = c->track_merge;
  a.prio = c->track_prio;
  a.aos = 1;
  hipStream_t st = c->stream;
  const bool frame_major = stride == (long)nseq * seq_stride;

  // the start images' group: pyramids 0 .. nseq-1 of a bank
  int bi = c->bank_next;
  if (build_fused_bank(c, c->bank[bi], pd, frames, pitch, seq_stride, nseq, st, 0, 1 << 30, 0, 1 << 30, kLayoutRec))
    return -1;
  long prev_first = 0;  // the group this chunk starts from: pyramids prev_first .. +nseq of bank bi
  for (int j0 = 0; j0 < nframes; j0 += F0) {
    const int F = F0 < nframes - j0 ? F0 : nframes - j0, pb = bi;
    bi = (bi + 1) % 3;
    Bank &K = c->bank[bi];
    const unsigned char *src = frames + (long)(j0 + 1) * stride;
    if (frame_major) {
      if (build_fused_bank(c, K, pd, src, pitch, seq_stride, nseq * F, st, 0, 1 << 30, 0, 1 << 30, kLayoutRec))
        return -1;
    } else {
      for (int s = 0; s < nseq; ++s)
        if (build_fused_bank(c, K, pd, src + (long)s * seq_stride, pitch, stride, F, st, 0, 1 << 30, 0, 1 << 30,
                             kLayoutRec, s, nseq))
          return -1;
    }
    TrkFramesArgs b;
    memset(&b, 0, sizeof b);
    for (int l = 0; l < pd->nlevels; ++l) {
      a.A[l] = level_view(c->bank[pb].lv[l], prev_first);
      a.B[l] = level_view(K.lv[l], 0);
      b.lfs[l] = (long)K.lv[l].w * K.lv[l].h * 3;
    }
    b.nframes = F;
    if (tab_x) {
      b.tx = tab_x + (long)j0 * tab_stride;
      b.ty = tab_y + (long)j0 * tab_stride;
      b.tv = tab_val + (long)j0 * tab_stride;
      b.tstride = tab_stride;
    }
    b.count = c->d_trk_count;
    if (n > 0) {
      TimedScope ts(c, T_TRACK, st, F);
      if (launched(c, "k_track7_multi", launch_track7_multi(st, a, b, ms, x, y, val, n, &c->track_kernel))) return -1;
    }
    prev_first = (long)(F - 1) * nseq;
  }
  c->bank_next = (bi + 1) % 3;
  return 0;
}
