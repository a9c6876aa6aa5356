// runtime_track.hip -- host side of libklt_amd.so: the tracker launch, the
// per-call tracking and affine entry points and the pipelined sequence, over
// track.hip / track7.hip / affine.hip (runtime.h).  No kernels here.
#include "runtime.h"

int check_window(klt_hip_ctx *c, const klt_hip_track_desc *d) {
  const int npx = d->window_width * d->window_height;
  if (d->window_width < 1 || d->window_height < 1 || npx > 16 * kWave)
    return fail(c, "track: window %dx%d unsupported (max %d pixels)", d->window_width, d->window_height,
                16 * kWave);
  return 0;
}

void fill_trk_args(const klt_hip_track_desc *d, int nlev, int ss, int ncols, int nrows, TrkArgs &a) {
  memset(&a, 0, sizeof a);
  const int npx = d->window_width * d->window_height;
  a.nlev = nlev;
  a.ss = (float)ss;
  a.ss_inv = ss > 0 && (ss & (ss - 1)) == 0 ? 1.0f / (float)ss : 0.0f;
  a.ww = d->window_width;
  a.wh = d->window_height;
  a.max_it = d->max_iterations;
  a.min_det = d->min_determinant;
  a.min_disp = d->min_displacement;
  a.max_res = d->max_residue;
  a.step = d->step_factor;
  a.borderx = d->borderx;
  a.bordery = d->bordery;
  a.ncols = ncols;
  a.nrows = nrows;
  a.li = d->lighting_insensitive;
  int rp = (npx + 3) & ~3;  // 16-byte rows with an odd slot count: distinct banks per sum
  if (((rp / 4) & 1) == 0) rp += 4;
  a.red_pitch = rp;
}

namespace {
// fewer features than this: input order (the sort launch would not pay)
constexpr int kOrderMin = 2048;
// the processing order (a locality hint: any permutation gives the same
// results) is re-sorted once it covers this many tracked frames; features
// move about a pixel per frame, the XCDs' row bands are ~H/8 rows tall
constexpr int kOrderMaxAge = 32;

// KLT_ORDER_BALANCE=0 in the environment (A/B in one tree, read once): the
// order keeps the lost features last instead of spreading them over the XCDs
bool order_balanced() {
  static const bool on = [] {
    const char *v = getenv("KLT_ORDER_BALANCE");
    return !(v && *v && atoi(v) == 0);
  }();
  return on;
}

// slots per XCD of a tracker launch over n features in XCD-major order
// (TrkFramesArgs::xcd_per workgroups of kBlock / kWave waves)
int order_xcd_per(int n) {
  const int per = kBlock / kWave, nb = (n + per - 1) / per;
  return (nb + 7) / 8;
}
}  // namespace

KLT_API int klt_hip_order_slot(int n, int xcd_per, int n_live, int rank, int lost, int *slot) {
  if (n < 1 || xcd_per < 1 || n_live < 0 || n_live > n || rank < 0 || !slot) return -1;
  const long seg = (long)xcd_per * (kBlock / kWave);
  if (seg * kXcds < n || seg > INT32_MAX / kXcds) return -1;  // the eight segments hold every slot
  if (rank >= (lost ? n - n_live : n_live)) return -1;
  int live_st[kXcds + 1], lost_st[kXcds + 1];
  for (int x = 0; x <= kXcds; ++x) {
    live_st[x] = order_live_start(n, (int)seg, n_live, x);
    lost_st[x] = order_lost_start(n, (int)seg, n_live, x);
  }
  *slot = order_slot_of(live_st, lost_st, (int)seg, rank, lost != 0);
  return 0;
}

KLT_API int klt_hip_band_order_probe(klt_hip_ctx *c, const float *y, const int *v, int n, int nrows, int *perm_out) {
  if (!c) return fail(c, "band_order_probe: null context");
  if (n < 1 || !y || !v || !perm_out) return fail(c, "band_order_probe: n %d, or a null array", n);
  if (use_device(c)) return -1;
  int *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, sizeof(int) * (size_t)n));
  const int seg = order_balanced() ? order_xcd_per(n) * (kBlock / kWave) : 0;
  hipError_t e = hipMemsetAsync(d, 0xFF, sizeof(int) * (size_t)n, c->stream);  // a slot left unwritten reads -1
  if (e == hipSuccess) e = launch_band_order(c->stream, y, v, n, nrows, d, 0.0f, 0.0f, nullptr, seg);
  if (e == hipSuccess) e = hipMemcpyAsync(perm_out, d, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(c, "band_order_probe: %s", hipGetErrorString(e));
  return 0;
}

// the default configuration's latency-lean tracker (track7.hip) serves this
// launch: 7x7 window, exact sums, no gain/bias, the lane-patch path on, and
// the generic kernel not forced (klt_hip_set_track_impl, A/B only)
bool t7_tracks(const klt_hip_ctx *c, const klt_hip_track_desc *d) {
#ifdef KLT_TRACK_PROF
  const bool prof_ok = true;  // the instrumented build instruments both kernels
#else
  const bool prof_ok = !c->prof;
#endif
  const bool li = d->lighting_insensitive != 0;
  const bool win7 = d->window_width == 7 && d->window_height == 7;
  return c->track_impl == 0 && win7 && !li && c->track_patch && prof_ok;  // exact or fast sums
}

// The processing order of a tracker launch over n features (k_band_order on
// st, reading y/v as they stand in st's order): bb.perm / xcd_per / n_dev.
// own != nullptr (band mode): only live features with own[0] <= y < own[1].
// The batched path queues it before the tracking stream waits for the chunk's
// pyramids, so the sort runs while they are built.
int order_features(klt_hip_ctx *c, hipStream_t st, int nrows, const float *y, const int *v, int n, int nframes,
                   const float *own, TrkFramesArgs &bb) {
  if (own || (c->track_order == 0 && n >= kOrderMin)) {
    // a launch reuses the order of a recent one with the same feature count
    // while that order covers at most kOrderMaxAge frames in all: any
    // permutation gives the same results, and features move little from one
    // frame to the next (per-call KLTTrackFeatures and short batched calls
    // then skip the sort; 64-frame chunks re-sort every launch)
    const bool reuse = !own && c->perm_n == n && c->perm_age + nframes <= kOrderMaxAge;
    if (reuse) {
      c->perm_age += nframes;
    } else {
      if (grow(c, &c->d_perm, &c->perm_cap, (size_t)n)) return -1;
      if (own && !c->d_count) HIPCHK(c, hipMalloc((void **)&c->d_count, sizeof(int)));
#ifdef KLT_HOST_PROF
      timespec t0_, t1_;
      clock_gettime(CLOCK_MONOTONIC, &t0_);
#endif
      const int seg = !own && order_balanced() ? order_xcd_per(n) * (kBlock / kWave) : 0;
      if (launched(c, "k_band_order", launch_band_order(st, y, v, n, nrows, c->d_perm, own ? own[0] : 0.0f,
                                                        own ? own[1] : 0.0f, own ? c->d_count : (int *)nullptr, seg)))
        return -1;
#ifdef KLT_HOST_PROF
      clock_gettime(CLOCK_MONOTONIC, &t1_);
      fprintf(stderr, "hostmark band_order_launch %.2f us\n",
              (t1_.tv_sec - t0_.tv_sec) * 1e6 + (t1_.tv_nsec - t0_.tv_nsec) * 1e-3);
#endif
      c->perm_n = own ? -1 : n;  // a band's order lists only the band's features
      c->perm_age = nframes;
    }
    if (own) bb.n_dev = c->d_count;
    bb.perm = c->d_perm;
    bb.xcd_per = order_xcd_per(n);
  }
  return 0;
}

// The forward-backward check (klt_hip_set_fb) has instances for exact sums on
// whole-frame pyramids only: anything else fails before a launch.
int fb_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, const char *who) {
  if (!c->fb_on) return 0;
  if (band) return fail(c, "%s: the forward-backward check does not cover band calls (klt_hip_set_fb)", who);
  if (d->reduction != KLT_HIP_EXACT)
    return fail(c, "%s: the forward-backward check needs KLT_HIP_EXACT sums (klt_hip_set_fb)", who);
  return 0;
}

// The affine check inside the launch (klt_hip_set_frames_affine) has instances
// for exact sums on whole-frame pyramids, without the forward-backward check;
// its window store must hold n features' windows of this size and its tables
// n features per row: anything else fails before a launch.
int aff_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, int n, const char *who) {
  if (!c->aff_on) return 0;
  if (band) return fail(c, "%s: the affine check does not cover band calls (klt_hip_set_frames_affine)", who);
  if (d->reduction != KLT_HIP_EXACT)
    return fail(c, "%s: the affine check needs KLT_HIP_EXACT sums (klt_hip_set_frames_affine)", who);
  if (c->fb_on)
    return fail(c, "%s: the forward-backward check does not combine with the affine check "
                "(klt_hip_set_fb, klt_hip_set_frames_affine)", who);
  const int S = (c->aff_p.ww + 2) * (c->aff_p.wh + 2);
  if (n > 0 && (!c->d_aff_store || c->aff_S != S || c->aff_store_cap < (size_t)n * 3 * S))
    return fail(c, "%s: affine window store not reserved for %d features of %dx%d (klt_hip_affine_reserve)", who, n,
                c->aff_p.ww, c->aff_p.wh);
  if ((c->aff_tab || c->aff_stab) && c->aff_tab_stride < n)
    return fail(c, "%s: affine table stride %ld < n %d", who, c->aff_tab_stride, n);
  return 0;
}

// The motion prior (klt_hip_set_predict) has instances of k_track7 for exact
// sums on whole-frame pyramids, without either check: anything else fails
// before a launch.
int pred_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, const char *who) {
  if (!c->pred_on) return 0;
  if (band) return fail(c, "%s: the motion prior does not cover band calls (klt_hip_set_predict)", who);
  if (d->reduction != KLT_HIP_EXACT)
    return fail(c, "%s: the motion prior needs KLT_HIP_EXACT sums (klt_hip_set_predict)", who);
  if (c->fb_on)
    return fail(c, "%s: the forward-backward check does not combine with the motion prior "
                "(klt_hip_set_fb, klt_hip_set_predict)", who);
  if (c->aff_on)
    return fail(c, "%s: the affine check does not combine with the motion prior "
                "(klt_hip_set_frames_affine, klt_hip_set_predict)", who);
  if (!t7_tracks(c, d))
    return fail(c, "%s: the motion prior needs the default tracker kernel: a 7x7 window without lighting-insensitive "
                "mode (klt_hip_set_predict; klt_hip_set_track_impl 0, klt_hip_set_track_patch 1, no klt_hip_set_prof "
                "buffer)", who);
  return 0;
}

// The region mask's tracking use (klt_hip_set_mask, KLT_HIP_MASK_TRACK) has
// instances of k_track7 for exact sums on whole-frame pyramids, without either
// check or the motion prior: anything else fails before a launch.  The
// selection use alone refuses nothing.
int mask_track_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, const char *who) {
  if (!mask_tracks(c)) return 0;
  if (band) return fail(c, "%s: the region mask's tracking use does not cover band calls (klt_hip_set_mask)", who);
  if (d->reduction != KLT_HIP_EXACT)
    return fail(c, "%s: the region mask's tracking use needs KLT_HIP_EXACT sums (klt_hip_set_mask)", who);
  if (c->fb_on)
    return fail(c, "%s: the forward-backward check does not combine with the region mask's tracking use "
                "(klt_hip_set_fb, klt_hip_set_mask)", who);
  if (c->aff_on)
    return fail(c, "%s: the affine check does not combine with the region mask's tracking use "
                "(klt_hip_set_frames_affine, klt_hip_set_mask)", who);
  if (c->pred_on)
    return fail(c, "%s: the motion prior does not combine with the region mask's tracking use "
                "(klt_hip_set_predict, klt_hip_set_mask)", who);
  if (!t7_tracks(c, d))
    return fail(c, "%s: the region mask's tracking use needs the default tracker kernel: a 7x7 window without "
                "lighting-insensitive mode (klt_hip_set_mask; klt_hip_set_track_impl 0, klt_hip_set_track_patch 1, no "
                "klt_hip_set_prof buffer)", who);
  return 0;
}

// all of the above, and the tables' rows hold n features:
// what a tracker launch of n features in the name of `who` refuses.  An entry
// point that hands its work to another one asks the two above alone and
// leaves the table to the launch underneath, in that one's name
int track_refused(klt_hip_ctx *c, const klt_hip_track_desc *d, bool band, int n, const char *who) {
  if (mask_track_refused(c, d, band, who)) return -1;
  if (pred_refused(c, d, band, who) || fb_refused(c, d, band, who) || aff_refused(c, d, band, n, who)) return -1;
  if (c->fb_on && c->fb_tab && c->fb_stride < n)
    return fail(c, "%s: forward-backward table stride %ld < n %d", who, c->fb_stride, n);
  if (c->pred_on && c->pred_tvx && c->pred_stride < n)
    return fail(c, "%s: motion prior table stride %ld < n %d", who, c->pred_stride, n);
  return 0;
}

int track_frames_launch(klt_hip_ctx *c, hipStream_t st, const klt_hip_track_desc *d, const TrkArgs &a,
                        const TrkFramesArgs &b, float *x, float *y, int *v, int n, const float *own, bool ordered,
                        long fb_row, TailRelease *tail) {
  if (tail) tail->wait = false;
  if (track_refused(c, d, own != nullptr || a.escape != nullptr, n, "track")) return -1;
  if (mask_tracks(c) && mask_refused(c, a.ncols, "track")) return -1;
  TimedScope ts(c, T_TRACK, st, b.nframes);
  const int npx = d->window_width * d->window_height;
  const bool exact = d->reduction == KLT_HIP_EXACT, li = d->lighting_insensitive != 0;
  const bool patch = c->track_patch && (d->window_width + 1) * (d->window_height + 1) <= kWave;
  // the default 7x7 window gets compile-time window geometry (unrolled ordered sums)
  const bool win7 = d->window_width == 7 && d->window_height == 7;
  TrkFramesArgs bb = b;
  if (!ordered && order_features(c, st, a.nrows, y, v, n, b.nframes, own, bb)) return -1;
  bb.prof = c->prof;
  bb.count = c->d_trk_count;
  const TrkFramesArgs &b2 = bb;
  TrkArgs aa = a;
  aa.merge_res = c->track_merge;
  aa.prio = c->track_prio;
  aa.aos = 0;
  aa.fast = 0;
  // k_track7 reads interleaved levels as built; other kernels (or a mix of
  // layouts) get planes of the interleaved ones.  Its fast-sum instance
  // covers interleaved two-level pyramids; other fast cases take the generic
  // kernel's tree sums
  const bool ilA = a.A[0].il != 0, ilB = a.B[0].il != 0;
  // the affine check runs in the generic family only (a 15x15 affine window
  // costs far more than the lean kernel saves on the 7x7 translation step)
  const bool t7 = !c->aff_on && t7_tracks(c, d) && (exact || (ilA && ilB && a.nlev == 2));
  if (t7 && ilA && ilB) {
    aa.aos = 1;
    aa.fast = exact ? 0 : 1;
  } else if (ilA || ilB) {
    for (int l = 0; l < a.nlev; ++l) {
      for (int k = 0; k < 2; ++k) {
        TrkLevel &L = k == 0 ? aa.A[l] : aa.B[l];
        if (!L.il) continue;
        const long np = (long)L.w * L.h, F = k == 0 ? 1 : bb.nframes;
        if (grow(c, &c->pl_scr[k][l], &c->pl_cap[k][l], (size_t)(3 * np * F))) return -1;
        float *p = c->pl_scr[k][l];
        if (launched(c, "k_from_il", launch_from_il(st, L.img, p, p + np * F, p + 2 * np * F, np * F))) return -1;
        L = TrkLevel{p, p + np * F, p + 2 * np * F, L.w, L.h, L.vlo, L.vhi, 0};
        if (k == 1) bb.lfs[l] = np;
      }
    }
  }
  HMARK_IN("track_args");
  TrkFbArgs fb{};
  if (c->fb_on) {
    const volatile float t2 = c->fb_dist * c->fb_dist;  // one float product
    fb.t2 = t2;
    fb.err = c->fb_tab ? c->fb_tab + fb_row * c->fb_stride : nullptr;
    fb.stride = c->fb_stride;
  }
  const TrkFbArgs *fbp = c->fb_on ? &fb : nullptr;
  TrkPredArgs pr{};
  if (c->pred_on) {  // track_refused: t7, exact sums
    pr.vx = c->pred_vx;
    pr.vy = c->pred_vy;
    pr.tvx = c->pred_tvx ? c->pred_tvx + fb_row * c->pred_stride : nullptr;
    pr.tvy = c->pred_tvy ? c->pred_tvy + fb_row * c->pred_stride : nullptr;
    pr.tstride = c->pred_stride;
  }
  const TrkPredArgs *prp = c->pred_on ? &pr : nullptr;
  const TrkMaskArgs mk{c->mask, c->mask_pitch};  // track_refused: t7, exact sums, whole frames
  const TrkMaskArgs *mkp = mask_tracks(c) ? &mk : nullptr;
  if (t7) {
    // the lazy-gradient instances have twins that count and take times
    if (aa.lazy && aa.aos) bb.wave_t = c->wave_t;
    if (tail && aa.lazy && aa.aos && c->d_exits && !bb.n_dev) {
      const int per = kBlock / kWave, nb = (n + per - 1) / per;
      const unsigned waves = (unsigned)(bb.xcd_per > 0 ? 8 * bb.xcd_per : nb) * per;  // launch_track7's grid
      tail->wait = klt_hip_tail_threshold(c->exits_base, waves, tail->left, &tail->thr) != 0;
      if (tail->wait) {  // a launch of no more than `left` waves does not count at all
        bb.exits = c->d_exits;
        bb.exit_sig = c->d_exit_sig;
        bb.exit_thr = tail->thr;
        c->exits_base += waves;
      }
    }
    const int rc =
        launched(c, "k_track7", launch_track7(st, aa.escape != nullptr, aa, b2, x, y, v, n, &c->track_kernel, fbp, prp,
                                                  mkp));
    if (rc && tail && tail->wait) {  // counted on the host, maybe not on the device: no wait, and re-base next time
      tail->wait = false;
      c->exits_base = kExitsRebase + 1;
    }
    return rc;
  }
  TrkAffArgs af{};
  if (c->aff_on) {
    af.p = c->aff_p;
    af.aff = c->aff_dev;
    af.state = c->aff_state_dev;
    af.store = c->d_aff_store;
    af.fresh = c->aff_fresh;
    af.lds_wave = (int)(track_affine_lds_bytes(af.p.mode) / sizeof(float) / (kBlock / kWave));
    af.stride = c->aff_tab_stride;
    af.tab_aff = c->aff_tab ? c->aff_tab + 6 * fb_row * af.stride : nullptr;
    af.tab_state = c->aff_stab ? c->aff_stab + fb_row * af.stride : nullptr;
    c->aff_fresh = 0;
  }
  const TrkAffArgs *afp = c->aff_on ? &af : nullptr;
  c->track_kernel = afp ? "kltdev::k_track_frames_g_aff" : fbp ? "kltdev::k_track_frames_g_fb" : "kltdev::k_track_frames_g";
  return launched(c, "k_track_frames",
                  launch_track_frames(st, exact, li, patch, win7, npx, aa, b2, x, y, v, n, fbp, afp));
}

// klt_hip_track_affine's and klt_hip_set_frames_affine's argument checks
static int affine_desc_check(klt_hip_ctx *c, const klt_hip_affine_desc *ad, const char *who) {
  if (ad->mode < 0 || ad->mode > 2) return fail(c, "%s: mode %d (0, 1 or 2)", who, ad->mode);
  if (ad->window_width < 3 || ad->window_height < 3 || ad->window_width % 2 == 0 || ad->window_height % 2 == 0)
    return fail(c, "%s: affine window %dx%d must be odd and >= 3", who, ad->window_width, ad->window_height);
  return 0;
}

static AffParams affine_params(const klt_hip_affine_desc *ad) {
  AffParams p;
  p.mode = ad->mode;
  p.ww = ad->window_width;
  p.wh = ad->window_height;
  p.max_it = ad->max_iterations;
  p.li = ad->lighting_insensitive;
  p.min_det = ad->min_determinant;
  p.th = ad->min_displacement;
  p.th_aff = ad->affine_min_displacement;
  p.max_res = ad->max_residue;
  p.mdd = ad->max_displacement_differ;
  p.step = ad->step_factor;
  return p;
}

KLT_API int klt_hip_set_frames_affine(klt_hip_ctx *c, const klt_hip_affine_desc *ad, float *dev_aff,
                                      int *dev_state) {
  if (!c) return fail(c, "set_frames_affine: null context");
  if (ad) {
    if (!dev_aff || !dev_state) return fail(c, "set_frames_affine: null device array");
    if (affine_desc_check(c, ad, "set_frames_affine")) return -1;
    c->aff_p = affine_params(ad);
  }
  c->aff_on = ad ? 1 : 0;
  c->aff_dev = ad ? dev_aff : nullptr;
  c->aff_state_dev = ad ? dev_state : nullptr;
  return 0;
}

KLT_API int klt_hip_get_frames_affine(klt_hip_ctx *c, int *on) {
  if (!c) return fail(c, "get_frames_affine: null context");
  if (on) *on = c->aff_on;
  return 0;
}

KLT_API int klt_hip_set_affine_table(klt_hip_ctx *c, float *dev_aff_tab, int *dev_state_tab, long stride) {
  if (!c) return fail(c, "set_affine_table: null context");
  if ((dev_aff_tab || dev_state_tab) && stride < 1) return fail(c, "set_affine_table: stride %ld < 1", stride);
  c->aff_tab = dev_aff_tab;
  c->aff_stab = dev_state_tab;
  c->aff_tab_stride = dev_aff_tab || dev_state_tab ? stride : 0;
  return 0;
}

KLT_API int klt_hip_affine_state_put(klt_hip_ctx *c, const float *aff, const int *state, int n, float **dev_aff,
                                     int **dev_state) {
  if (!c || !dev_aff || !dev_state || n < 0 || (n > 0 && (!aff || !state)))
    return fail(c, "affine_state_put: bad argument");
  if (use_device(c)) return -1;
  if (grow(c, &c->d_aff, &c->aff_cap, (size_t)(n ? n : 1) * 6) ||
      grow(c, &c->d_astate, &c->astate_cap, (size_t)(n ? n : 1)))
    return -1;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(c->d_aff, aff, sizeof(float) * n * 6, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_astate, state, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's arrays are pageable: read by now
  }
  *dev_aff = c->d_aff;
  *dev_state = c->d_astate;
  return 0;
}

KLT_API int klt_hip_affine_state_get(klt_hip_ctx *c, float *aff, int *state, int n) {
  if (!c || n < 0 || (n > 0 && (!aff || !state))) return fail(c, "affine_state_get: bad argument");
  if (n == 0) return 0;
  if (!c->d_aff || !c->d_astate || c->aff_cap < (size_t)n * 6 || c->astate_cap < (size_t)n)
    return fail(c, "affine_state_get: no arrays of %d features (klt_hip_affine_state_put)", n);
  if (use_device(c)) return -1;
  HIPCHK(c, hipMemcpyAsync(aff, c->d_aff, sizeof(float) * n * 6, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(state, c->d_astate, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// A host feature list packed into the context's pinned block h_feat
// (x | y | val).  The kernels of the per-call path read and write it in place
// (pinned host memory is mapped into the device's address space): no copy
// engine, no copy-to-kernel handoff.  The previous call is complete (every
// host-list call ends with a stream synchronize).
int feat_pack(klt_hip_ctx *c, const float *x, const float *y, const int *val, int n) {
  if (n <= 0) return 0;
  if ((size_t)n > c->f_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(c->d_feat);
    if (c->h_feat) hipHostFree(c->h_feat);
    c->d_feat = c->h_feat = nullptr;
    c->d_fx = c->d_fy = nullptr;
    c->d_fv = nullptr;
    c->f_cap = 0;
    HIPCHK(c, hipMalloc((void **)&c->d_feat, 3 * sizeof(float) * n));
    HIPCHK(c, hipHostMalloc((void **)&c->h_feat, 3 * sizeof(float) * n, hipHostMallocDefault));
    c->f_cap = (size_t)n;
  }
  c->d_fx = c->d_feat;
  c->d_fy = c->d_feat + n;
  c->d_fv = reinterpret_cast<int *>(c->d_feat + 2 * (size_t)n);
  memcpy(c->h_feat, x, sizeof(float) * n);
  memcpy(c->h_feat + n, y, sizeof(float) * n);
  memcpy(c->h_feat + 2 * (size_t)n, val, sizeof(int) * n);
  return 0;
}

// ... or copied into the device block (d_fx | d_fy | d_fv) in one H2D copy
int feat_stage_in(klt_hip_ctx *c, const float *x, const float *y, const int *val, int n) {
  if (n <= 0) return 0;
  if (feat_pack(c, x, y, val, n)) return -1;
  HIPCHK(c, hipMemcpyAsync(c->d_feat, c->h_feat, 3 * sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
  return 0;
}

// the pinned block back into the host list once the stream is done with it
// feat_unpack blocks in hipStreamSynchronize.  Polling instead was measured
// slower on the registered call (tools/exp/r06_upload_pipe_ab.sh): polling
// hipEventQuery 112-124 against 103-105 us, polling a pinned word written by
// hipStreamWriteValue32 109-123 us -- a stream command costs ~10 us here.
int feat_unpack(klt_hip_ctx *c, float *x, float *y, int *val, int n) {
  if (n <= 0) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(x, c->h_feat, sizeof(float) * n);
  memcpy(y, c->h_feat + n, sizeof(float) * n);
  memcpy(val, c->h_feat + 2 * (size_t)n, sizeof(int) * n);
  return 0;
}

KLT_API int klt_hip_track(klt_hip_ctx *c, int s1, int s2, const klt_hip_track_desc *d, float *x, float *y,
                          int *val, int n, int on_device) {
  if (!c || !d) return fail(c, "track: null argument");
  if (s1 < 0 || s1 >= KLT_HIP_MAX_SLOTS || s2 < 0 || s2 >= KLT_HIP_MAX_SLOTS) return fail(c, "track: bad slot");
  const Slot &A = c->slot[s1], &B = c->slot[s2];
  if (A.nlev < 1 || A.nlev != B.nlev) return fail(c, "track: slots not built / level mismatch");
  for (int l = 0; l < A.nlev; ++l)
    if (A.lv[l].w != B.lv[l].w || A.lv[l].h != B.lv[l].h) return fail(c, "track: slot size mismatch");
  if (check_window(c, d)) return -1;
  if (mask_track_refused(c, d, false, "track") || mask_refused(c, A.lv[0].w, "track")) return -1;
  if (mask_tracks(c) && !on_device)
    return fail(c, "track: the region mask's tracking use takes device arrays (on_device = 1; klt_hip_set_mask)");
  if (pred_refused(c, d, false, "track") || fb_refused(c, d, false, "track")) return -1;
  if (c->pred_on && !on_device)
    return fail(c, "track: the motion prior takes device arrays (on_device = 1; klt_hip_set_predict)");
  if (c->pred_on && c->pred_tvx && c->pred_stride < n)
    return fail(c, "track: motion prior table stride %ld < n %d", c->pred_stride, n);
  if (c->aff_on && !on_device)
    return fail(c, "track: the affine check inside the launch takes device arrays (on_device = 1; "
                "klt_hip_set_frames_affine)");
  if (aff_refused(c, d, false, n, "track")) return -1;
  AffCall aff_call(c);
  const int npx = d->window_width * d->window_height;
  if (n <= 0) return 0;
  if (use_device(c)) return -1;
  TrkArgs a;
  fill_trk_args(d, A.nlev, A.ss, A.lv[0].w, A.lv[0].h, a);
  for (int l = 0; l < A.nlev; ++l) {
    a.A[l] = level_view(A.lv[l]);
    a.B[l] = level_view(B.lv[l]);
  }

  float *x_d = x, *y_d = y;
  int *v_d = val;
  const bool kstage = !on_device && c->feat_mode == 2;
  if (kstage) {
    // the pinned block to the device block by a copy kernel (no copy engine)
    if (feat_pack(c, x, y, val, n)) return -1;
    if (launched(c, "k_copy_words", launch_copy_words(c->stream, c->h_feat, c->d_feat, 3L * n))) return -1;
    x_d = c->d_fx;
    y_d = c->d_fy;
    v_d = c->d_fv;
  } else if (!on_device) {
    if (c->feat_mode == 1) {
      if (feat_pack(c, x, y, val, n)) return -1;
      x_d = c->h_feat;
      y_d = c->h_feat + n;
      v_d = reinterpret_cast<int *>(c->h_feat + 2 * (size_t)n);
    } else {
      if (feat_stage_in(c, x, y, val, n)) return -1;
      x_d = c->d_fx;
      y_d = c->d_fy;
      v_d = c->d_fv;
    }
  }
  {
    // one frame through the batched kernels: frame 0 tracks a.A -> a.B, no table
    TrkFramesArgs b;
    memset(&b, 0, sizeof b);
    b.nframes = 1;
    if (track_frames_launch(c, c->stream, d, a, b, x_d, y_d, v_d, n)) return -1;
  }
  if (kstage) {
    if (launched(c, "k_copy_words", launch_copy_words(c->stream, c->d_feat, c->h_feat, 3L * n))) return -1;
    return feat_unpack(c, x, y, val, n);
  }
  if (!on_device) {
    if (c->feat_mode == 0)
      HIPCHK(c, hipMemcpyAsync(c->h_feat, c->d_feat, 3 * sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    return feat_unpack(c, x, y, val, n);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// affine consistency check (include/klt_hip.h)
// ---------------------------------------------------------------------------
KLT_API int klt_hip_affine_reserve(klt_hip_ctx *c, int n, int ww, int wh) {
  if (!c) return fail(c, "affine_reserve: null context");
  if (n < 0 || ww < 1 || wh < 1) return fail(c, "affine_reserve: bad size");
  if (use_device(c)) return -1;
  const int S = (ww + 2) * (wh + 2);
  const size_t need = (size_t)(n ? n : 1) * 3 * S;
  if (c->d_aff_store && c->aff_S == S && c->aff_store_cap >= need) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  hipFree(c->d_aff_store);
  c->d_aff_store = nullptr;
  c->aff_store_cap = 0;
  HIPCHK(c, hipMalloc((void **)&c->d_aff_store, sizeof(float) * need));
  c->aff_store_cap = need;
  c->aff_S = S;
  return 1;
}

static int affine_move(klt_hip_ctx *c, int dir, const int *idx, int m, float *win) {
  if (!c || (m > 0 && (!idx || !win))) return fail(c, "affine windows: null argument");
  if (m <= 0) return 0;
  if (!c->d_aff_store) return fail(c, "affine windows: no store (klt_hip_affine_reserve)");
  const int s3 = 3 * c->aff_S;
  const size_t cap_feat = c->aff_store_cap / s3;
  for (int j = 0; j < m; ++j)
    if (idx[j] < 0 || (size_t)idx[j] >= cap_feat) return fail(c, "affine windows: index %d out of range", idx[j]);
  if (use_device(c)) return -1;
  if (grow(c, &c->d_astage, &c->astage_cap, (size_t)m * s3) || grow(c, &c->d_aidx, &c->aidx_cap, (size_t)m))
    return -1;
  HIPCHK(c, hipMemcpyAsync(c->d_aidx, idx, sizeof(int) * m, hipMemcpyHostToDevice, c->stream));
  if (dir == 0)
    HIPCHK(c, hipMemcpyAsync(c->d_astage, win, sizeof(float) * m * s3, hipMemcpyHostToDevice, c->stream));
  if (launched(c, "k_affine_move", launch_affine_move(c->stream, dir, c->d_aidx, m, s3, c->d_astage, c->d_aff_store)))
    return -1;
  if (dir == 1)
    HIPCHK(c, hipMemcpyAsync(win, c->d_astage, sizeof(float) * m * s3, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

KLT_API int klt_hip_affine_put(klt_hip_ctx *c, const int *idx, int m, const float *win) {
  return affine_move(c, 0, idx, m, const_cast<float *>(win));
}

KLT_API int klt_hip_affine_get(klt_hip_ctx *c, const int *idx, int m, float *win) {
  return affine_move(c, 1, idx, m, win);
}

KLT_API int klt_hip_track_affine(klt_hip_ctx *c, int s1, int s2, const klt_hip_track_desc *d,
                                 const klt_hip_affine_desc *ad, float *x, float *y, int *val, float *aff,
                                 int *state, int n) {
  if (!c || !d || !ad || (n > 0 && (!x || !y || !val || !aff || !state)))
    return fail(c, "track_affine: null argument");
  if (affine_desc_check(c, ad, "track_affine")) return -1;
  if (c->fb_on)
    return fail(c, "track_affine: the forward-backward check does not combine with the affine check (klt_hip_set_fb)");
  if (c->aff_on)
    return fail(c, "track_affine: the affine check is set to run inside the tracker launch "
                "(klt_hip_set_frames_affine); turn that off for per-call checks");
  if (c->pred_on)
    return fail(c, "track_affine: the affine check does not combine with the motion prior (klt_hip_set_predict)");
  if (mask_tracks(c))
    return fail(c, "track_affine: the affine check does not combine with the region mask's tracking use "
                "(klt_hip_set_mask)");
  if (n <= 0) return 0;
  if (s1 < 0 || s1 >= KLT_HIP_MAX_SLOTS || s2 < 0 || s2 >= KLT_HIP_MAX_SLOTS)
    return fail(c, "track_affine: bad slot");
  const int S = (ad->window_width + 2) * (ad->window_height + 2);
  if (!c->d_aff_store || c->aff_S != S || c->aff_store_cap < (size_t)n * 3 * S)
    return fail(c, "track_affine: window store not reserved for %d features (klt_hip_affine_reserve)", n);
  if (use_device(c)) return -1;
  if (grow(c, &c->d_aff, &c->aff_cap, (size_t)n * 6) || grow(c, &c->d_astate, &c->astate_cap, (size_t)n) ||
      grow(c, &c->d_xp, &c->xp_cap, (size_t)n) || grow(c, &c->d_yp, &c->yp_cap, (size_t)n))
    return -1;
  // positions before the translation track: the window is stored around them
  HIPCHK(c, hipMemcpyAsync(c->d_xp, x, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_yp, y, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_aff, aff, sizeof(float) * n * 6, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_astate, state, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
  if (feat_stage_in(c, x, y, val, n)) return -1;
  if (klt_hip_track(c, s1, s2, d, c->d_fx, c->d_fy, c->d_fv, n, 1)) return -1;
  const Slot &A = c->slot[s1], &B = c->slot[s2];
  // k_affine reads level 0 as planes
  TrkLevel pa = level_view(A.lv[0]), pb = level_view(B.lv[0]);
  for (int k = 0; k < 2; ++k) {
    TrkLevel &L = k == 0 ? pa : pb;
    if (!L.il) continue;
    const long np = (long)L.w * L.h;
    if (grow(c, &c->pl_scr[k][0], &c->pl_cap[k][0], (size_t)(3 * np))) return -1;
    float *p = c->pl_scr[k][0];
    if (launched(c, "k_from_il", launch_from_il(c->stream, L.img, p, p + np, p + 2 * np, np))) return -1;
    L = TrkLevel{p, p + np, p + 2 * np, L.w, L.h};
  }
  AffArgs a;
  memset(&a, 0, sizeof a);
  a.ai = pa.img;
  a.agx = pa.gx;
  a.agy = pa.gy;
  a.aw = pa.w;
  a.ah = pa.h;
  a.bi = pb.img;
  a.bgx = pb.gx;
  a.bgy = pb.gy;
  a.bw = pb.w;
  a.bh = pb.h;
  a.xp = c->d_xp;
  a.yp = c->d_yp;
  a.x = c->d_fx;
  a.y = c->d_fy;
  a.v = c->d_fv;
  a.xo = c->d_fx;
  a.yo = c->d_fy;
  a.aff = c->d_aff;
  a.state = c->d_astate;
  a.store = c->d_aff_store;
  a.n = n;
  a.p = affine_params(ad);
  if (launched(c, "k_affine", launch_affine(c->stream, a))) return -1;
  HIPCHK(c, hipMemcpyAsync(x, c->d_fx, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(y, c->d_fy, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(val, c->d_fv, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(aff, c->d_aff, sizeof(float) * n * 6, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(state, c->d_astate, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// Pipelined sequence: pyramids are built on a second stream one frame ahead of
// the tracker.  Three slots rotate: frame t's pyramid goes into the slot that
// held frame t-3, which the tracker released after tracking t-3 -> t-2.
KLT_API int klt_hip_track_sequence(klt_hip_ctx *c, const klt_hip_pyr_desc *pd, const klt_hip_track_desc *td,
                                   const unsigned char *frames, long pitch, long stride, int t0, int nsteps,
                                   float *x, float *y, int *val, int n, int *cur_slot) {
  if (!c || !pd || !td || !frames || !cur_slot) return fail(c, "track_sequence: null argument");
  if (*cur_slot < 0 || *cur_slot > 2) return fail(c, "track_sequence: cur_slot must be 0, 1 or 2");
  if (c->rep_on)
    return fail(c, "track_sequence: not covered while lost features are replaced (klt_hip_set_frames_replace)");
  if (nsteps <= 0) return 0;
  if (mask_track_refused(c, td, false, "track_sequence") || mask_refused(c, pd->ncols, "track_sequence")) return -1;
  if (pred_refused(c, td, false, "track_sequence") || fb_refused(c, td, false, "track_sequence") ||
      aff_refused(c, td, false, n, "track_sequence"))
    return -1;
  AffCall aff_call(c);
  if (use_device(c)) return -1;
  if (ensure_pipeline(c)) return -1;
  // the pyramid stream starts behind everything already queued on the tracking stream
  HIPCHK(c, hipEventRecord(c->ev_start, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->pstream, c->ev_start, 0));
  hipStream_t track_stream = c->stream;
  for (int k = 0; k < nsteps; ++k) {
    const int prev = *cur_slot, next = (prev + 1) % 3;
    HIPCHK(c, hipStreamWaitEvent(c->pstream, c->ev_free[next], 0));
    if (build_pyramid_on(c, next, pd, frames + (long)(t0 + k) * stride, pitch, 0, c->pstream)) return -1;
    HIPCHK(c, hipEventRecord(c->ev_built[next], c->pstream));
    HIPCHK(c, hipStreamWaitEvent(track_stream, c->ev_built[next], 0));
    if (klt_hip_track(c, prev, next, td, x, y, val, n, 1)) return -1;
    HIPCHK(c, hipEventRecord(c->ev_free[prev], track_stream));
    *cur_slot = next;
  }
  return 0;
}
