// track7_body.h -- the body shared by k_track7 and k_track7_fb (track7.hip),
// included inside each kernel: the FB-off kernels keep their by-value
// arguments and compile to what they were before the forward-backward
// instances existed.  The including kernel provides: the template parameters
// BAND, AOS, NL, FAST, LAZY, HOOK; constexpr bool FB, MULTI, PRED, MASK; TrkArgs a;
// TrkFramesArgs b; TrkFbArgs fb; TrkMultiArgs ms; TrkPredArgs pr; TrkMaskArgs mk;
// fx, fy, fv, n; and the LDS array red_all.  The lazy-gradient instances run at their scalar register
// limit; what LATE, ROLL and the pinned lane numbers below do for them keeps
// spilled scalars and argument loads out of their frame loop (DESIGN section 4,
// "Scalar spills off the lazy tracker's chain").  Every other instance
// compiles to the code it was.
  // LATE: what only a leaving wave needs is read from the argument segment
  // there (track7.hip's T7KArgs: the arguments of k_track7 / k_track7_hook)
  constexpr bool LATE = LAZY && !FB && !MULTI;
  static_assert(!PRED || (!FB && !MULTI && !LAZY && !BAND && !FAST && !HOOK), "k_track7_pred: full records, exact sums");
  static_assert(!MASK || (!FB && !MULTI && !BAND && !FAST && !PRED && LAZY == HOOK),
                "k_track7_mask: exact sums on full records, k_track7_mask_lazy: the lazy-gradient hook instances");
  static_assert(!HOOK || LATE, "wave_exit reads T7KArgs");
  if (a.prio) __builtin_amdgcn_s_setprio(3);  // the chain issues ahead of co-resident pyramid waves
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if constexpr (HOOK)
    if (b.wave_t && lane == 0) wave_time(b.wave_t, 0, blockIdx.x * kWaves + wave);
  if (b.n_dev) n = *b.n_dev;
  // XCD-major block order over the (band-sorted) features actually processed
  const int xcd_per = b.n_dev && b.xcd_per > 0 ? ((n + kWaves - 1) / kWaves + 7) / 8 : b.xcd_per;
  if (xcd_per > 0 && (int)(blockIdx.x / 8) >= xcd_per) {
    if constexpr (HOOK) wave_exit(lane, blockIdx.x * kWaves + wave);
    return;
  }
  const int blk = xcd_per > 0 ? (int)(blockIdx.x % 8) * xcd_per + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int slot = blk * kWaves + wave;
  if (slot >= n) {  // whole wave; no workgroup barrier in this kernel
    if constexpr (HOOK) wave_exit(lane, slot);
    return;
  }
  const int f = u(b.perm ? b.perm[slot] : slot);
  // MULTI: the sequence of this wave's feature -- a wave's own lookup (the
  // four features of a workgroup may belong to different sequences), by
  // bisection over the sequences' first features, scalar throughout:
  // first[sq] <= f < first[sq + 1], empty sequences skipped
  int sq = 0, nsq = 1;
  if constexpr (MULTI) {
    nsq = ms.nseq;
    int hi = nsq;
    while (hi - sq > 1) {
      const int mid = (sq + hi) >> 1;
      if (f >= ms.first[mid]) sq = mid;
      else hi = mid;
    }
    sq = u(sq);
  }
  float *red = red_all[wave];
  for (int i = lane; i < kRedF; i += kWave) red[i] = 0.0f;  // pads stay +0
  wave_lds_sync();
  // lane p < 49: window pixel p; lanes past the window take the last pixel's
  // offsets (valid addresses) and contribute nothing
  const bool on = lane < kNpx;
  const int pl = on ? lane : kNpx - 1;
  const float fi = (float)(pl % kWin - kHw), fj = (float)(pl / kWin - kHw);  // x + i in the reference: int i as float

  float x = u(fx[f]), y = u(fy[f]);
  int v = u(fv[f]);
  const int nlev = NL > 0 ? NL : a.nlev;
  const bool merge = !FB && !PRED && (!MASK || LAZY) && a.merge_res && nlev >= 2;
  // PRED (klt_hip_set_predict): the feature's last displacement, wave-uniform
  // over the frames; loaded with the list, stored with it by lane 0
  float pvx = 0.0f, pvy = 0.0f;
  if constexpr (PRED) pvx = u(pr.vx[f]), pvy = u(pr.vy[f]);
  Pending pd;
  Counts cnt;
  Carry carry;  // lazy-gradient instances: the last level-0 pass's image-2 corners (unused otherwise)
#ifdef KLT_TRACK_PROF
  const unsigned long long wall0 = wall_clock64();
#endif
  // ROLL (the lazy-gradient instances of a compile-time depth): image 1's level
  // bases are carried from frame to frame -- the kept pyramid's (a.A) for the
  // launch's first frame, then the bank frame just tracked -- with its level-0
  // layout, so that the frame loop selects nothing and reads no field of a.A
  constexpr bool ROLL = LAZY && NL > 0 && !FB && !MULTI;
  const float *pimg[NL > 0 ? NL : 1] = {};
  int pil = kLayoutImg;
  if constexpr (ROLL) {
#pragma unroll
    for (int r = 0; r < NL; ++r) pimg[r] = a.A[r].img;
    pil = a.A[0].il;
  }
  for (int j = 0; j < b.nframes; ++j) {
    T7_T(t_f0);
    const bool job = pd.on;  // frame j-1 is tentatively tracked at (x, y)
    const float xp = x, yp = y;
    int rstat = kTracked;
    if constexpr (PRED)
      if (v != 0) pvx = 0.0f, pvy = 0.0f;  // lost, or fresh from selection or replacement: no prior
    if (v >= 0 || job) {
      // one frame of KLTTrackFeatures for this feature (:1348-1437)
      const Lev R = lev_img1<MULTI, ROLL>(a, b, 0, j, sq, nsq, pimg[0], pil);
      // the corners kept from frame j-1 serve this frame's level 0 only: a frame
      // that does not reach level 0 leaves nothing for the one after it
      const unsigned cpx = carry.px;
      carry.px = ~0u;
      float xl = x, yl = y;
#pragma unroll
      for (int r = nlev - 1; r >= 0; --r) {  // xloc /= subsampling, nlev times (:1352-1355)
        xl = u(a.ss_inv != 0.0f ? xl * a.ss_inv : xl / a.ss);
        yl = u(a.ss_inv != 0.0f ? yl * a.ss_inv : yl / a.ss);
      }
      float xo = xl, yo = yl;
      if constexpr (PRED) {  // image 2's start: the position moved by the last displacement, scaled like xl
        xo = u(x + pvx);
        yo = u(y + pvy);
#pragma unroll
        for (int r = nlev - 1; r >= 0; --r) {
          xo = u(a.ss_inv != 0.0f ? xo * a.ss_inv : xo / a.ss);
          yo = u(a.ss_inv != 0.0f ? yo * a.ss_inv : yo / a.ss);
        }
      }
      int val = kTracked;
      bool lost_prev = false;
#pragma unroll
      for (int r = nlev - 1; r >= 0; --r) {
        xl = u(xl * a.ss);
        yl = u(yl * a.ss);
        xo = u(xo * a.ss);
        yo = u(yo * a.ss);
        const Lev LA = lev_img1<MULTI, ROLL>(a, b, r, j, sq, nsq, pimg[ROLL ? r : 0], pil);
        const Lev LB = lev_cur<MULTI>(a, b, r, j, sq, nsq);
        if constexpr (PRED)  // a start whose window is not inside the coarsest level (NaN included): unpredicted
          if (r == nlev - 1) {
            const bool in = !out7(xo, yo, LB.tx, LB.ty);
            xo = u(in ? xo : xl);
            yo = u(in ? yo : yl);
          }
        const bool lj = job && r == nlev - 1;
        T7_T(t_l0);
        if (LAZY && r == 0)
          val = level7<BAND, AOS, FAST, LAZY ? 2 : 0>(a, LA, LB, xl, yl, xo, yo, lane, fi, fj, on, red, true,
                                                      merge && j + 1 < b.nframes, pd, lj, R, rstat, lost_prev, cnt,
                                                      &carry, cpx);
        else
          val = level7<BAND, AOS, FAST, LAZY ? 1 : 0>(a, LA, LB, xl, yl, xo, yo, lane, fi, fj, on, red, r == 0,
                           merge && r == 0 && j + 1 < b.nframes, pd, lj, R, rstat, lost_prev, cnt);
        T7_ADD(10, t_l0);
        if (lost_prev) break;
        if (val == kSmallDet || val == kOOB) break;
      }
      if (!lost_prev) {
        const bool border = xo < a.borderx || xo > a.ncols - 1 - a.borderx || yo < a.bordery ||
                            yo > a.nrows - 1 - a.bordery;
        // MASK (klt_hip_set_mask): a test of position like the border's, after it.
        // Every level ran unless the loop broke (SMALL_DET is left alone, OOB
        // comes first), so (xo, yo) is a level-0 position: on a masked pixel the
        // frame's status is kMasked whatever the residue or the iteration count
        // and a residue verdict deferred to the next frame is dropped: the
        // tentative position is tested at once.  One byte per feature-frame, at a
        // wave-uniform address.  The lazy-gradient instances read the mask's
        // pointer and pitch from the argument segment here, frame by frame (two
        // scalar loads the compiler may not hoist), so that they hold no scalar
        // registers over the frame loop
        if constexpr (MASK)
          if (val != kOOB && !border && val != kSmallDet && xo >= 0.0f && yo >= 0.0f && xo < (float)a.ncols &&
              yo < (float)a.nrows) {
            const unsigned char *mp = mk.mask;
            long mpitch = mk.pitch;
            if constexpr (LATE) {
              T7MaskKArgsPtr ka = t7_mask_kargs();
              asm volatile("" : "+s"(ka));
              mp = ka->mk.mask;
              mpitch = ka->mk.pitch;
            }
            if (mp[(long)u((int)yo) * mpitch + u((int)xo)] == 0) {
              val = kMasked;
              pd.on = false;
            }
          }
        if (val == kOOB || border) {
          pd.on = false;  // outside the border: OOB whatever the residue (trackFeatures.c:1383-1398)
          x = -1.0f;
          y = -1.0f;
          v = kOOB;
        } else if (val != kTracked) {
          x = -1.0f;
          y = -1.0f;
          v = val;
        } else {
          x = xo;
          y = yo;
          v = kTracked;
        }
      }
    }
    if constexpr (PRED) {  // two float subtractions; a lost feature keeps no motion
      pvx = v == kTracked ? u(x - xp) : 0.0f;
      pvy = v == kTracked ? u(y - yp) : 0.0f;
      if (pr.tvx && lane == 0) {
        pr.tvx[j * pr.tstride + f] = pvx;
        pr.tvy[j * pr.tstride + f] = pvy;
      }
    }
    if constexpr (FB) {
      float e = -1.0f;  // no distance: lost before, by, or on the way back from this frame
      if (v == kTracked) {
        // KLTTrackFeatures(img2, img1) from the forward position: bank frame j is image 1
        float xl = x, yl = y;
#pragma unroll
        for (int r = nlev - 1; r >= 0; --r) {
          xl = u(a.ss_inv != 0.0f ? xl * a.ss_inv : xl / a.ss);
          yl = u(a.ss_inv != 0.0f ? yl * a.ss_inv : yl / a.ss);
        }
        float xo = xl, yo = yl;
        int vb = kTracked;
        bool none = false;
        const Lev R = lev_prev(a, b, 0, j);  // unused without a job
#pragma unroll
        for (int r = nlev - 1; r >= 0; --r) {
          xl = u(xl * a.ss);
          yl = u(yl * a.ss);
          xo = u(xo * a.ss);
          yo = u(yo * a.ss);
          const Lev LA = lev_of(a.B[r], (long)j * b.lfs[r], a.oobx[r], a.ooby[r]);
          const Lev LB = lev_prev(a, b, r, j);
          vb = level7<false, AOS, false>(a, LA, LB, xl, yl, xo, yo, lane, fi, fj, on, red, r == 0, false, pd, false, R,
                                         rstat, none, cnt);
          if (vb == kSmallDet || vb == kOOB) break;
        }
        const bool border = xo < a.borderx || xo > a.ncols - 1 - a.borderx || yo < a.bordery ||
                            yo > a.nrows - 1 - a.bordery;
        bool rej = vb != kTracked || border;
        if (!rej) {  // five float operations, each rounded (contraction is off in this file)
          const float dx = xo - xp, dy = yo - yp;
          const float dx2 = dx * dx, dy2 = dy * dy;
          e = u(dx2 + dy2);
          rej = e > fb.t2;
        }
        if (rej) {
          x = -1.0f;
          y = -1.0f;
          v = kFbRejected;
        }
      }
      if (fb.err && lane == 0) fb.err[j * fb.stride + f] = e;
    }
    // the table's writer: in the LATE instances a lane number the compiler cannot
    // see through, so that it keeps no lane mask alive (or spilled) over the frames
    int tl = lane;
    if constexpr (LATE) asm volatile("" : "+v"(tl));
    if (job) {  // frame j-1's verdict came with frame j's first pass
      if (rstat != kTracked) {
        x = -1.0f;
        y = -1.0f;
        v = rstat;
      }
      if (b.tx && tl == 0) {
        b.tx[(j - 1) * b.tstride + f] = rstat != kTracked ? -1.0f : xp;
        b.ty[(j - 1) * b.tstride + f] = rstat != kTracked ? -1.0f : yp;
        b.tv[(j - 1) * b.tstride + f] = rstat;
      }
    }
    if (b.tx && tl == 0 && !pd.on) {
      b.tx[j * b.tstride + f] = x;
      b.ty[j * b.tstride + f] = y;
      b.tv[j * b.tstride + f] = v;
    }
    if constexpr (ROLL) {  // this frame's image 2 is the next frame's image 1
#pragma unroll
      for (int r = 0; r < NL; ++r) pimg[r] = a.B[r].img + (long)j * b.lfs[r];
      pil = kLayoutImg;
    }
    T7_ADD(4, t_f0);
  }
#ifdef KLT_TRACK_PROF
  cnt.c[5] = cnt.solves;
  cnt.c[6] = cnt.passes;
  cnt.c[8] = wall0;
  cnt.c[9] = wall_clock64();
  cnt.c[7] = cnt.c[9] - wall0;
  if (b.prof && lane == 0)
    for (int k = 0; k < kProfN; ++k) b.prof[(long)slot * kProfN + k] = cnt.c[k];
#endif
  if (lane == 0) {
    float *ox = fx, *oy = fy;
    int *ov = fv;
    unsigned long long *count = nullptr;
    if constexpr (LATE) {
      const T7KArgsPtr ka = t7_kargs();
      ox = ka->fx, oy = ka->fy, ov = ka->fv, count = ka->b.count;
    } else {
      count = b.count;
    }
    ox[f] = x;
    oy[f] = y;
    ov[f] = v;
    if constexpr (PRED) {
      pr.vx[f] = pvx;
      pr.vy[f] = pvy;
    }
    if (count) {
      const int k = slot & (kCountSlots - 1);
      atomicAdd(&count[k], (unsigned long long)cnt.solves);
      atomicAdd(&count[kCountSlots + k], (unsigned long long)cnt.passes);
    }
  }
  if constexpr (HOOK) wave_exit(lane, f);
