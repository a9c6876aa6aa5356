// track_body.h -- the body shared by k_track_frames_g, k_track_frames_g_fb and
// k_track_frames_g_aff (track.hip), included inside each kernel: the plain
// kernels keep their by-value arguments and compile to what they were before
// the forward-backward and affine instances existed.  The including kernel
// provides: the template parameters PPL, PATCH, WIN, EXACT, LI, BAND;
// constexpr bool FB, AFF; TrkArgs a; TrkFramesArgs b; TrkFbArgs fb; TrkAffArgs
// af; fx, fy, fv, n; the LDS array red_all; and, AFF, the dynamic LDS aff_dyn.
  if (a.prio) __builtin_amdgcn_s_setprio(3);  // the chain issues ahead of co-resident pyramid waves
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  // consecutive workgroups land on the 8 XCDs round-robin: give each XCD a
  // contiguous run of the (band-sorted) order so its L2 sees one image band
  if (b.n_dev) n = *b.n_dev;
  // band mode: the grid is sized for every feature, but only the n_dev kept
  // ones are processed -- spread THEIR blocks over the 8 XCDs (a per-XCD run
  // sized for all features would put a small band on one XCD)
  const int xcd_per = b.n_dev && b.xcd_per > 0 ? ((n + kBlock / kWave - 1) / (kBlock / kWave) + 7) / 8 : b.xcd_per;
  if (xcd_per > 0 && (int)(blockIdx.x / 8) >= xcd_per) return;  // past this XCD's run: no duplicate slots
  const int blk = xcd_per > 0 ? (int)(blockIdx.x % 8) * xcd_per + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int slot = blk * (kBlock / kWave) + wave;
  if (slot >= n) return;  // whole wave; the kernel has no workgroup barrier
  const int f = b.perm ? b.perm[slot] : slot;
  float x = uni(fx[f]), y = uni(fy[f]);
  int v = uni(fv[f]);
  const LaneWin<PPL, PATCH, WIN> w = lane_window<PPL, PATCH, WIN>(a.ww, a.wh, lane);
  {  // row pads of the ordered-sum staging stay +0 for the whole kernel
    float *red = red_all[wave];
    for (int i = lane; i < red_floats(PPL); i += kWave) red[i] = 0.0f;
    lds_wave_sync();
  }
  const bool head = lane == 0;
#ifdef KLT_TRACK_PROF
  Prof prof;
  const unsigned long long wall0 = wall_clock64();
#endif
  // deferred residues (ResCarry): one-feature waves, exact sums, default gain
  // (band mode too: the residue's rows were checked against the band at frame
  // j's final position, and an escape voids the whole chunk anyway)
  const bool merge = !FB && !AFF && EXACT && !LI && a.merge_res && a.nlev >= 2;
  ResCarry<PPL> rc;
  TrkCount cnt;
  // affine check: the feature's six values and its window state stay in
  // (wave-uniform) registers for the launch
  float aff6[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  int ast = 0;
  if constexpr (AFF) {
#pragma unroll
    for (int q = 0; q < 6; ++q) aff6[q] = uni(af.aff[6 * (long)f + q]);
    ast = uni(af.state[f]);
    if (af.fresh) ast = ast != 0 ? 1 : 0;  // held from before the call
  }
  for (int j = 0; j < b.nframes; ++j) {
    const bool job = rc.pending;  // frame j-1 is tentatively tracked at (x, y)
    const bool live = v >= 0 || job;  // lost features are not tracked (:1346)
    const float xp = x, yp = y;
    int rstat = kTracked;
    PROF_T(t_f0);
    if (wave_any(live)) {
      auto LA = [&](int r) { return j == 0 ? a.A[r] : at_frame(a.B[r], (long)(j - 1) * b.lfs[r]); };
      track_feature<PPL, PATCH, WIN, EXACT, LI, BAND>(
          PROF_ARG a, w, LA, [&](int r) { return at_frame(a.B[r], (long)j * b.lfs[r]); }, x, y, v, live, lane,
          red_all[wave], rc, job, merge && j + 1 < b.nframes, LA(0), rstat, cnt);
    }
    if constexpr (FB) {
      float e = -1.0f;  // no distance: lost before, by, or on the way back from this frame
      const bool back = live && v == kTracked;
      if (wave_any(back)) {
        auto LA = [&](int r) { return j == 0 ? a.A[r] : at_frame(a.B[r], (long)(j - 1) * b.lfs[r]); };
        float xb = x, yb = y;
        int vb = v;
        track_feature<PPL, PATCH, WIN, EXACT, LI, BAND>(
            PROF_ARG a, w, [&](int r) { return at_frame(a.B[r], (long)j * b.lfs[r]); }, LA, xb, yb, vb, back, lane,
            red_all[wave], rc, false, false, LA(0), rstat, cnt);
        if (back) {
          bool rej = vb != kTracked;
          if (!rej) {  // five float operations, each rounded (contraction is off in this file)
            const float dx = xb - xp, dy = yb - yp;
            const float dx2 = dx * dx, dy2 = dy * dy;
            e = uni(dx2 + dy2);
            rej = e > fb.t2;
          }
          if (rej) {
            x = -1.0f;
            y = -1.0f;
            v = kFbRejected;
          }
        }
      }
      if (fb.err && head) fb.err[j * fb.stride + f] = e;
    }
    if constexpr (AFF) {
      // the reference's record stage (trackFeatures.c:1438-1497) for a feature
      // frame j's translation step left TRACKED (no deferred residue: its
      // verdict is final), on level 0 as planes; every operand is wave-uniform
      if (live && v == kTracked) {
        const TrkLevel P = j == 0 ? a.A[0] : at_frame(a.B[0], (long)(j - 1) * b.lfs[0]);
        const TrkLevel Q = at_frame(a.B[0], (long)j * b.lfs[0]);
        const AffImg I1{P.img, P.gx, P.gy, P.w, P.h}, I2{Q.img, Q.gx, Q.gy, Q.w, Q.h};
        const int S = (af.p.ww + 2) * (af.p.wh + 2);
        float *lds = aff_dyn + wave * af.lds_wave;
        const int was = ast;
        int status;
        ast = aff_stage<kAffChunk>(lds, lds + af.lds_wave - aff::SOLVE, af.p, I1, I2,
                                   af.store + (size_t)f * 3 * S, aff6, xp, yp, x, y, ast, lane, status);
        if (status != kTracked) {
          x = -1.0f;
          y = -1.0f;
          v = status;
        }
        if (was == 0) {
          // the window this wave just stored is read from the next frame on,
          // each lane reading what other lanes wrote (and lines that hold a
          // neighbour's window too): stores complete, stale lines dropped
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
      } else {
        ast = 0;  // lost by the translation step, now or before: no window
      }
      if (head) {
        if (af.tab_aff) {
          float *row = af.tab_aff + 6 * ((long)j * af.stride + f);
#pragma unroll
          for (int q = 0; q < 6; ++q) row[q] = aff6[q];
        }
        if (af.tab_state) af.tab_state[(long)j * af.stride + f] = ast;
      }
    }
    PROF_ADD(4, t_f0);
    if (job) {  // frame j-1's verdict came with frame j's first pass
      if (rstat != kTracked) {
        x = -1.0f;
        y = -1.0f;
        v = rstat;
      }
      if (b.tx && head) {
        b.tx[(j - 1) * b.tstride + f] = rstat != kTracked ? -1.0f : xp;
        b.ty[(j - 1) * b.tstride + f] = rstat != kTracked ? -1.0f : yp;
        b.tv[(j - 1) * b.tstride + f] = rstat;
      }
    }
    if (b.tx && head && !rc.pending) {
      b.tx[j * b.tstride + f] = x;
      b.ty[j * b.tstride + f] = y;
      b.tv[j * b.tstride + f] = v;
    }
  }
  if (head) {
    fx[f] = x;
    fy[f] = y;
    fv[f] = v;
    if constexpr (AFF) {
#pragma unroll
      for (int q = 0; q < 6; ++q) af.aff[6 * (long)f + q] = aff6[q];
      af.state[f] = ast;
    }
    if (b.count) {  // one pair of atomics per feature per launch, spread over kCountSlots addresses
      const int k = (blk * (kBlock / kWave) + wave) & (kCountSlots - 1);
      atomicAdd(&b.count[k], (unsigned long long)cnt.solves);
      atomicAdd(&b.count[kCountSlots + k], (unsigned long long)cnt.passes);
    }
  }
#ifdef KLT_TRACK_PROF
  prof.c[8] = wall0;
  prof.c[9] = wall_clock64();
  prof.c[7] = prof.c[9] - wall0;  // constant-rate ticks over the wave's life
  if (b.prof && lane == 0)
    for (int k = 0; k < kProfN; ++k) b.prof[(long)(blk * (kBlock / kWave) + wave) * kProfN + k] = prof.c[k];
#endif
