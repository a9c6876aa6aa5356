// runtime_pyr.hip -- host side of libklt_amd.so: pyramid slots, the bank arena
// of the batched calls, and the pyramid builds that drive pyramid.hip
// (runtime.h).  No kernels here.
#include "runtime.h"

bool fused_ok(const klt_hip_pyr_desc *d) {
  return d->smooth_input && d->smooth.width == 2 * kRS + 1 && d->grad_gauss.width == 2 * kRG + 1 &&
         d->grad_deriv.width == 2 * kRG + 1 && d->grad_deriv.k[kRG] == 0.0f && kDC == kRG &&
         (d->nlevels == 1 || (d->nlevels == 2 && d->subsampling == kSS && d->pyr.width == 2 * kRP + 1));
}

int ensure_slot(klt_hip_ctx *c, int s, const klt_hip_pyr_desc *d) {
  Slot &S = c->slot[s];
  int w = d->ncols, h = d->nrows;
  S.nlev = d->nlevels;
  S.ss = d->nlevels > 1 ? d->subsampling : 1;
  for (int l = 0; l < d->nlevels; ++l) {
    Level &L = S.lv[l];
    L.w = w;
    L.h = h;
    size_t n = (size_t)w * h;
    if (L.cap < n || !L.img) {
      if (L.img) hipFree(L.img);
      L.img = L.gx = L.gy = nullptr;
      const size_t m = n ? n : 1;
      HIPCHK(c, hipMalloc((void **)&L.img, 3 * m * sizeof(float)));
      L.gx = L.img + m;
      L.gy = L.img + 2 * m;
      L.cap = m;
    }
    w /= d->subsampling > 0 ? d->subsampling : 1;
    h /= d->subsampling > 0 ? d->subsampling : 1;
  }
  return 0;
}

namespace {
// the level-0 input as floats: the generic path's first pass (fmt: the source pixels)
hipError_t to_f32(hipStream_t st, const uint8_t *src, long pitch, int W, int H, int fmt, float *out) {
  return fmt == KLT_HIP_FRAME_GRAY8 ? launch_u8_to_f32(st, src, pitch, W, H, out)
                                    : launch_px_to_f32(st, src, pitch, W, H, fmt, out);
}

int build_generic(klt_hip_ctx *c, int s, const klt_hip_pyr_desc *d, const uint8_t *src, long pitch,
                  hipStream_t st, int fmt) {
  Slot &S = c->slot[s];
  for (int l = 0; l < d->nlevels; ++l) S.lv[l].il = 0;  // planes
  const long n0 = (long)d->ncols * d->nrows;
  if (grow(c, &c->d_tmp[0], &c->tmp_cap[0], (size_t)n0)) return -1;
  if (grow(c, &c->d_tmp[1], &c->tmp_cap[1], (size_t)n0)) return -1;
  TimedScope ts(c, T_GEN, st);
  const RTaps sm = reverse_taps(d->smooth), py = reverse_taps(d->pyr);
  const RTaps gg = reverse_taps(d->grad_gauss), gd = reverse_taps(d->grad_deriv);
  Level &L0 = S.lv[0];
  float *t0 = c->d_tmp[0], *t1 = c->d_tmp[1];
  if (n0 > 0) {
    if (d->smooth_input) {
      if (launched(c, "k_u8_to_f32", to_f32(st, src, pitch, d->ncols, d->nrows, fmt, t1)) ||
          launched(c, "k_rows", launch_rows(st, t1, d->ncols, d->nrows, sm, t0)) ||
          launched(c, "k_cols", launch_cols(st, t0, d->ncols, d->nrows, sm, L0.img)))
        return -1;
    } else {
      if (launched(c, "k_u8_to_f32", to_f32(st, src, pitch, d->ncols, d->nrows, fmt, L0.img))) return -1;
    }
  }
  for (int l = 1; l < d->nlevels; ++l) {
    Level &P = S.lv[l - 1], &L = S.lv[l];
    if ((long)P.w * P.h == 0) continue;
    if (launched(c, "k_rows", launch_rows(st, P.img, P.w, P.h, py, t0)) ||
        launched(c, "k_cols", launch_cols(st, t0, P.w, P.h, py, t1)) ||
        launched(c, "k_subsample", launch_subsample(st, t1, P.w, d->subsampling, L.img, L.w, L.h)))
      return -1;
  }
  for (int l = 0; l < d->nlevels; ++l) {
    Level &L = S.lv[l];
    if (launched(c, "k_rows", launch_rows(st, L.img, L.w, L.h, gd, t0)) ||
        launched(c, "k_cols", launch_cols(st, t0, L.w, L.h, gg, L.gx)) ||
        launched(c, "k_rows", launch_rows(st, L.img, L.w, L.h, gg, t0)) ||
        launched(c, "k_cols", launch_cols(st, t0, L.w, L.h, gd, L.gy)))
      return -1;
  }
  return 0;
}

DefTaps default_taps(const klt_hip_pyr_desc *d) {
  DefTaps T;
  const RTaps s = reverse_taps(d->smooth), g = reverse_taps(d->grad_gauss);
  const RTaps dd = reverse_taps(d->grad_deriv), p = reverse_taps(d->pyr);
  for (int m = 0; m < 5; ++m) T.s[m] = s.k[m];
  for (int m = 0; m < 7; ++m) {
    T.g[m] = g.k[m];
    T.d[m] = dd.k[m];
  }
  for (int m = 0; m < 21; ++m) T.p[m] = d->nlevels > 1 ? p.k[m] : 0.0f;
  return T;
}

// Level 0 of the fused pyramid for F frames, rows [r0, r1) (global
// coordinates; every built value is the full-frame value).  Whole 32-row tiles:
// the rows actually built are returned in r0/r1.
int launch_l0(klt_hip_ctx *c, hipStream_t st, const uint8_t *src, long pitch, long stride, int W, int H,
              const DefTaps &T, int vec_u8, int vec_out, float *img, float *gx, float *gy, float *hs, int W1,
              int do_hs, long fs0, long fsh, int F, int &r0, int &r1, int *p0 = nullptr, int *p1 = nullptr,
              int il = 0, int fmt = KLT_HIP_FRAME_GRAY8) {
  if (r1 <= r0 || F <= 0) return 0;
  const int TH = geom::L0_TH;
  const int nty = (H + TH - 1) / TH;
  const int ty0 = r0 / TH, ty1 = r1 >= H ? nty : clampi((r1 + TH - 1) / TH, ty0, nty);
  r0 = ty0 * TH;
  r1 = ty1 >= nty ? H : ty1 * TH;
  // planes rows [*p0, *p1) (whole tiles, inside the built ones); null: every built tile
  int py0 = ty0, py1 = ty1;
  if (p0 && p1) {
    py0 = clampi(*p0 / TH, ty0, ty1);
    py1 = *p1 >= H ? ty1 : clampi((*p1 + TH - 1) / TH, py0, ty1);
    *p0 = py0 * TH;
    *p1 = py1 >= nty ? H : py1 * TH;
  }
  return launched(c, "k_pyr_l0", launch_pyr_l0(st, src, (int)pitch, stride, W, H, T, vec_u8, vec_out, img, gx, gy,
                                               hs, W1, do_hs, fs0, fsh, F, ty0, ty1, py0, py1, il, fmt,
                                               c->l0_strip));
}

// KLT_L1_THIN=0: a single frame's level 1 in 32-row tiles too (A/B)
bool l1_thin() {
  static const bool on = [] {
    const char *v = getenv("KLT_L1_THIN");
    return !(v && *v && atoi(v) == 0);
  }();
  return on;
}

int build_fused(klt_hip_ctx *c, int s, const klt_hip_pyr_desc *d, const uint8_t *src, long pitch,
                hipStream_t st, int fmt) {
  Slot &S = c->slot[s];
  const int W = d->ncols, H = d->nrows;
  const DefTaps T = default_taps(d);
  const bool two = d->nlevels == 2;
  const int W1 = two ? S.lv[1].w : 0, H1 = two ? S.lv[1].h : 0;
  for (int l = 0; l < d->nlevels; ++l) S.lv[l].il = 1;  // interleaved
  if (two && grow(c, &c->d_hs, &c->hs_cap, (size_t)hs_size(W1 > 0 ? W1 : 1, H))) return -1;
  if ((long)W * H == 0) return 0;
  const int vec_u8 = vec_u8_ok(src, pitch, 0L, W);
  const int vec_out = (W % 4 == 0) ? 1 : 0;
  {
    TimedScope ts(c, T_L0, st);
    int r0 = 0, r1 = H;
    if (launch_l0(c, st, src, pitch, 0L, W, H, T, vec_u8, vec_out, S.lv[0].img, S.lv[0].gx, S.lv[0].gy, c->d_hs,
                  W1, (two && W1 > 0) ? 1 : 0, 0L, 0L, 1, r0, r1, nullptr, nullptr, 1, fmt))
      return -1;
  }
  if (two && (long)W1 * H1 > 0) {
    TimedScope ts(c, T_L1, st);
    const int vec = (W1 % 4 == 0 && W1 >= 8) ? 1 : 0;
    // one frame: thin tiles (a 32-row tile per workgroup leaves most CUs idle)
    const int thin = l1_thin() ? 1 : 0, th = thin ? kL1ThinRows : geom::L1_TH;
    const int ty = (H1 + th - 1) / th;
    if (launched(c, "k_pyr_l1", launch_pyr_l1(st, c->d_hs, W1, H, H1, T, vec, S.lv[1].img, S.lv[1].gx, S.lv[1].gy,
                                              0L, 0L, 1, 0, ty, 1, thin)))
      return -1;
  }
  return 0;
}

// The three banks live in one device arena per context: for each bank, level
// l's img | gx | gy planes (each `frames` pyramids long) and the sigma-3.6 row
// pass, every plane on a 64 KiB boundary.  One allocation instead of 21 keeps
// the physical placement of the banks independent of what the process
// allocated and freed before: separate plane allocations made after a smaller
// context's banks were freed ran the 4K pass 7 % slower (staggering
// the planes' offsets by 256 B .. 16 KiB changed nothing).
size_t bank_plane_floats(const klt_hip_pyr_desc *d, int l, int frames) {
  int w = d->ncols, h = d->nrows;
  for (int k = 0; k < l; ++k) {
    w /= d->subsampling;
    h /= d->subsampling;
  }
  return (size_t)(w > 0 ? w : 1) * (h > 0 ? h : 1) * frames;
}

size_t bank_hs_floats(const klt_hip_pyr_desc *d, int frames) {
  const int W1 = d->nlevels == 2 ? d->ncols / d->subsampling : 0;
  return d->nlevels == 2 ? (size_t)hs_size(W1 > 0 ? W1 : 1, d->nrows) * frames : 0;
}

constexpr size_t kPlaneAlign = 64 << 10;
}  // namespace

size_t bank_arena_bytes(const klt_hip_pyr_desc *d, int frames) {
  size_t total = 0;
  auto add = [&](size_t floats) { total = (total + kPlaneAlign - 1) / kPlaneAlign * kPlaneAlign + floats * sizeof(float); };
  for (int b = 0; b < 3; ++b) {
    for (int l = 0; l < d->nlevels; ++l) add(3 * bank_plane_floats(d, l, frames));  // one block per level
    if (d->nlevels == 2) add(bank_hs_floats(d, frames));
  }
  return total;
}

namespace {
size_t env_size(const char *name, size_t dflt) {
  const char *v = getenv(name);
  return v && *v ? (size_t)strtoull(v, nullptr, 10) : dflt;
}
}  // namespace

void free_banks(klt_hip_ctx *c) {
  BankRing &R = c->banks;
  for (auto &K : R.bank) {
    for (auto &L : K.lv) {
      if (!R.arena) hipFree(L.img);  // one block per level
      L.img = L.gx = L.gy = nullptr;
      L.cap = 0;
    }
    if (!R.arena) hipFree(K.hs);
    K.hs = nullptr;
    K.hs_cap = 0;
    K.frames = 0;
  }
  hipFree(R.arena);
  R.arena = nullptr;
  R.arena_bytes = 0;
}

// Default bank budget: a quarter of the device's memory, at most 64 GiB --
// three 64-frame banks of 4K pyramids take 21 GB, of 1080p 5.3 GB.
size_t bank_budget_of(klt_hip_ctx *c) {
  if (c->bank_budget) return c->bank_budget;
  if (!c->dev_total) {
    size_t fr = 0, tot = 0;
    c->dev_total = hipMemGetInfo(&fr, &tot) == hipSuccess && tot ? tot : (size_t)64 << 30;
  }
  const size_t q = c->dev_total / 4, cap = (size_t)64 << 30;
  return q < cap ? q : cap;
}

// the largest chunk whose three banks fit the budget (0: not even one frame)
int budget_chunk(klt_hip_ctx *c, const klt_hip_pyr_desc *d) {
  const size_t budget = bank_budget_of(c), one = bank_arena_bytes(d, 1);
  if (one > budget) return 0;
  int lo = 1, hi = 1 << 16;
  while (lo < hi) {  // bank_arena_bytes grows with frames
    const int mid = lo + (hi - lo + 1) / 2;
    if (bank_arena_bytes(d, mid) <= budget) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// all three banks hold `frames` pyramids shaped like desc d
bool banks_fit(const klt_hip_ctx *c, const klt_hip_pyr_desc *d, int frames) {
  for (const Bank &K : c->banks.bank) {
    if (K.nlev != d->nlevels) return false;
    // the level sizes below follow the bank's own subsampling: a bank laid out
    // for another one (a context reused for a pyramid of the same depth) does
    // not fit, whatever its first level's size
    if (K.ss != (d->nlevels > 1 ? d->subsampling : 1)) return false;
    int w = d->ncols, h = d->nrows;
    for (int l = 0; l < d->nlevels; ++l) {
      const Level &L = K.lv[l];
      if (L.w != w || L.h != h || !L.img || L.cap < (size_t)(w > 0 ? w : 1) * (h > 0 ? h : 1) * frames) return false;
      w /= K.ss;
      h /= K.ss;
    }
    if (d->nlevels == 2 && K.hs_cap < (size_t)(K.lv[1].w > 0 ? K.lv[1].w : 1) * d->nrows * frames) return false;
  }
  return true;
}

// The three banks for `frames` pyramids shaped like desc d.  Banks that do not
// fit are laid out again with both streams drained, and a build-ahead record
// goes with the old layout; a kept pyramid living in a bank is the caller's to
// move out first.
int ensure_banks(klt_hip_ctx *c, const klt_hip_pyr_desc *d, int frames) {
  if (banks_fit(c, d, frames)) return 0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->pstream) HIPCHK(c, hipStreamSynchronize(c->pstream));
  c->banks.drop_ahead();
  const bool arena = env_size("KLT_BANK_ARENA", 1) != 0;  // 0: the old per-plane allocations (A/B only)
  const size_t need = bank_arena_bytes(d, frames);
  if (!arena || need > c->banks.arena_bytes || !c->banks.arena) free_banks(c);
  if (!arena) {  // one allocation per plane (the round-1/2 layout; experiments only)
    for (auto &K : c->banks.bank) {
      for (int l = 0; l < d->nlevels; ++l) {
        const size_t n = bank_plane_floats(d, l, frames);
        HIPCHK(c, hipMalloc((void **)&K.lv[l].img, 3 * n * sizeof(float)));
      }
      if (d->nlevels == 2) HIPCHK(c, hipMalloc((void **)&K.hs, bank_hs_floats(d, frames) * sizeof(float)));
    }
  } else if (!c->banks.arena) {
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    if (need > fr)
      return fail(c, "track_frames: the bank arena for %d-frame chunks of %dx%d needs %zu bytes, %zu free on the device",
                  frames, d->ncols, d->nrows, need, fr);
    // physically contiguous when the driver can (experiment hook KLT_BANK_CONTIG=1)
    if (!(env_size("KLT_BANK_CONTIG", 0) &&
          hipExtMallocWithFlags(&c->banks.arena, need, hipDeviceMallocContiguous) == hipSuccess)) {
      (void)hipGetLastError();
      c->banks.arena = nullptr;
      HIPCHK(c, hipMalloc(&c->banks.arena, need));
    }
    c->banks.arena_bytes = need;
  }
  size_t off = 0;
  auto take = [&](size_t floats) {
    off = (off + kPlaneAlign - 1) / kPlaneAlign * kPlaneAlign;
    float *p = reinterpret_cast<float *>(static_cast<char *>(c->banks.arena) + off);
    off += floats * sizeof(float);
    return p;
  };
  for (auto &K : c->banks.bank) {
    int w = d->ncols, h = d->nrows;
    K.nlev = d->nlevels;
    K.ss = d->nlevels > 1 ? d->subsampling : 1;
    for (int l = 0; l < d->nlevels; ++l) {
      Level &L = K.lv[l];
      L.w = w;
      L.h = h;
      L.cap = bank_plane_floats(d, l, frames);
      if (arena) L.img = take(3 * L.cap);
      L.gx = L.img + L.cap;
      L.gy = L.img + 2 * L.cap;
      w /= K.ss;
      h /= K.ss;
    }
    if (d->nlevels == 2) {
      K.hs_cap = bank_hs_floats(d, frames);
      if (arena) K.hs = take(K.hs_cap);
    }
    K.frames = frames;
  }
  return 0;
}

// fused pyramids of F frames (src + f*stride) into bank K, two launches.
// Level-0 rows [row_lo, row_hi) are built (whole 32-row tiles, global
// coordinates, so every built value is the full-frame value) and the level-1
// tiles whose sigma-3.6 inputs lie inside them; K.holds records what is valid.
// row_lo/row_hi: the level-0 rows to build (the sigma-3.6 rows pass hs over
// all of them); plane_lo/plane_hi: the rows whose level-0 planes are stored
// (a band's outer margin feeds only level 1)
// first / step: frame f goes to pyramid first + f * step of the bank (the
// frame-major banks of klt_hip_track_frames_multi: one sequence's frames are
// nseq pyramids apart); the caller keeps first + (F - 1) * step < K.frames
int build_fused_bank(klt_hip_ctx *c, Bank &K, const klt_hip_pyr_desc *d, const uint8_t *src, long pitch,
                     long stride, int F, hipStream_t st, int row_lo, int row_hi, int plane_lo, int plane_hi,
                     int il, long first, long step) {
  const int W = d->ncols, H = d->nrows;
  const DefTaps T = default_taps(d);
  const bool two = d->nlevels == 2;
  const int W1 = two ? K.lv[1].w : 0, H1 = two ? K.lv[1].h : 0;
  if ((long)W * H == 0 || F <= 0) {
    K.holds(il);
    return 0;
  }
  const int vec_u8 = vec_u8_ok(src, pitch, stride, W);
  const int vec_out = (W % 4 == 0) ? 1 : 0;
  const long fs0 = (long)W * H, fsh = hs_size(W1, H), fs1 = (long)W1 * H1;
  int r0 = clampi(row_lo, 0, H), r1 = row_hi >= H ? H : clampi(row_hi, r0, H);
  int p0 = clampi(plane_lo, 0, H), p1 = plane_hi >= H ? H : clampi(plane_hi, p0, H);
  // il: interleaved (frame f at img + 3 f w h); else planes (frame f at
  // img / gx / gy + f w h), for a batch that a planes-reading tracker takes
  // kLayoutImg: level 0 the img plane alone (frame f at img + f w h), the
  // levels above interleaved
  const int il1 = il == kLayoutImg ? kLayoutRec : il;
  const int np0 = il == kLayoutRec ? 3 : 1, np = il1 ? 3 : 1;
  int lo[KLT_HIP_MAX_LEVELS] = {}, hi[KLT_HIP_MAX_LEVELS];  // valid rows per level: whole frames unless set below
  for (int &v : hi) v = 1 << 30;
  {
    TimedScope ts(c, T_L0, st, F);
    const long o0 = first * np0 * fs0;
    if (launch_l0(c, st, src, pitch, stride, W, H, T, vec_u8, vec_out, K.lv[0].img + o0, K.lv[0].gx + o0,
                  K.lv[0].gy + o0, K.hs + first * fsh, W1, (two && W1 > 0) ? 1 : 0, step * np0 * fs0, step * fsh, F, r0,
                  r1, &p0, &p1, il, c->frame_format))
      return -1;
  }
  lo[0] = p0;
  hi[0] = p1 >= H ? (1 << 30) : p1;
  if (two && (long)W1 * H1 > 0) {
    // level-1 row Y (img1 and its gradients) reads hs rows 4Y-20 .. 4Y+24:
    // it is exact when those lie inside the built level-0 rows (or past an
    // image edge, where the zero rules apply).  The L1 tiles covering the
    // valid rows are launched whole; their rows outside [vlo, vhi) read stale
    // hs rows and are never used (the tracker's band test stops at vlo/vhi).
    const int TH1 = geom::L1_TH;
    const int nt1 = (H1 + TH1 - 1) / TH1;
    const int ylo = r0 == 0 ? 0 : (r0 + 20 + 3) / 4;
    const int yhi = r1 >= H ? H1 : (r1 >= 25 ? (r1 - 25) / 4 + 1 : 0);
    lo[1] = ylo;
    hi[1] = yhi >= H1 ? (1 << 30) : yhi;
    if (yhi > ylo) {
      const int t1lo = ylo / TH1, t1hi = clampi((yhi + TH1 - 1) / TH1, t1lo, nt1);
      HMARK_IN("l0_launched");
      TimedScope ts(c, T_L1, st, F);
      const int vec = (W1 % 4 == 0 && W1 >= 8) ? 1 : 0;
      const long o1 = first * np * fs1;
      if (launched(c, "k_pyr_l1", launch_pyr_l1(st, K.hs + first * fsh, W1, H, H1, T, vec, K.lv[1].img + o1,
                                                K.lv[1].gx + o1, K.lv[1].gy + o1, step * fsh, step * np * fs1, F, t1lo,
                                                t1hi, il1)))
        return -1;
      HMARK_IN("l1_launched");
    }
  }
  K.holds(il, lo, hi);
  return 0;
}

KLT_API int klt_hip_build_pyramid(klt_hip_ctx *c, int s, const klt_hip_pyr_desc *d,
                                  const unsigned char *frame, long pitch, int buf) {
  if (!c) return fail(c, "build_pyramid: null context");
  if (s < 0 || s >= KLT_HIP_MAX_SLOTS) return fail(c, "build_pyramid: bad slot %d", s);
  return build_pyramid_on(c, s, d, frame, pitch, buf, c->stream);
}

int build_pyramid_on(klt_hip_ctx *c, int s, const klt_hip_pyr_desc *d, const unsigned char *frame,
                            long pitch, int buf, hipStream_t st) {
  if (!c || !d) return fail(c, "build_pyramid: null argument");
  if (s < 0 || s >= KLT_HIP_MAX_SLOTS + 2) return fail(c, "build_pyramid: bad slot %d", s);
  if (d->nlevels < 1 || d->nlevels > KLT_HIP_MAX_LEVELS) return fail(c, "bad nlevels %d", d->nlevels);
  if (d->nlevels > 1 && d->subsampling < 2) return fail(c, "bad subsampling %d", d->subsampling);
  for (const klt_hip_taps *t : {&d->smooth, &d->pyr, &d->grad_gauss, &d->grad_deriv})
    if (t->width < 0 || t->width > KLT_HIP_MAX_TAPS || (t->width % 2) != 1)
      if (!(t == &d->pyr && d->nlevels == 1) && !(t == &d->smooth && !d->smooth_input))
        return fail(c, "build_pyramid: bad tap width %d", t->width);
  if (use_device(c)) return -1;
  const uint8_t *src = frame;
  if (!src) {
    if (buf < 0 || buf > 1 || !c->d_u8[buf]) return fail(c, "build_pyramid: no uploaded frame");
    if (c->u8_w[buf] != d->ncols || c->u8_h[buf] != d->nrows)
      return fail(c, "build_pyramid: uploaded frame is %dx%d, desc %dx%d", c->u8_w[buf], c->u8_h[buf],
                  d->ncols, d->nrows);
    src = c->d_u8[buf];
    pitch = d->ncols;
  }
  // a caller's device frame holds the context's pixels; a staging buffer is gray
  const int fmt = frame ? c->frame_format : KLT_HIP_FRAME_GRAY8;
  if (pitch < (long)d->ncols * frame_bpp(fmt))
    return fail(c, "build_pyramid: pitch %ld < ncols %d * %d bytes per pixel", pitch, d->ncols, frame_bpp(fmt));
  if (ensure_slot(c, s, d)) return -1;
  const bool fz = fused_ok(d) && !c->force_generic;
  c->slot[s].fused = fz ? 1 : 0;
  return fz ? build_fused(c, s, d, src, pitch, st, fmt) : build_generic(c, s, d, src, pitch, st, fmt);
}

KLT_API int klt_hip_fused_path(klt_hip_ctx *c, const klt_hip_pyr_desc *d) {
  if (!c || !d) return fail(c, "fused_path: null argument");
  return fused_ok(d) && !c->force_generic ? 1 : 0;
}

KLT_API int klt_hip_pyramid_path(klt_hip_ctx *c, int s) {
  if (!c || s < 0 || s >= KLT_HIP_MAX_SLOTS) return -1;
  return c->slot[s].fused;
}

KLT_API int klt_hip_level_dims(klt_hip_ctx *c, int s, int l, int *w, int *h) {
  if (!c || s < 0 || s >= KLT_HIP_MAX_SLOTS || l < 0 || l >= c->slot[s].nlev) return fail(c, "bad slot/level");
  *w = c->slot[s].lv[l].w;
  *h = c->slot[s].lv[l].h;
  return 0;
}

KLT_API const float *klt_hip_level_ptr(klt_hip_ctx *c, int s, int l, int which) {
  if (!c || s < 0 || s >= KLT_HIP_MAX_SLOTS || l < 0 || l >= c->slot[s].nlev) return nullptr;
  const Level &L = c->slot[s].lv[l];
  if (L.il) return which == 0 ? L.img : nullptr;  // interleaved: the level's base
  return which == 0 ? L.img : (which == 1 ? L.gx : L.gy);
}

KLT_API int klt_hip_level_interleaved(klt_hip_ctx *c, int s, int l) {
  if (!c || s < 0 || s >= KLT_HIP_MAX_SLOTS || l < 0 || l >= c->slot[s].nlev) return -1;
  return c->slot[s].lv[l].il;
}

KLT_API int klt_hip_download_level(klt_hip_ctx *c, int s, int l, int which, float *host) {
  if (!c || s < 0 || s >= KLT_HIP_MAX_SLOTS || l < 0 || l >= c->slot[s].nlev || which < 0 || which > 2)
    return fail(c, "download_level: bad slot/level");
  if (use_device(c)) return -1;
  const Level &L = c->slot[s].lv[l];
  const long n = (long)L.w * L.h;
  const float *p = which == 0 ? L.img : (which == 1 ? L.gx : L.gy);
  if (L.il && n > 0) {  // the plane out of the interleaved level first
    if (grow(c, &c->d_tmp[0], &c->tmp_cap[0], (size_t)(3 * n))) return -1;
    float *t = c->d_tmp[0];
    if (launched(c, "k_from_il", launch_from_il(c->stream, L.img, t, t + n, t + 2 * n, n))) return -1;
    p = t + which * n;
  }
  HIPCHK(c, hipMemcpyAsync(host, p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// pixel formats of device frames (klt_hip.h, "Pixel format of DEVICE frames")
// ---------------------------------------------------------------------------
KLT_API int klt_hip_frame_bpp(int format) { return frame_bpp(format); }

KLT_API int klt_hip_set_frame_format(klt_hip_ctx *c, int format) {
  if (!c) return -1;
  if (frame_bpp(format) < 0)
    return fail(c, "set_frame_format: unknown format %d (KLT_HIP_FRAME_GRAY8 .. KLT_HIP_FRAME_BGRA8)", format);
  c->frame_format = format;
  return 0;
}

KLT_API int klt_hip_get_frame_format(klt_hip_ctx *c) { return c ? c->frame_format : -1; }

KLT_API int klt_hip_gray_host(int format, const unsigned char *src, long pitch, int ncols, int nrows,
                              unsigned char *dst, long dst_pitch) {
  const int bpp = frame_bpp(format);
  if (bpp < 0 || !src || !dst || ncols < 0 || nrows < 0 || pitch < (long)ncols * bpp || dst_pitch < ncols) return -1;
  const bool bgr = frame_bgr(format);
  for (int y = 0; y < nrows; ++y) {
    const unsigned char *s = src + (long)y * pitch;
    unsigned char *o = dst + (long)y * dst_pitch;
    if (bpp == 1) {
      memmove(o, s, (size_t)ncols);
      continue;
    }
    for (int x = 0; x < ncols; ++x, s += bpp) o[x] = (unsigned char)gray_of(s[0], s[1], s[2], bgr);
  }
  return 0;
}

KLT_API int klt_hip_to_gray(klt_hip_ctx *c, int format, const unsigned char *dev_src, long pitch, long stride,
                            int nframes, int ncols, int nrows, unsigned char *dev_dst, long dst_pitch,
                            long dst_stride) {
  if (!c) return fail(c, "to_gray: null context");
  const int bpp = frame_bpp(format);
  if (bpp < 0) return fail(c, "to_gray: unknown format %d", format);
  if (nframes < 0 || ncols < 0 || nrows < 0) return fail(c, "to_gray: bad nframes/ncols/nrows");
  if (nframes == 0 || (long)ncols * nrows == 0) return 0;
  if (!dev_src || !dev_dst) return fail(c, "to_gray: null frames");
  if (pitch < (long)ncols * bpp)
    return fail(c, "to_gray: pitch %ld < ncols %d * %d bytes per pixel", pitch, ncols, bpp);
  if (dst_pitch < ncols) return fail(c, "to_gray: dst_pitch %ld < ncols %d", dst_pitch, ncols);
  if (use_device(c)) return -1;
  return launched(c, "k_to_gray", launch_to_gray(c->stream, format, dev_src, pitch, stride, nframes, ncols, nrows,
                                                 dev_dst, dst_pitch, dst_stride));
}
