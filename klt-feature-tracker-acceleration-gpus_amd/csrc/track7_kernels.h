// track7_kernels.h -- the Lucas-Kanade Newton loop for the default configuration
// (7x7 window, exact ordered sums, no gain/bias normalisation), written for
// the length of one feature's dependent chain: the kernel templates and all
// their device code.  Three units include it and instantiate what they launch,
// each a code object of its own: track7.hip (k_track7, _hook, _fb, _multi),
// track7_pred.hip (k_track7_pred), track7_mask.hip (k_track7_mask, _mask_lazy).
//
// Same algorithm and results as k_track_frames_g in track.hip, which serves
// every other configuration: _trackFeature (trackFeatures.c:381-486) inside
// the coarse-to-fine level loop of KLTTrackFeatures (:1343-1437), one wave64
// per feature carried through a batch of frames, the finest level's residue
// deferred into the next frame's first pass.  What differs is the shape of
// the code on the chain that one wave walks for each Newton pass:
//   * lane p < 49 owns window pixel p (row-major, the reference's order) and
//     gathers its four bilinear corners itself: from a level stored
//     interleaved ({gx, gy, img} per pixel, as the fused pyramid kernels
//     write it) one 24-byte run per row for all three planes, from planes
//     two 8-byte loads per plane:
//     no lane shuffles and no patch-fit test, so there is no fallback path;
//     every load of a pass (img2's three planes, img1's on a level's first
//     pass, the deferred residue's img2 plane) is issued before any is used;
//   * per-feature state is wave-uniform and kept in scalar registers
//     (readfirstlane where a value is produced), so every test is one scalar
//     branch and nothing is re-derived per pass;
//   * the five (or six) ordered sums go through LDS once per pass: each lane
//     writes its products, lane s reads row s with all thirteen 16-byte reads
//     in flight and adds them in pixel order -- the reference's sequential
//     float sum, started from +0 (the rows' pads past pixel 48 stay +0);
//   * the 2x2 solve runs on two lanes (track7_solve.h): the sums stay in the
//     lanes that added them, lane 0 divides for dx and lane 1 for dy with one
//     instruction stream, and the position is kept in those two lanes.
// Parity: -ffp-contract=off, IEEE division, every expression in the
// reference's evaluation order.
#pragma once
#pragma clang fp contract(off)
// the level loops carry #pragma unroll for the two-level instances; the
// runtime-depth ones (NL == 0) cannot unroll them, which is expected
#pragma clang diagnostic ignored "-Wpass-failed"

#include <math.h>

#include "klt_dev.h"

#ifndef KLT_T7_REUSE
#define KLT_T7_REUSE 1  // a pass whose window corners are the previous pass's takes them from registers
#endif
#ifndef KLT_T7_BATCH
#define KLT_T7_BATCH 7  // 16-byte LDS reads in flight per ordered-sum batch (13 per row)
#endif

namespace kltdev {
namespace {

constexpr int kWin = 7, kHw = 3, kNpx = kWin * kWin;  // 49 window pixels
constexpr int kRow = 52;                                 // LDS row of one sum: 13 chunks of 4 (pads 49..51 = +0)
constexpr int kRows = 6;                                 // 5 Newton sums + the deferred residue
constexpr int kWaves = kBlock / kWave;

__device__ __forceinline__ float u(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ int u(int v) { return __builtin_amdgcn_readfirstlane(v); }

#include "track7_solve.h"  // KLT_T7_SOLVE2: the solve on two lanes

// window bounds test (trackFeatures.c:421-427 / :460-462, one_plus_eps 1.001):
//   x - 3 < 0 || w - (x + 3) < 1.001 || (the same for y and h)
// in float arithmetic.  x - 3 < 0 exactly when x < 3, and w - (x + 3) never
// grows with x, so the second test holds exactly from one float on (tx, found
// on the host by bisection with the same float operations); IEEE order of
// non-negative floats is the order of their bit patterns, and a negative
// float's pattern is a negative int.  So the test is four integer compares
// of wave-uniform values -- scalar instructions, no VALU round trip --
// that also send infinities and NaNs out (the reference would fault on them)
constexpr int kThreeBits = 0x40400000;  // 3.0f

__device__ __forceinline__ bool out7(float x, float y, int tx, int ty) {
  const int xb = __float_as_int(x), yb = __float_as_int(y);
  return xb < kThreeBits || xb >= tx || yb < kThreeBits || yb >= ty;
}

// _interpolate (trackFeatures.c:31-57) for this lane's pixel: corner offset and weights
struct Pix {
  unsigned off;  // byte offset of the top-left corner in a plane
  unsigned px;   // its pixel index
  float w0, w1, w2, w3;
};

// Every caller gathers at a position that passed out7 (this pass's, the
// level's x1, the previous frame's final one for the deferred residue), so
// x + i lies in [0, w - 2.001) for every window column i and (int) needs no
// clamp: the four corners are inside the level.
__device__ __forceinline__ Pix pix_at(int w, int h, float x, float y) {
  const int xt = (int)x, yt = (int)y;
  const float ax = x - xt, ay = y - yt;
  Pix p;
  p.px = (unsigned)(yt * w + xt);
  p.off = p.px * 4u;
  p.w0 = (1.0f - ax) * (1.0f - ay);
  p.w1 = ax * (1.0f - ay);
  p.w2 = (1.0f - ax) * ay;
  p.w3 = ax * ay;
  return p;
}

struct Quad {
  float2 r0, r1;
};

// uniform plane base + 32-bit per-lane byte offsets: scalar-base addressing
__device__ __forceinline__ Quad quad(const float *P, const Pix &p, unsigned rowb) {
  const char *b = reinterpret_cast<const char *>(P);
  const unsigned o1 = p.off + rowb;
  Quad q;
  q.r0 = *reinterpret_cast<const float2 *>(b + p.off);
  q.r1 = *reinterpret_cast<const float2 *>(b + o1);
  return q;
}

// interleaved levels ({gx, gy, img} per pixel, 12 bytes): one 24-byte run per
// row holds both corners of all three planes
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
struct Tri {
  Quad i, x, y;
};
__device__ __forceinline__ Tri tri(const float *P, const Pix &p, unsigned rowb) {
  // uniform base + 32-bit lane offsets for both rows (scalar-base addressing)
  const char *base = reinterpret_cast<const char *>(P);
  const unsigned o0 = p.px * 12u, o1 = o0 + rowb;
  const f4u a0 = *reinterpret_cast<const f4u *>(base + o0), b0 = *reinterpret_cast<const f4u *>(base + o1);
  const f2u a1 = *reinterpret_cast<const f2u *>(base + o0 + 16), b1 = *reinterpret_cast<const f2u *>(base + o1 + 16);
  // records {gx, gy, img} (klt_dev.h): a0 = gx0 gy0 img0 gx1, a1 = gy1 img1
  static_assert(kRecGx == 0 && kRecGy == 1 && kRecImg == 2, "record layout");
  Tri t;
  t.i.r0 = make_float2(a0.z, a1.y);
  t.i.r1 = make_float2(b0.z, b1.y);
  t.x.r0 = make_float2(a0.x, a0.w);
  t.x.r1 = make_float2(b0.x, b0.w);
  t.y.r0 = make_float2(a0.y, a1.x);
  t.y.r1 = make_float2(b0.y, b1.x);
  return t;
}
// img alone from an interleaved level
__device__ __forceinline__ Quad quad_i(const float *P, const Pix &p, unsigned rowb) {
  const unsigned o0 = p.px * 12u, o1 = o0 + rowb;
  const float *b = reinterpret_cast<const float *>(reinterpret_cast<const char *>(P) + o0);
  const float *c = reinterpret_cast<const float *>(reinterpret_cast<const char *>(P) + o1);
  Quad q;
  q.r0 = make_float2(b[kRecImg], b[kRec + kRecImg]);
  q.r1 = make_float2(c[kRecImg], c[kRec + kRecImg]);
  return q;
}

// (1-ax)(1-ay)p00 + ax(1-ay)p01 + (1-ax)ay p10 + ax ay p11, left to right
__device__ __forceinline__ float interp(const Pix &p, const Quad &q) {
  return p.w0 * q.r0.x + p.w1 * q.r0.y + p.w2 * q.r1.x + p.w3 * q.r1.y;
}

// The ordered sums hand values between the lanes of one wave through LDS.
// A wave's LDS operations are performed in order, so a read issued after a
// write sees it: wavefront-scope fences only keep the compiler from moving
// the accesses across (no s_waitcnt lgkmcnt(0) between the writes and the
// reads, as workgroup scope would emit).  KLT_T7_WAVEFENCE=0 restores those.
#ifndef KLT_T7_WAVEFENCE
#define KLT_T7_WAVEFENCE 1
#endif
__device__ __forceinline__ void wave_lds_sync() {
#if KLT_T7_WAVEFENCE
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#else
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

typedef float f4 __attribute__((ext_vector_type(4)));

// NS ordered sums: lane p (< 49) contributes v[s] as pixel p of sum s; returns
// the sums, wave-uniform.  The reference's sequential float sums (:241-248,
// :271-278, :354-367), each from +0 in pixel order.
// PIN (the lazy-gradient instances, which run at their scalar register limit):
// the test lane < NS is made anew from a lane number the compiler cannot see
// through, one compare.  Left to itself it keeps the three masks (NS 1, 5, 6)
// as frame-loop invariants in scalar pairs, spills them and reads them back
// lane by lane in every pass.
// sums7_acc leaves sum s in lane s (the two-lane solve takes them there).
template <int NS, bool PIN = false>
__device__ __forceinline__ float sums7_acc(float *red, int lane, bool on, const float (&v)[NS]) {
  if (on) {
#pragma unroll
    for (int s = 0; s < NS; ++s) red[s * kRow + lane] = v[s];
  }
  wave_lds_sync();
  float acc = 0.0f;
  if constexpr (PIN) asm volatile("" : "+v"(lane));
  if (lane < NS) {
    const float *r = red + lane * kRow;
    constexpr int NCH = kRow / 4, B = KLT_T7_BATCH;
#pragma unroll
    for (int k0 = 0; k0 < NCH; k0 += B) {
      f4 c[B];
#pragma unroll
      for (int k = 0; k < B; ++k)
        if (k0 + k < NCH) c[k] = *reinterpret_cast<const f4 *>(r + 4 * (k0 + k));
#pragma unroll
      for (int k = 0; k < B; ++k) {
        const int q = 4 * (k0 + k);
        if (k0 + k >= NCH) break;
        acc += c[k].x;
        if (q + 1 < kNpx) acc += c[k].y;
        if (q + 2 < kNpx) acc += c[k].z;
        if (q + 3 < kNpx) acc += c[k].w;
      }
    }
  }
  wave_lds_sync();  // the rows are rewritten by the next pass
  return acc;
}
template <int NS, bool PIN = false>
__device__ __forceinline__ void sums7(float *red, int lane, bool on, const float (&v)[NS], float (&out)[NS]) {
  const float acc = sums7_acc<NS, PIN>(red, lane, on, v);
#pragma unroll
  for (int s = 0; s < NS; ++s) out[s] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc), s));
}

// KLT_HIP_FAST (not bit-exact; the tolerance is tests/test_gpu_long.py's):
// the NS sums by DPP within the VALU -- two quad butterflies and two row
// rotations leave every lane of a 16-lane row its row's sum, then the four
// row sums are read out and added -- no LDS round trip and no 49-add chain
constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kRowRor4 = 0x124, kRowRor8 = 0x128;  // DPP controls
constexpr int kRowBcast15 = 0x142, kRowBcast31 = 0x143;                                // GFX9 DPP broadcasts
#ifndef KLT_T7_BCAST
#define KLT_T7_BCAST 1  // the fast sums' row totals combined by DPP broadcasts (A/B hook: 0 reads four lanes)
#endif
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x) {
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}

template <int NS>
__device__ __forceinline__ void tree7(bool on, const float (&v)[NS], float (&out)[NS]) {
  float x[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) x[s] = on ? v[s] : 0.0f;
#pragma unroll
  for (int s = 0; s < NS; ++s) x[s] = dpp_add<kQuadXor1>(x[s]);
#pragma unroll
  for (int s = 0; s < NS; ++s) x[s] = dpp_add<kQuadXor2>(x[s]);
#pragma unroll
  for (int s = 0; s < NS; ++s) x[s] = dpp_add<kRowRor4>(x[s]);
#pragma unroll
  for (int s = 0; s < NS; ++s) x[s] = dpp_add<kRowRor8>(x[s]);
#if KLT_T7_BCAST
  // the four row sums r0..r3 combined in the VALU: row_bcast:15 adds row 0's
  // sum into row 1 and row 2's into row 3, row_bcast:31 then row 1's
  // (r0 + r1) into row 3, so lane 63 holds (r2 + r3) + (r0 + r1) -- the same
  // float as (r0 + r1) + (r2 + r3), addition being commutative -- and one
  // readlane per sum leaves the VALU instead of four.  Every row is enabled
  // (bound_ctrl: a lane without a source adds +0) so that each step is one
  // v_add_f32_dpp; the other rows' values are not read
#pragma unroll
  for (int s = 0; s < NS; ++s) x[s] = x[s] + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x[s]),
                                                                                          kRowBcast15, 0xF, 0xF, true));
#pragma unroll
  for (int s = 0; s < NS; ++s) x[s] = x[s] + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x[s]),
                                                                                          kRowBcast31, 0xF, 0xF, true));
#pragma unroll
  for (int s = 0; s < NS; ++s) out[s] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[s]), 63));
#else
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int b = __float_as_int(x[s]);
    out[s] = (__int_as_float(__builtin_amdgcn_readlane(b, 0)) + __int_as_float(__builtin_amdgcn_readlane(b, 16))) +
             (__int_as_float(__builtin_amdgcn_readlane(b, 32)) + __int_as_float(__builtin_amdgcn_readlane(b, 48)));
  }
#endif
}

template <int NS, bool FAST, bool PIN = false>
__device__ __forceinline__ void sums(float *red, int lane, bool on, const float (&v)[NS], float (&out)[NS]) {
  if constexpr (FAST) tree7<NS>(on, v, out);
  else sums7<NS, PIN>(red, lane, on, v, out);
}

// ---------------------------------------------------------------------------
// Lazy level-0 gradients (klt_hip_set_lazy_grad): the level is the img plane
// alone and the wave computes gx / gy of the pixels its window touches, bit
// for bit as the pyramid kernels do (pyramid.hip k_rows / k_cols and
// pyr_l0_tile): tx = rows_d(img), ty = rows_g(img), gx = cols_g(tx),
// gy = cols_d(ty), every sum from +0 over all seven taps in tap order, one
// rounding per operation, and +0 within kHw pixels of a frame edge (the
// passes' zero borders; every other pixel reads only in-frame values).
//
// A window at (x, y) has lane p's top-left corner at ((int)(x + i), (int)(y + j)),
// i, j in -3..3.  With X0 = (int)(x - 3) (exact: x >= 3) that is X0 + i + 3, or
// one more when the float sum x + i rounds up to the next integer -- and then
// the lane's fraction is exactly 0, so its right-hand corners carry weight +0.
// So the corners with a non-zero weight lie in the 8 x 8 block from (X0, Y0),
// whose gradients read tx / ty on 14 rows x 8 columns, which read the 14 x 14
// img block from (X0 - 3, Y0 - 3).  A corner index past the block (weight +0
// only) is clamped into it: the product is a zero either way, and a zero's
// sign changes no ordered sum, which start from +0, nor the residue's |.|.
//
// Per wave in LDS, one patch at a time: S, the img block (16 rows of pitch kPS,
// two spare rows and columns loaded like the rest from clamped addresses); T,
// {tx, ty} of 16 x 8; G, {gx, gy} of 8 x 8, over S once the rows pass has read
// it (the lane's img corners are taken from S before).  Hand-offs are
// wave-scope (wave_lds_sync).  2.5 KB per wave keeps a workgroup at 15 KB, so
// that pyramid workgroups of an overlapped build still fit beside five
// tracker workgroups per CU.
// ---------------------------------------------------------------------------
constexpr int kPS = 24;                                   // S pitch: the rows pass's 32-lane groups hit distinct banks
constexpr int kPatS = 16 * kPS, kPatT = 2 * 16 * 8, kPatG = 2 * 8 * 8;
constexpr int kPat = kPatS + kPatT;                       // floats per wave (640)
static_assert(kPatG <= kPatS, "G over S");
constexpr int kRedF = kRows * kRow + 4;                   // floats of a wave's ordered-sum rows

typedef float f2 __attribute__((ext_vector_type(2)));

// this lane's four pixels of the staged block, rows sr + 4k of column sc; all
// four loads are issued here, clamped into the frame
__device__ __forceinline__ void patch_load(const float *img, int w, int h, int X0, int Y0, int lane, float (&v)[4]) {
  const int sc = lane & 15, sr = 2 * ((lane >> 4) & 1) + (lane >> 5);
  const unsigned xc = (unsigned)clampi(X0 - kHw + sc, 0, w - 1);
  const char *b = reinterpret_cast<const char *>(img);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned yc = (unsigned)clampi(Y0 - kHw + sr + 4 * k, 0, h - 1);
    v[k] = *reinterpret_cast<const float *>(b + (yc * (unsigned)w + xc) * 4u);
  }
}

// One patch: v the lane's staged pixels (patch_load), cx / cy this lane's
// corner column and row in the 8 x 8 block (0..7).  Out: the lane's corners of
// img, gx, gy.
__device__ __forceinline__ void patch_grads(float *pat, int lane, const TrkArgs &a, int w, int h, const float (&v)[4],
                                            int X0, int Y0, int cx, int cy, Quad &qi, Quad &qx, Quad &qy) {
  const int sc = lane & 15, sr = 2 * ((lane >> 4) & 1) + (lane >> 5);
#pragma unroll
  for (int k = 0; k < 4; ++k) pat[(sr + 4 * k) * kPS + sc] = v[k];
  wave_lds_sync();
  {
    const float *S = pat + (cy + kHw) * kPS + cx + kHw;  // the block's 14 columns hold cx + 1 <= 8
    qi.r0 = make_float2(S[0], S[1]);
    qi.r1 = make_float2(S[kPS], S[kPS + 1]);
  }
  // rows pass: {tx, ty} of block rows r and r + 8 (rows 14 and 15 are spare), column c = pixel X0 + c.
  // Both passes multiply by the same seven scalar pairs {gd[m], gg[m]}: tx takes
  // gd here and gg in the columns pass, ty the other way round, so T holds each
  // pair exchanged, {ty, tx} (two 4-byte stores from either register, one LDS
  // instruction), and the columns pass forms {gy, gx}.  With {gg[m], gd[m]} for
  // the columns as well, the packed multiplies' aligned scalar pairs took 28
  // registers, most of them spilled and read back lane by lane in every patch.
  const int c = lane & 7, r = lane >> 3;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float *row = pat + (r + 8 * k) * kPS + c;
    f2 t = {0.0f, 0.0f};
#pragma unroll
    for (int m = 0; m < 7; ++m) t += f2{row[m], row[m]} * f2{a.gd[m], a.gg[m]};
    float *T = pat + kPatS + 2 * ((r + 8 * k) * 8 + c);
    T[0] = t.y;
    T[1] = t.x;
  }
  wave_lds_sync();
  // columns pass: {gy, gx} of pixel (X0 + c, Y0 + r) from T rows r .. r + 6; G goes over S
  {
    const float *col = pat + kPatS + 2 * (r * 8 + c);
    f2 g = {0.0f, 0.0f};
#pragma unroll
    for (int m = 0; m < 7; ++m) g += *reinterpret_cast<const f2 *>(col + 16 * m) * f2{a.gd[m], a.gg[m]};
    const int x = X0 + c, y = Y0 + r;
    if (x < kHw || x + kHw >= w || y < kHw || y + kHw >= h) g = f2{0.0f, 0.0f};  // w and h as they are: no w - 3, h - 3 to keep
    *reinterpret_cast<f2 *>(pat + 2 * (r * 8 + c)) = g;
  }
  wave_lds_sync();
  const int cx1 = min(cx + 1, 7), cy1 = min(cy + 1, 7);
  const f2 g00 = *reinterpret_cast<const f2 *>(pat + 2 * (cy * 8 + cx));
  const f2 g01 = *reinterpret_cast<const f2 *>(pat + 2 * (cy * 8 + cx1));
  const f2 g10 = *reinterpret_cast<const f2 *>(pat + 2 * (cy1 * 8 + cx));
  const f2 g11 = *reinterpret_cast<const f2 *>(pat + 2 * (cy1 * 8 + cx1));
  qx.r0 = make_float2(g00.y, g01.y);
  qx.r1 = make_float2(g10.y, g11.y);
  qy.r0 = make_float2(g00.x, g01.x);
  qy.r1 = make_float2(g10.x, g11.x);
  wave_lds_sync();  // the patch area is rewritten by the next patch
}

// The last level-0 pass's image-2 corners of a frame, kept for the next frame
// (lazy-gradient instances): frame j's image 2 is frame j + 1's image 1, and
// frame j + 1 starts where frame j ended, mostly in the same cell -- its
// image-1 corners are then these, and no image-1 patch is computed.  px: the
// corners' pixel per lane, ~0u when nothing is kept.
struct Carry {
  unsigned px = ~0u;
  Quad i, x, y;
};
#ifndef KLT_T7_CARRY
#define KLT_T7_CARRY 1  // A/B hook: 0 computes every first pass's image-1 patch
#endif

struct Lev {
  const float *img, *gx, *gy;
  int w, h, vlo, vhi;
  int tx, ty;  // out7's thresholds for this level's size (TrkArgs::oobx / ooby)
  int il;      // the level's layout (klt_dev.h kLayout*); read by the lazy-gradient instances only
};

__device__ __forceinline__ Lev lev_of(const TrkLevel &L, long off, int tx, int ty) {
  return Lev{L.img + off, L.gx + off, L.gy + off, L.w, L.h, L.vlo, L.vhi, tx, ty, L.il};
}

// image 1 of frame j at level r: the previous pyramid (a.A) for the batch's
// first frame, else bank frame j-1.  Selected field by field so that both
// structs' fields stay loop-invariant scalars (a select of the struct's
// address would load them through a pointer on every frame)
__device__ __forceinline__ Lev lev_prev(const TrkArgs &a, const TrkFramesArgs &b, int r, int j) {
  const TrkLevel &P = a.A[r], &Q = a.B[r];
  const bool f = j == 0;
  const long off = f ? 0L : (long)(j - 1) * b.lfs[r];
  return Lev{(f ? P.img : Q.img) + off, (f ? P.gx : Q.gx) + off, (f ? P.gy : Q.gy) + off, f ? P.w : Q.w,
             f ? P.h : Q.h, f ? P.vlo : Q.vlo, f ? P.vhi : Q.vhi, a.oobx[r], a.ooby[r], f ? P.il : Q.il};
}

// The two images of frame j at level r.  MULTI (k_track7_multi): the launch
// carries nsq sequences through frame-major banks, the wave's feature belongs
// to sequence sq (wave-uniform, scalar): image 2 is pyramid j * nsq + sq of
// a.B, image 1 pyramid (j - 1) * nsq + sq of it or, for the launch's first
// frame, pyramid sq of a.A (a group laid out like a bank's: same level sizes,
// layout and pyramid stride).  Offsets in 64 bits.  Otherwise lev_of / lev_prev
// as they stand.
template <bool MULTI>
__device__ __forceinline__ Lev lev_cur(const TrkArgs &a, const TrkFramesArgs &b, int r, int j, int sq, int nsq) {
  if constexpr (MULTI) return lev_of(a.B[r], ((long)j * nsq + sq) * b.lfs[r], a.oobx[r], a.ooby[r]);
  else return lev_of(a.B[r], (long)j * b.lfs[r], a.oobx[r], a.ooby[r]);
}
template <bool MULTI>
__device__ __forceinline__ Lev lev_before(const TrkArgs &a, const TrkFramesArgs &b, int r, int j, int sq, int nsq) {
  if constexpr (MULTI) {
    const TrkLevel &P = a.A[r], &Q = a.B[r];
    const bool f = j == 0;
    const long off = (f ? (long)sq : (long)(j - 1) * nsq + sq) * b.lfs[r];
    return Lev{(f ? P.img : Q.img) + off, nullptr, nullptr, Q.w, Q.h, Q.vlo, Q.vhi, a.oobx[r], a.ooby[r], Q.il};
  } else {
    return lev_prev(a, b, r, j);
  }
}

// ROLL (track7_body.h): image 1's base and level-0 layout come with the
// caller, the level's size is image 2's (launch_track7 refuses a kept pyramid
// of another size)
template <bool MULTI, bool ROLL>
__device__ __forceinline__ Lev lev_img1(const TrkArgs &a, const TrkFramesArgs &b, int r, int j, int sq, int nsq,
                                        const float *pimg, int pil) {
  if constexpr (ROLL) {
    const TrkLevel &Q = a.B[r];
    return Lev{pimg, nullptr, nullptr, Q.w, Q.h, Q.vlo, Q.vhi, a.oobx[r], a.ooby[r], pil};
  } else {
    return lev_before<MULTI>(a, b, r, j, sq, nsq);
  }
}

// band-built pyramids (klt_hip_track_frames_band): every row the window's
// bilinear samples touch must have been built
__device__ __forceinline__ bool band_bad(const Lev &L, float y) {
  return (int)(y - kHw) < L.vlo || (int)(y + kHw) + 1 >= L.vhi;
}

// the deferred residue of the previous frame (finest level, final position)
struct Pending {
  bool on = false;
  float x2 = 0.0f, y2 = 0.0f;
  int it = 0;
  float aim = 0.0f;  // this lane's img1 sample of that frame's finest level
};

struct Counts {
  unsigned solves = 0, passes = 0;
#ifdef KLT_TRACK_PROF
  unsigned long long c[kProfN] = {};  // instrumented build: per-wave phase cycles (track.hip's layout)
#endif
};

// The HOOK instances: every way out of the kernel body (track7_body.h) passes
// wave_exit once per wave, and its entry wave_time(.., 0) -- the optional
// times and the optional count of the waves that have left (TrkFramesArgs::
// wave_t / ::exits).  The count is a scheduling hint: nothing in the kernel
// waits for it, and the one store to signal memory (read by the command
// processor, hipStreamWaitValue32) is relaxed at system scope.  The times
// take no place in a list by counting: 5024 adds to one word, serialised
// between the XCDs, held every wave of a launch back -- by up to 220 us when
// each wave waited for its place, lost features included, and still by 55 us
// without a result.  A wave's entry time goes to its number in the grid, its
// exit time to a number it has at hand when it leaves, so that the kernel
// body keeps nothing alive for the hook: its feature's index, or its slot
// when that holds no feature (slots past n: no feature has that index).  A
// band launch's waves past their XCD's run leave under their number in the
// grid, which a feature may share.
constexpr int kWaveXcdShift = 60;
constexpr unsigned long long kWaveTimeMask = (1ull << kWaveXcdShift) - 1ull;
__device__ __forceinline__ void wave_time(unsigned long long *wave_t, int which, unsigned k) {
  const unsigned long long t = wall_clock64(), cap = wave_t[2];
  // the wave's XCD (XCC_ID, as pyramid.hip's PYR_END reads it) rides in the top four bits of its times
  const unsigned long long xcd = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u;
  if (k < cap) wave_t[4 + which * cap + k] = (t & kWaveTimeMask) | (xcd << kWaveXcdShift);
}
// What a wave needs only as it leaves -- the list's pointers, the work
// counters, the hook's -- the lazy-gradient instances read from the kernel's
// argument segment there (track7_body.h's LATE) and not from the by-value
// arguments, which are loaded at the kernel's entry and would be held in scalar
// registers, or spilled and reloaded, all through the frame loop.  T7KArgs is
// the explicit arguments of k_track7 / k_track7_hook as the segment holds them:
// in order, each at its natural alignment.
struct T7KArgs {
  TrkArgs a;
  TrkFramesArgs b;
  float *fx, *fy;
  int *fv;
  int n;
};
typedef const __attribute__((address_space(4))) T7KArgs *T7KArgsPtr;
__device__ __forceinline__ T7KArgsPtr t7_kargs() {
  return (T7KArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
}
// the lazy-gradient mask instances (k_track7_mask_lazy): T7KArgs first, so that
// everything above reads them as it reads the others, the mask after it
struct T7MaskKArgs {
  T7KArgs k;
  TrkMaskArgs mk;
};
typedef const __attribute__((address_space(4))) T7MaskKArgs *T7MaskKArgsPtr;
__device__ __forceinline__ T7MaskKArgsPtr t7_mask_kargs() {
  return (T7MaskKArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
}
// the hook's way out (the HOOK instances are lazy-gradient ones)
__device__ __forceinline__ void wave_exit(int lane, unsigned k) {
  if (lane != 0) return;
  const T7KArgsPtr ka = t7_kargs();
  unsigned long long *const wave_t = ka->b.wave_t;
  unsigned *const exits = ka->b.exits;
  if (wave_t) wave_time(wave_t, 1, k);
  if (exits) {
    const unsigned k = atomicAdd(exits, 1u) + 1u;
    if (k == ka->b.exit_thr) __hip_atomic_store(ka->b.exit_sig, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

#ifdef KLT_TRACK_PROF
#define T7_T(t) const unsigned long long t = clock64()
#define T7_ADD(k, t0) cnt.c[k] += clock64() - (t0)
#else
#define T7_T(t)
#define T7_ADD(k, t0)
#endif

// Level state shared by the passes of one _trackFeature call.
struct LevState {
  float x2, y2;              // current position (wave-uniform)
  float pxy;                 // KLT_T7_SOLVE2: the same in lane 0 (x2) and lane 1 (y2), where the solve adds to it
  float aim, agx, agy;       // this lane's img1 samples at (x1, y1), from the first pass
  int it = 0;                // Newton iterations
  int status = kTracked;
  // KLT_T7_REUSE: the last pass's image-2 corners (this lane's) and where they
  // came from; a pass whose corners are the same pixels in every lane takes
  // these instead of a gather round trip -- the same values, only the weights
  // (the position's fractions) change
  unsigned bpx = ~0u;
  Quad bi, bx, by;
};

enum { kPassAgain = 0, kPassDone = 1, kPassOOB = 2, kPassLostPrev = 3 };

// One pass of the Newton loop (trackFeatures.c:418-457): the top-of-loop
// bounds test, one gather round trip (img2's planes at x2; img1's at x1 on the
// level's FIRST pass; the deferred residue's img2 plane with a JOB), the
// ordered sums, the solve.  Separate instances for the first pass and the
// rest keep the first pass's addresses out of the loop.
// LZ (the lazy-gradient instances, AOS): 1 a level above 0, interleaved like
// any AOS level; 2 level 0, image 2 the img plane alone and image 1 that or
// (the launch's first frame, from a whole previous pyramid) interleaved.  In
// both the deferred residue's level 0 (R: a bank frame) is the img plane.
template <bool BAND, bool FIRST, bool JOB, bool AOS, bool FAST, int LZ = 0>
__device__ __forceinline__ int pass7(const TrkArgs &a, const Lev &A, const Lev &B, float x1, float y1, bool x1_out,
                                     LevState &ls, int lane, float fi, float fj, bool on, float *red, Pending &pd,
                                     const Lev &R, int &rstat, Counts &cnt, const Carry &cr = Carry{},
                                     unsigned cpx = ~0u) {
  T7_T(t_top);
  if constexpr (KLT_T7_SOLVE2 && !FIRST) ls.x2 = lane_of(ls.pxy, 0), ls.y2 = lane_of(ls.pxy, 1);
  bool stop = (FIRST && x1_out) || out7(ls.x2, ls.y2, A.tx, A.ty);
  if (BAND && !stop && (band_bad(B, ls.y2) || (FIRST && band_bad(A, y1)))) {
    *a.escape = 1;  // the caller redoes the chunk from whole-frame pyramids
    stop = true;
  }
  if (stop) {
    ls.status = kOOB;
    if (JOB) {  // the previous frame's verdict still needs its own pass
      const Pix q = pix_at(R.w, R.h, pd.x2 + fi, pd.y2 + fj);
      const float rb =
          interp(q, AOS && !LZ ? quad_i(R.img, q, (unsigned)R.w * 12u) : quad(R.img, q, (unsigned)R.w * 4u));
      float v[1] = {on ? fabsf(pd.aim - rb) : 0.0f}, S[1];
      ++cnt.passes;
      sums<1, FAST, LZ != 0>(red, lane, on, v, S);
      rstat = S[0] / (float)kNpx > a.max_res ? kLargeResidue : (pd.it >= a.max_it ? kMaxIter : kTracked);
      pd.on = false;
      if (rstat != kTracked) return kPassLostPrev;
    }
    return kPassOOB;
  }
  T7_ADD(11, t_top);
  T7_T(t_g0);
  ++cnt.passes;
  const unsigned rowB = (unsigned)B.w * (AOS ? 12u : 4u);
  const Pix qb = pix_at(B.w, B.h, ls.x2 + fi, ls.y2 + fj);
  Quad bi, bx, by;
  // a later pass whose corners are the last pass's pixels in every lane (the
  // position moved within its cell): no round trip (wave-uniform test)
  const bool reuse = !FIRST && KLT_T7_REUSE && __ballot(qb.px != ls.bpx) == 0ull;
  Pix qa = qb, qr = qb;
  Quad ai{}, ax{}, ay{}, ri{};
  if constexpr (LZ == 2) {
    // image 2's patch (unless the corners are reused), on a first pass image
    // 1's as well; every global load of the pass is issued before any is used
    float *pat = red + kRedF;
    if (FIRST) qa = pix_at(A.w, A.h, x1 + fi, y1 + fj);
    if (JOB) {
      qr = pix_at(R.w, R.h, pd.x2 + fi, pd.y2 + fj);
      ri = quad(R.img, qr, (unsigned)R.w * 4u);
    }
    const int X0b = u((int)(ls.x2 - (float)kHw)), Y0b = u((int)(ls.y2 - (float)kHw));
    const int cxb = (int)(ls.x2 + fi) - X0b, cyb = (int)(ls.y2 + fj) - Y0b;
    // image 1's corners kept from the previous frame's last pass (wave-uniform test)
    const bool carry = FIRST && KLT_T7_CARRY && __ballot(qa.px != cpx) == 0ull;
    if (reuse) {
      bi = ls.bi;
      bx = ls.bx;
      by = ls.by;
    } else if (!FIRST || carry) {
      float v[4];
      patch_load(B.img, B.w, B.h, X0b, Y0b, lane, v);
      patch_grads(pat, lane, a, B.w, B.h, v, X0b, Y0b, cxb, cyb, bi, bx, by);
      if (FIRST) ai = cr.i, ax = cr.x, ay = cr.y;
    } else if (A.il == kLayoutImg) {
      const int X0a = u((int)(x1 - (float)kHw)), Y0a = u((int)(y1 - (float)kHw));
      float v[4], va[4];
      patch_load(B.img, B.w, B.h, X0b, Y0b, lane, v);
      patch_load(A.img, A.w, A.h, X0a, Y0a, lane, va);
      patch_grads(pat, lane, a, B.w, B.h, v, X0b, Y0b, cxb, cyb, bi, bx, by);
      patch_grads(pat, lane, a, A.w, A.h, va, X0a, Y0a, (int)(x1 + fi) - X0a, (int)(y1 + fj) - Y0a, ai, ax, ay);
    } else {  // a whole previous pyramid: interleaved
      float v[4];
      patch_load(B.img, B.w, B.h, X0b, Y0b, lane, v);
      const Tri t = tri(A.img, qa, (unsigned)A.w * 12u);
      patch_grads(pat, lane, a, B.w, B.h, v, X0b, Y0b, cxb, cyb, bi, bx, by);
      ai = t.i, ax = t.x, ay = t.y;
    }
  } else if (reuse) {
    bi = ls.bi;
    bx = ls.bx;
    by = ls.by;
  } else if constexpr (AOS) {
    const Tri t = tri(B.img, qb, rowB);
    bi = t.i;
    bx = t.x;
    by = t.y;
  } else {
    bi = quad(B.img, qb, rowB);
    bx = quad(B.gx, qb, rowB);
    by = quad(B.gy, qb, rowB);
  }
  if (KLT_T7_REUSE) {
    ls.bpx = qb.px;
    ls.bi = bi;
    ls.bx = bx;
    ls.by = by;
  }
  if (FIRST && LZ != 2) {
    const unsigned rowA = (unsigned)A.w * (AOS ? 12u : 4u);
    qa = pix_at(A.w, A.h, x1 + fi, y1 + fj);
    if constexpr (AOS) {
      const Tri t = tri(A.img, qa, rowA);
      ai = t.i;
      ax = t.x;
      ay = t.y;
    } else {
      ai = quad(A.img, qa, rowA);
      ax = quad(A.gx, qa, rowA);
      ay = quad(A.gy, qa, rowA);
    }
  }
  if (JOB && LZ != 2) {
    qr = pix_at(R.w, R.h, pd.x2 + fi, pd.y2 + fj);
    ri = AOS && !LZ ? quad_i(R.img, qr, (unsigned)R.w * 12u) : quad(R.img, qr, (unsigned)R.w * 4u);
  }
  if (FIRST) {
    ls.aim = interp(qa, ai);
    ls.agx = interp(qa, ax);
    ls.agy = interp(qa, ay);
  }
  const float bim = interp(qb, bi), bgx = interp(qb, bx), bgy = interp(qb, by);
  // _computeIntensityDifference / _computeGradientSum (:68-123)
  const float dif = ls.aim - bim, gxs = ls.agx + bgx, gys = ls.agy + bgy;
#ifdef KLT_TRACK_PROF
  asm volatile("" ::"v"(dif), "v"(gxs), "v"(gys));
#endif
  T7_ADD(0, t_g0);
  T7_T(t_s0);
  // S2L: the exact sums stay in their lanes (row order kSum*) for the two-lane solve
  constexpr bool S2L = KLT_T7_SOLVE2 && !FAST;
  constexpr int iXX = S2L ? kSumGxx : 0, iXY = S2L ? kSumGxy : 1, iYY = S2L ? kSumGyy : 2, iEX = S2L ? kSumEx : 3,
                iEY = S2L ? kSumEy : 4, iRes = S2L ? kSumRes : 5;
  float S[6], acc = 0.0f;
  if (JOB) {
    const float rb = interp(qr, ri);
    float v[6];
    v[iXX] = gxs * gxs, v[iXY] = gxs * gys, v[iYY] = gys * gys, v[iEX] = dif * gxs, v[iEY] = dif * gys;
    v[iRes] = fabsf(pd.aim - rb);
    if constexpr (S2L) {
      acc = sums7_acc<6, LZ != 0>(red, lane, on, v);
      S[5] = lane_of(acc, kSumRes);
    } else {
      sums<6, FAST, LZ != 0>(red, lane, on, v, S);
    }
    rstat = S[5] / (float)kNpx > a.max_res ? kLargeResidue : (pd.it >= a.max_it ? kMaxIter : kTracked);
    pd.on = false;
    if (rstat != kTracked) return kPassLostPrev;  // that frame's feature is lost: this frame does not happen
  } else {
    float v[5];
    v[iXX] = gxs * gxs, v[iXY] = gxs * gys, v[iYY] = gys * gys, v[iEX] = dif * gxs, v[iEY] = dif * gys;
    if constexpr (S2L) {
      acc = sums7_acc<5, LZ != 0>(red, lane, on, v);
    } else {
      float S5[5];
      sums<5, FAST, LZ != 0>(red, lane, on, v, S5);
#pragma unroll
      for (int k = 0; k < 5; ++k) S[k] = S5[k];
    }
  }
  T7_ADD(1, t_s0);
  T7_T(t_v0);
  // _compute2by2GradientMatrix / _compute2by1ErrorVector / _solveEquation (:227-307): track7_solve.h
  ++cnt.solves;
  if constexpr (S2L) S[0] = lane_of(acc, kSumGxx), S[1] = lane_of(acc, kSumGxy), S[2] = lane_of(acc, kSumGyy);
  const float det = solve_det(S[0], S[1], S[2]);
  if (det < a.min_det) {
    ls.status = kSmallDet;  // x2 has not moved: the post-loop bounds test repeats this pass's
    return kPassDone;
  }
  bool moved;
  if constexpr (KLT_T7_SOLVE2) {
    float d;
    if constexpr (S2L) {
      d = solve2(acc, S[1], a.step, det);
    } else {
      int l = lane;
      if constexpr (LZ != 0) asm volatile("" : "+v"(l));  // no lane mask kept over the frames (sums7's PIN)
      const float S5[5] = {S[0], S[1], S[2], S[3], S[4]};
      d = solve2u(S5, l == 0, a.step, det);
    }
    ls.pxy += d;  // read out where it is next needed: no scalar pair held for it through a pass
    moved = (__ballot(fabsf(d) >= a.min_disp) & 3ull) != 0ull;  // |dx| or |dy|
  } else {
    const float S5[5] = {S[0], S[1], S[2], S[3], S[4]};
    float dx, dy;
    solve1(S5, a.step, det, dx, dy);
    dx = u(dx);
    dy = u(dy);
    ls.x2 = u(ls.x2 + dx);
    ls.y2 = u(ls.y2 + dy);
    moved = fabsf(dx) >= a.min_disp || fabsf(dy) >= a.min_disp;
  }
  ++ls.it;
  T7_ADD(2, t_v0);
  return (moved && ls.it < a.max_it) ? kPassAgain : kPassDone;
}

// _trackFeature at one level.  Returns the level's status; x2/y2 (uniform)
// move.  job: the previous frame's deferred residue rides along with this
// level's first pass (its verdict goes to rstat; when it loses that frame's
// feature the level stops at once and lost_prev is set).  defer: this
// (finest) level hands its own residue on (pd) instead of taking a pass for
// it.  residue: the finest level.
template <bool BAND, bool AOS, bool FAST, int LZ = 0>
__device__ int level7(const TrkArgs &a, const Lev &A, const Lev &B, float x1, float y1, float &x2, float &y2,
                      int lane, float fi, float fj, bool on, float *red, bool residue, bool defer, Pending &pd,
                      bool job, const Lev &R, int &rstat, bool &lost_prev, Counts &cnt, Carry *cr = nullptr,
                      unsigned cpx = ~0u) {
  const bool x1_out = out7(x1, y1, A.tx, A.ty);
  LevState ls;
  ls.x2 = x2;
  ls.y2 = y2;
  // x2 everywhere, y2 written into lane 1: no lane mask to make or keep.  The
  // compiler pads no hazard inside the statement, hence the two idle cycles
  // between the move that writes pxy and the lane write
  ls.pxy = x2;
  asm("s_nop 1\n\tv_writelane_b32 %0, %1, 1" : "+v"(ls.pxy) : "s"(y2));
  const Carry none{};
  const Carry &c0 = LZ == 2 ? *cr : none;
  int r = job ? pass7<BAND, true, true, AOS, FAST, LZ>(a, A, B, x1, y1, x1_out, ls, lane, fi, fj, on, red, pd, R, rstat,
                                                       cnt, c0, cpx)
              : pass7<BAND, true, false, AOS, FAST, LZ>(a, A, B, x1, y1, x1_out, ls, lane, fi, fj, on, red, pd, R, rstat,
                                                        cnt, c0, cpx);
  while (r == kPassAgain)
    r = pass7<BAND, false, false, AOS, FAST, LZ>(a, A, B, x1, y1, x1_out, ls, lane, fi, fj, on, red, pd, R, rstat, cnt);
  if constexpr (KLT_T7_SOLVE2) ls.x2 = lane_of(ls.pxy, 0), ls.y2 = lane_of(ls.pxy, 1);
  x2 = ls.x2;
  y2 = ls.y2;
  if constexpr (LZ == 2 && KLT_T7_CARRY && KLT_T7_REUSE) {  // this frame's image 2 is the next frame's image 1
    cr->px = ls.bpx;
    cr->i = ls.bi;
    cr->x = ls.bx;
    cr->y = ls.by;
  }
  if (r == kPassLostPrev) {
    lost_prev = true;
    return kTracked;
  }
  if (r == kPassOOB) return kOOB;
  // after the loop (:460-474)
  if (out7(x2, y2, A.tx, A.ty)) return kOOB;
  if (BAND && band_bad(B, y2)) {
    *a.escape = 1;
    return kOOB;
  }
  if (ls.status == kSmallDet) return kSmallDet;
  if (!residue) return ls.it >= a.max_it ? kMaxIter : kTracked;  // replaced by the next level's status
  if (defer) {  // the next frame's first pass computes it
    pd.on = true;
    pd.x2 = x2;
    pd.y2 = y2;
    pd.it = ls.it;
    pd.aim = ls.aim;
    return kTracked;
  }
  ++cnt.passes;
  T7_T(t_r0);
  const Pix q = pix_at(B.w, B.h, x2 + fi, y2 + fj);
  const float rb =
      interp(q, AOS && LZ != 2 ? quad_i(B.img, q, (unsigned)B.w * 12u) : quad(B.img, q, (unsigned)B.w * 4u));
  float v[1] = {on ? fabsf(ls.aim - rb) : 0.0f}, S1[1];
  sums<1, FAST, LZ != 0>(red, lane, on, v, S1);
  T7_ADD(3, t_r0);
  if (S1[0] / (float)kNpx > a.max_res) return kLargeResidue;
  return ls.it >= a.max_it ? kMaxIter : kTracked;
}

// NL > 0: the pyramid depth as a compile-time constant (the default 2), so
// the level loops unroll and every level's fields are loop-invariant scalars;
// NL == 0 reads a.nlev
//
// The body is track7_body.h, shared with k_track7_fb below.
// FB: the forward-backward instance (klt_hip_set_fb).  After frame j's forward
// track (image 1 = lev_prev(j), image 2 = bank frame j) a tracked feature goes
// through the same level loop with the two images exchanged, from its forward
// position -- KLTTrackFeatures(img2, img1) on a copy of the list -- and is
// rejected (x = y = -1, val = kFbRejected) when that loses it or ends farther
// than sqrt(fb.t2) from where frame j started.  A kept feature is the forward
// result.  Frame j's final status must be known before the backward pass, so
// the residue is not deferred (a.merge_res is ignored).  Each level7 call
// starts with an empty corner-reuse cache (LevState::bpx), so no corners of
// one direction's image 2 reach the other's or the next frame's; the bounds
// thresholds (oobx/ooby) depend on the level's size only and serve both.
// LAZY: level 0 of the bank is the img plane alone (klt_hip_set_lazy_grad);
// each wave's LDS then holds a gradient patch past its ordered-sum rows.
// Its two-level instances are held to five waves per SIMD (96 VGPRs; they
// take 95 and 92, no scratch), so that 5000 features are resident at once; the
// runtime-depth one (a one-level pyramid) takes 101 without a bound.  The
// other instances' bound of 1 wave is no constraint.
template <bool BAND, bool AOS, int NL, bool FAST = false, bool LAZY = false>
__global__ __launch_bounds__(kBlock, LAZY && NL == 2 ? 5 : LAZY ? 4 : 1) void k_track7(TrkArgs a, TrkFramesArgs b, float *__restrict__ fx,
                                                   float *__restrict__ fy, int *__restrict__ fv, int n) {
  static_assert(!LAZY || (AOS && !BAND), "lazy gradients: whole-frame interleaved pyramids");
  __shared__ __attribute__((aligned(16))) float red_all[kWaves][kRedF + (LAZY ? kPat : 0)];
  constexpr bool FB = false, HOOK = false, MULTI = false, PRED = false, MASK = false;
  const TrkFbArgs fb{};
  const TrkMultiArgs ms{};
  const TrkPredArgs pr{};
  const TrkMaskArgs mk{};
#include "track7_body.h"
}

// the lazy-gradient instances with the exit count and the wave times
// (TrkFramesArgs::exits / ::wave_t; track7_body.h's HOOK): kernels of their
// own, so that every other instance stays the code it was
template <int NL, bool FAST>
__global__ __launch_bounds__(kBlock, NL == 2 ? 5 : 4) void k_track7_hook(TrkArgs a, TrkFramesArgs b,
                                                                          float *__restrict__ fx,
                                                                          float *__restrict__ fy,
                                                                          int *__restrict__ fv, int n) {
  __shared__ __attribute__((aligned(16))) float red_all[kWaves][kRedF + kPat];
  constexpr bool BAND = false, AOS = true, LAZY = true, FB = false, HOOK = true, MULTI = false, PRED = false, MASK = false;
  const TrkFbArgs fb{};
  const TrkMultiArgs ms{};
  const TrkPredArgs pr{};
  const TrkMaskArgs mk{};
#include "track7_body.h"
}

// the forward-backward instances: whole-frame pyramids, exact sums
template <bool AOS, int NL>
__global__ __launch_bounds__(kBlock) void k_track7_fb(TrkArgs a, TrkFramesArgs b, TrkFbArgs fb,
                                                      float *__restrict__ fx, float *__restrict__ fy,
                                                      int *__restrict__ fv, int n) {
  __shared__ __attribute__((aligned(16))) float red_all[kWaves][kRedF];
  constexpr bool BAND = false, FAST = false, FB = true, LAZY = false, HOOK = false, MULTI = false, PRED = false, MASK = false;
  const TrkMultiArgs ms{};
  const TrkPredArgs pr{};
  const TrkMaskArgs mk{};
#include "track7_body.h"
}

// the multi-sequence instances (klt_hip_track_frames_multi): whole-frame
// interleaved pyramids with full level-0 records, exact sums.  Kernels of their
// own with the sequences' first features beside TrkFramesArgs, so that every
// other instance keeps its arguments and stays the code it was; in the body
// only the wave's sequence lookup and the level bases differ (lev_cur /
// lev_before).
template <int NL>
__global__ __launch_bounds__(kBlock) void k_track7_multi(TrkArgs a, TrkFramesArgs b, TrkMultiArgs ms,
                                                         float *__restrict__ fx, float *__restrict__ fy,
                                                         int *__restrict__ fv, int n) {
  __shared__ __attribute__((aligned(16))) float red_all[kWaves][kRedF];
  constexpr bool BAND = false, AOS = true, FAST = false, FB = false, LAZY = false, HOOK = false, MULTI = true,
                 PRED = false, MASK = false;
  const TrkFbArgs fb{};
  const TrkPredArgs pr{};
  const TrkMaskArgs mk{};
#include "track7_body.h"
}

// the motion-prior instances (klt_hip_set_predict): whole-frame pyramids with
// full level-0 records, exact sums.  Frame j's search starts in image 2 at the
// feature's position moved by its displacement over frame j-1 (TrkPredArgs:
// read with the list, written back with it), unless that start's window leaves
// the coarsest level.  The displacement is known only once the frame's status
// is, so the residue is taken in place (a.merge_res is ignored) and no corners
// are carried.  Kernels of their own, like the forward-backward ones, so that
// every other instance keeps its arguments and stays the code it was; they are
// instantiated in a code object of their own (track7_pred.hip).
template <bool AOS, int NL>
__global__ __launch_bounds__(kBlock) void k_track7_pred(TrkArgs a, TrkFramesArgs b, TrkPredArgs pr,
                                                        float *__restrict__ fx, float *__restrict__ fy,
                                                        int *__restrict__ fv, int n) {
  __shared__ __attribute__((aligned(16))) float red_all[kWaves][kRedF];
  constexpr bool BAND = false, FAST = false, FB = false, LAZY = false, HOOK = false, MULTI = false, PRED = true, MASK = false;
  const TrkFbArgs fb{};
  const TrkMultiArgs ms{};
  const TrkMaskArgs mk{};
#include "track7_body.h"
}

// the region-mask instances (klt_hip_set_mask, KLT_HIP_MASK_TRACK): whole-frame
// pyramids with full level-0 records, exact sums.  After the level loop a
// feature whose position is inside the border and lies on a masked pixel is
// lost with kMasked (TrkMaskArgs: one byte read per feature-frame).  The test
// needs the frame's final position, so the residue is taken in place
// (a.merge_res is ignored).  Kernels of their own in a code object of their own
// (track7_mask.hip), like the motion-prior ones.
template <bool AOS, int NL>
__global__ __launch_bounds__(kBlock) void k_track7_mask(TrkArgs a, TrkFramesArgs b, TrkMaskArgs mk,
                                                        float *__restrict__ fx, float *__restrict__ fy,
                                                        int *__restrict__ fv, int n) {
  __shared__ __attribute__((aligned(16))) float red_all[kWaves][kRedF];
  constexpr bool BAND = false, FAST = false, FB = false, LAZY = false, HOOK = false, MULTI = false, PRED = false,
                 MASK = true;
  const TrkFbArgs fb{};
  const TrkMultiArgs ms{};
  const TrkPredArgs pr{};
#include "track7_body.h"
}

// ... and their lazy-gradient twins, for the batched calls whose banks hold
// level 0 as the img plane alone (klt_hip_set_lazy_grad): the hook instances'
// body (exit count and wave times, so that the tail schedule applies), the
// deferred residue included.  The mask comes last in the argument segment
// (T7MaskKArgs) and is read from there at the test.
template <int NL>
__global__ __launch_bounds__(kBlock, NL == 2 ? 5 : 4) void k_track7_mask_lazy(TrkArgs a, TrkFramesArgs b,
                                                                               float *__restrict__ fx,
                                                                               float *__restrict__ fy,
                                                                               int *__restrict__ fv, int n,
                                                                               TrkMaskArgs mk) {
  __shared__ __attribute__((aligned(16))) float red_all[kWaves][kRedF + kPat];
  constexpr bool BAND = false, AOS = true, FAST = false, LAZY = true, FB = false, HOOK = true, MULTI = false,
                 PRED = false, MASK = true;
  const TrkFbArgs fb{};
  const TrkMultiArgs ms{};
  const TrkPredArgs pr{};
#include "track7_body.h"
}

// The fb, pred and mask launchers' tables hold the three <AOS, NL> instances
// in this order: <false, 0>, <true, 0>, <true, 2>.  Planes are tracked at the
// runtime depth whatever it is (interleaved levels are the fused path's, which
// is two levels deep).
inline int t7_layout_depth_row(bool aos, bool two) { return aos ? (two ? 2 : 1) : 0; }

}  // namespace
}  // namespace kltdev
