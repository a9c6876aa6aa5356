// track7_solve.h -- the 2x2 solve of one Newton pass (_solveEquation,
// trackFeatures.c:281-307, after the matrix and the error vector of :227-278),
// shared by track7_kernels.h's pass7 and the self-check kernel in pyramid.hip
// (klt_hip_selftest_solve2).  Included inside namespace kltdev; contraction is
// off for every file (csrc/Makefile).
//
// solve1: every value wave-uniform -- each of its VALU instructions is a whole
// wave64 instruction for one useful lane.
// solve2 (KLT_T7_SOLVE2): lane 0 computes dx and lane 1 dy with one instruction
// stream.  Per lane the operations and their operands are solve1's,
//   lane 0: (gyy * ex - gxy * ey) / det     lane 1: (gxx * ey - gxy * ex) / det
// as (a * e1 - gxy * e2) / det with {a, e1, e2} = {gyy, ex, ey} / {gxx, ey, ex},
// two rounded products, one subtraction, one IEEE division, so the results are
// solve1's bit for bit; det and its test stay uniform.  The other lanes compute
// on whatever they hold and are not read.  The numerator is solve_num in all of
// them: left to itself the compiler turns a * e1 - gxy * e2 into
// a * e1 + (-gxy) * e2 in some instances and not in others -- the same number,
// but a NaN e2 then comes out with the other sign.
#ifndef KLT_TRACK7_SOLVE_H
#define KLT_TRACK7_SOLVE_H

#ifndef KLT_T7_SOLVE2
#define KLT_T7_SOLVE2 1  // A/B hook: 0 solves on wave-uniform values
#endif

// The order of the ordered sums' rows with KLT_T7_SOLVE2 (exact sums: lane l
// adds up row l): one quad holds gyy, gxx, ex, ey, so that lanes 0 and 1 have
// their `a` in place and take e1 / e2 by two quad permutes; gxy is read out as
// the scalar operand (one constant-bus operand per instruction).
enum { kSumGyy = 0, kSumGxx = 1, kSumEx = 2, kSumEy = 3, kSumGxy = 4, kSumRes = 5 };
constexpr int kQuad2323 = 0xEE, kQuad3232 = 0xBB;  // DPP quad_perm:[2,3,2,3] / [3,2,3,2]

__device__ __forceinline__ float lane_of(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
template <int CTRL>
__device__ __forceinline__ float quad_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// det of {gxx, gxy; gxy, gyy}, wave-uniform in every variant; the caller tests it
// against min_det before it solves
__device__ __forceinline__ float solve_det(float gxx, float gxy, float gyy) { return gxx * gyy - gxy * gxy; }

// a * e1 - gxy * e2: two rounded products, one subtraction; the second product
// is a value of its own (no negation folded into a multiplicand)
__device__ __forceinline__ float solve_num(float a, float e1, float gxy, float e2) {
  float q = gxy * e2;
  asm volatile("" : "+v"(q));
  return a * e1 - q;
}

// S = {gxx, gxy, gyy, sum(dif * gx), sum(dif * gy)}
__device__ __forceinline__ void solve1(const float (&S)[5], float step, float det, float &dx, float &dy) {
  const float gxx = S[0], gxy = S[1], gyy = S[2];
  const float ex = S[3] * step, ey = S[4] * step;
  dx = solve_num(gyy, ex, gxy, ey) / det;
  dy = solve_num(gxx, ey, gxy, ex) / det;
}

// acc: lane kSum* holds that sum (the error sums before the step factor), gxy
// that lane's value.  Returns d: lane 0 dx, lane 1 dy.
__device__ __forceinline__ float solve2(float acc, float gxy, float step, float det) {
  const float es = acc * step;  // lanes 2, 3: ex, ey
  const float e1 = quad_mov<kQuad2323>(es), e2 = quad_mov<kQuad3232>(es);
  return solve_num(acc, e1, gxy, e2) / det;
}

// The same from wave-uniform sums (the fast sums leave every sum in one lane):
// l0 is lane == 0.
__device__ __forceinline__ float solve2u(const float (&S)[5], bool l0, float step, float det) {
  const float gxx = S[0], gxy = S[1], gyy = S[2];
  const float ex = S[3] * step, ey = S[4] * step;
  const float a = l0 ? gyy : gxx, e1 = l0 ? ex : ey, e2 = l0 ? ey : ex;
  return solve_num(a, e1, gxy, e2) / det;
}

#endif  // KLT_TRACK7_SOLVE_H
