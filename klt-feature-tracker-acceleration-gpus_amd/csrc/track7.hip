// track7.hip -- the launchers of the default configuration's tracker
// (track7_kernels.h) and the code object of its k_track7, k_track7_hook,
// k_track7_fb and k_track7_multi instances: nineteen kernels, one table row
// each.  The motion-prior and region-mask instances are track7_pred.hip's and
// track7_mask.hip's.
#include <string.h>

#include <type_traits>

#include "track7_kernels.h"

namespace kltdev {

// out7's threshold for a level dimension n: the bit pattern of the smallest
// float x >= 3 with (float)n - (x + 3) < 1.001f, by bisection over the
// patterns of [3, n] (the test is false at 3 unless n < 7.001, true at n)
static int oob_threshold(int n) {
  auto out = [n](int xb) {
    float x;
    memcpy(&x, &xb, sizeof x);
    volatile float t = x + 3.0f;  // the device's float operations, one rounding each
    volatile float g = (float)n - t;
    return g < 1.001f;
  };
  const float c = (float)(n > 3 ? n : 3);
  int lo, hi;
  const float three = 3.0f;
  memcpy(&lo, &three, sizeof lo);
  memcpy(&hi, &c, sizeof hi);
  if (out(lo)) return lo;
  while (hi - lo > 1) {  // out(lo) false, out(hi) true
    const int mid = lo + (hi - lo) / 2;
    if (out(mid)) hi = mid;
    else lo = mid;
  }
  return hi;
}

namespace {

// one pointer type per argument list: k_track7 and k_track7_hook share theirs
using T7Kernel = decltype(&k_track7<false, false, 0>);
using T7FbKernel = decltype(&k_track7_fb<false, 0>);
using T7MultiKernel = decltype(&k_track7_multi<0>);
static_assert(std::is_same<T7Kernel, decltype(&k_track7_hook<0, false>)>::value, "one argument list");

const KernelRow<T7MultiKernel> kMultiRows[2] = {  // [two levels]
    {"kltdev::k_track7_multi<0>", k_track7_multi<0>},
    {"kltdev::k_track7_multi<2>", k_track7_multi<2>},
};

const KernelRow<T7FbKernel> kFbRows[3] = {  // [t7_layout_depth_row]
    {"kltdev::k_track7_fb<false, 0>", k_track7_fb<false, 0>},
    {"kltdev::k_track7_fb<true, 0>", k_track7_fb<true, 0>},
    {"kltdev::k_track7_fb<true, 2>", k_track7_fb<true, 2>},
};

// full level-0 records or planes, exact sums.  The names of these eight
// instances are reported without the last template argument (LAZY = false),
// as they were before it existed; callers match on the strings, so they stay.
const KernelRow<T7Kernel> kExactRows[2][3] = {  // [band][t7_layout_depth_row]
    {{"kltdev::k_track7<false, false, 0, false>", k_track7<false, false, 0, false, false>},
     {"kltdev::k_track7<false, true, 0, false>", k_track7<false, true, 0, false, false>},
     {"kltdev::k_track7<false, true, 2, false>", k_track7<false, true, 2, false, false>}},
    {{"kltdev::k_track7<true, false, 0, false>", k_track7<true, false, 0, false, false>},
     {"kltdev::k_track7<true, true, 0, false>", k_track7<true, true, 0, false, false>},
     {"kltdev::k_track7<true, true, 2, false>", k_track7<true, true, 2, false, false>}},
};
// KLT_HIP_FAST: the runtime sends only interleaved two-level pyramids here
const KernelRow<T7Kernel> kFastRows[2] = {  // [band]
    {"kltdev::k_track7<false, true, 2, true>", k_track7<false, true, 2, true, false>},
    {"kltdev::k_track7<true, true, 2, true>", k_track7<true, true, 2, true, false>},
};
// lazy gradients; with the exit count or the wave times, the hook instances
const KernelRow<T7Kernel> kLazyRows[2][3] = {  // [hook][runtime depth, two levels, two levels with fast sums]
    {{"kltdev::k_track7<false, true, 0, false, true>", k_track7<false, true, 0, false, true>},
     {"kltdev::k_track7<false, true, 2, false, true>", k_track7<false, true, 2, false, true>},
     {"kltdev::k_track7<false, true, 2, true, true>", k_track7<false, true, 2, true, true>}},
    {{"kltdev::k_track7_hook<0, false>", k_track7_hook<0, false>},
     {"kltdev::k_track7_hook<2, false>", k_track7_hook<2, false>},
     {"kltdev::k_track7_hook<2, true>", k_track7_hook<2, true>}},
};

}  // namespace

hipError_t launch_track7_multi(hipStream_t st, const TrkArgs &a_in, const TrkFramesArgs &b, const TrkMultiArgs &m,
                               float *x, float *y, int *v, int n, const char **name) {
  // the runtime sends interleaved full-record levels of one size in A and B,
  // exact sums, and first[] ascending from 0 to n
  if (!a_in.aos || a_in.fast || a_in.lazy || a_in.escape || m.nseq < 1 || m.nseq > kMaxSeq || m.first[0] != 0 ||
      m.first[m.nseq] != n || b.perm || b.n_dev || b.xcd_per)
    return hipErrorInvalidValue;
  TrkArgs a = a_in;
  for (int l = 0; l < KLT_HIP_MAX_LEVELS; ++l) {
    a.oobx[l] = oob_threshold(a.B[l].w);
    a.ooby[l] = oob_threshold(a.B[l].h);
  }
  const int grid = (n + kWaves - 1) / kWaves;
  const KernelRow<T7MultiKernel> &row = kMultiRows[a.nlev == 2];
  if (name) *name = row.name;
  hipLaunchKernelGGL(row.kernel, dim3(grid), dim3(kBlock), 0, st, a, b, m, x, y, v, n);
  return hipGetLastError();
}

hipError_t launch_track7(hipStream_t st, bool band, const TrkArgs &a_in, const TrkFramesArgs &b, float *x, float *y,
                         int *v, int n, const char **name, const TrkFbArgs *fb, const TrkPredArgs *pr,
                         const TrkMaskArgs *mk) {
  TrkArgs a = a_in;
  for (int l = 0; l < KLT_HIP_MAX_LEVELS; ++l) {
    a.oobx[l] = oob_threshold(a.B[l].w);
    a.ooby[l] = oob_threshold(a.B[l].h);
  }
  const int nb = (n + kWaves - 1) / kWaves;
  const int grid = b.xcd_per > 0 ? 8 * b.xcd_per : nb;
  // band: escape checks (klt_hip_track_frames_band); aos: interleaved levels
  const bool two = a.nlev == 2;
  if (fb) {  // the runtime refuses band calls and fast sums with the check on
    if (band || a.fast || pr || mk) return hipErrorInvalidValue;
    const KernelRow<T7FbKernel> &row = kFbRows[t7_layout_depth_row(a.aos, two)];
    if (name) *name = row.name;
    hipLaunchKernelGGL(row.kernel, dim3(grid), dim3(kBlock), 0, st, a, b, *fb, x, y, v, n);
    return hipGetLastError();
  }
  if (pr) {  // the runtime refuses band calls, fast sums, lazy gradients and the checks with the prior on
    if (band || a.fast || a.lazy || mk || !pr->vx || !pr->vy) return hipErrorInvalidValue;
    return launch_track7_pred(st, a, b, *pr, x, y, v, n, grid, two, name);
  }
  if (mk) {  // the same refusals with the region mask's tracking use on
    if (band || a.fast || !mk->mask || mk->pitch < a.ncols) return hipErrorInvalidValue;
    if (a.lazy) {  // as below: whole-frame interleaved pyramids, level 0 of the bank an img plane
      if (!a.aos || a.B[0].il != kLayoutImg) return hipErrorInvalidValue;
      for (int l = 0; l < a.nlev; ++l)
        if (a.A[l].w != a.B[l].w || a.A[l].h != a.B[l].h) return hipErrorInvalidValue;
    }
    return launch_track7_mask(st, a, b, *mk, x, y, v, n, grid, two, name);
  }
  const KernelRow<T7Kernel> *row;
  if (a.lazy) {  // the runtime sends whole-frame interleaved pyramids here (fast sums: two levels)
    if (band || !a.aos || (a.fast && !two)) return hipErrorInvalidValue;
    // the bank's level 0 is an img plane, and the kept pyramid has the bank's
    // level sizes: the kernels take image 1's from image 2's (lev_img1)
    if (a.B[0].il != kLayoutImg) return hipErrorInvalidValue;
    for (int l = 0; l < a.nlev; ++l)
      if (a.A[l].w != a.B[l].w || a.A[l].h != a.B[l].h) return hipErrorInvalidValue;
    row = &kLazyRows[b.exits || b.wave_t][a.fast ? 2 : two ? 1 : 0];
  } else if (a.fast) {
    row = &kFastRows[band];
  } else {
    row = &kExactRows[band][t7_layout_depth_row(a.aos, two)];
  }
  if (name) *name = row->name;
  hipLaunchKernelGGL(row->kernel, dim3(grid), dim3(kBlock), 0, st, a, b, x, y, v, n);
  return hipGetLastError();
}

}  // namespace kltdev
