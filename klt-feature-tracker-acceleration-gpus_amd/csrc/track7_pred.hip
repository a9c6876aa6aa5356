// track7_pred.hip -- the motion-prior instances of the default tracker
// (k_track7_pred, klt_hip_set_predict) in a code object of their own, so that
// track7.hip's holds the instances it held before.  The kernel template, its
// body (track7_body.h) and everything it calls are track7_kernels.h's.
#include "track7_kernels.h"

namespace kltdev {
namespace {

using T7PredKernel = decltype(&k_track7_pred<false, 0>);

const KernelRow<T7PredKernel> kPredRows[3] = {  // [t7_layout_depth_row]
    {"kltdev::k_track7_pred<false, 0>", k_track7_pred<false, 0>},
    {"kltdev::k_track7_pred<true, 0>", k_track7_pred<true, 0>},
    {"kltdev::k_track7_pred<true, 2>", k_track7_pred<true, 2>},
};

}  // namespace

// a: launch_track7's, with the bounds thresholds set
hipError_t launch_track7_pred(hipStream_t st, const TrkArgs &a, const TrkFramesArgs &b, const TrkPredArgs &pr, float *x,
                              float *y, int *v, int n, int grid, bool two, const char **name) {
  const KernelRow<T7PredKernel> &row = kPredRows[t7_layout_depth_row(a.aos, two)];
  if (name) *name = row.name;
  hipLaunchKernelGGL(row.kernel, dim3(grid), dim3(kBlock), 0, st, a, b, pr, x, y, v, n);
  return hipGetLastError();
}

}  // namespace kltdev
