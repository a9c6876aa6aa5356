// track7_mask.hip -- the region-mask instances of the default tracker
// (k_track7_mask and k_track7_mask_lazy, klt_hip_set_mask with
// KLT_HIP_MASK_TRACK) in a code object of their own, as track7_pred.hip holds
// the motion prior's.  The kernel templates are track7_kernels.h's.
#include "track7_kernels.h"

namespace kltdev {
namespace {

// the mask is the third argument of k_track7_mask and the last of k_track7_mask_lazy
using T7MaskKernel = decltype(&k_track7_mask<false, 0>);
using T7MaskLazyKernel = decltype(&k_track7_mask_lazy<0>);

const KernelRow<T7MaskKernel> kMaskRows[3] = {  // [t7_layout_depth_row]
    {"kltdev::k_track7_mask<false, 0>", k_track7_mask<false, 0>},
    {"kltdev::k_track7_mask<true, 0>", k_track7_mask<true, 0>},
    {"kltdev::k_track7_mask<true, 2>", k_track7_mask<true, 2>},
};

const KernelRow<T7MaskLazyKernel> kMaskLazyRows[2] = {  // [two levels]
    {"kltdev::k_track7_mask_lazy<0>", k_track7_mask_lazy<0>},
    {"kltdev::k_track7_mask_lazy<2>", k_track7_mask_lazy<2>},
};

}  // namespace

// a: launch_track7's, with the bounds thresholds set
hipError_t launch_track7_mask(hipStream_t st, const TrkArgs &a, const TrkFramesArgs &b, const TrkMaskArgs &mk, float *x,
                              float *y, int *v, int n, int grid, bool two, const char **name) {
  if (a.lazy) {  // launch_track7 has checked the layout: interleaved levels, level 0 the img plane
    const KernelRow<T7MaskLazyKernel> &row = kMaskLazyRows[two];
    if (name) *name = row.name;
    hipLaunchKernelGGL(row.kernel, dim3(grid), dim3(kBlock), 0, st, a, b, x, y, v, n, mk);
    return hipGetLastError();
  }
  const KernelRow<T7MaskKernel> &row = kMaskRows[t7_layout_depth_row(a.aos, two)];
  if (name) *name = row.name;
  hipLaunchKernelGGL(row.kernel, dim3(grid), dim3(kBlock), 0, st, a, b, mk, x, y, v, n);
  return hipGetLastError();
}

}  // namespace kltdev
