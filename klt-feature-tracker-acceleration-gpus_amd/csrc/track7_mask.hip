// track7_mask.hip -- the region-mask instances of the default tracker
// (k_track7_mask, klt_hip_set_mask with KLT_HIP_MASK_TRACK) in a code object of
// their own, as track7_pred.hip holds the motion prior's: track7.hip is
// included with only launch_track7_mask compiled, so that its own code object
// holds the instances it held before.
#define KLT_T7_MASK_UNIT 1
#include "track7.hip"
