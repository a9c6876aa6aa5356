// track7_pred.hip -- the motion-prior instances of the default tracker
// (k_track7_pred, klt_hip_set_predict) in a code object of their own: the
// kernels, their shared body (track7_body.h) and everything they call are
// track7.hip's, included here with only launch_track7_pred compiled, so that
// track7.hip's own code object holds the instances it held before.
#define KLT_T7_PRED_UNIT 1
#include "track7.hip"
