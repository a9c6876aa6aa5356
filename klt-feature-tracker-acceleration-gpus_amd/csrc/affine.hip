// affine.hip -- the affine consistency check of KLTTrackFeatures on gfx950
// (trackFeatures.c:503-1225 and the record stage :1438-1497), one frame pair
// per launch (klt_hip_track_affine).  Not on the default path: it runs only
// when tc->affineConsistencyCheck >= 0.  The per-feature stage is
// affine_dev.h, which the batched tracker (track.hip) runs inside its launch.
#pragma clang fp contract(off)

#include <math.h>

#include "affine_dev.h"

namespace kltdev {
namespace {

namespace aff {
constexpr int CH = 256;  // pixels per ordered-sum chunk (4 per lane)
constexpr int LDS = NS * CH + SOLVE;
}  // namespace aff

// one wave per feature, after the translation tracker's launch of the same frame
__global__ __launch_bounds__(kWave) void k_affine(AffArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[aff::LDS];
  const int k = blockIdx.x, lane = threadIdx.x;
  if (k >= a.n) return;
  const int S = (a.p.ww + 2) * (a.p.wh + 2);
  const int v_in = a.v[k], st = a.state[k];
  if (v_in != kTracked) {  // lost this frame (windows dropped) or not tracked at all
    if (lane == 0) a.state[k] = 0;
    return;
  }
  float *afp = a.aff + 6 * k;
  float af[6] = {afp[0], afp[1], afp[2], afp[3], afp[4], afp[5]};
  const AffImg I1{a.ai, a.agx, a.agy, a.aw, a.ah}, I2{a.bi, a.bgx, a.bgy, a.bw, a.bh};
  int status;
  const int ns = aff_stage<aff::CH>(lds, lds + aff::NS * aff::CH, a.p, I1, I2, a.store + (size_t)k * 3 * S, af,
                                    a.xp[k], a.yp[k], a.x[k], a.y[k], st != 0 ? 1 : 0, lane, status);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) afp[q] = af[q];
    a.state[k] = ns;
    if (status != kTracked) {
      a.v[k] = status;
      a.xo[k] = -1.0f;
      a.yo[k] = -1.0f;
    }
  }
}

// stored windows between the store and a packed staging buffer:
// dir 0: staging[m] -> store[idx[m]], dir 1: store[idx[m]] -> staging[m]
__global__ __launch_bounds__(kBlock) void k_affine_move(int dir, const int *__restrict__ idx, int m, int s3,
                                                        float *__restrict__ staging, float *__restrict__ store) {
  const long total = (long)m * s3;
  for (long e = blockIdx.x * (long)kBlock + threadIdx.x; e < total; e += (long)gridDim.x * kBlock) {
    const int j = (int)(e / s3), q = (int)(e - (long)j * s3);
    float *st = store + (long)idx[j] * s3 + q;
    if (dir == 0) *st = staging[e];
    else staging[e] = *st;
  }
}

}  // namespace

hipError_t launch_affine(hipStream_t st, const AffArgs &a) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_affine, dim3(a.n), dim3(kWave), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_affine_move(hipStream_t st, int dir, const int *idx, int m, int s3, float *staging, float *store) {
  const long total = (long)m * s3;
  if (total <= 0) return hipSuccess;
  const int blocks = (int)((total + kBlock - 1) / kBlock < 4096 ? (total + kBlock - 1) / kBlock : 4096);
  hipLaunchKernelGGL(k_affine_move, dim3(blocks), dim3(kBlock), 0, st, dir, idx, m, s3, staging, store);
  return hipGetLastError();
}

}  // namespace kltdev
