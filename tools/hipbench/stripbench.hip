// Memory-pattern probe of a one-wave strip form of the image-only level 0,
// without its arithmetic, beside today's kernel and the tile pattern:
//   strip    one wave64 per workgroup walks a 192-pixel strip down a segment
//            of rows.  Per row: one clamped dword load per lane (lane l holds
//            pixels S-32+4l..+3, a ring of PF rows ahead), one 16-byte
//            nontemporal img0 store from lanes 8..55 (768 contiguous bytes),
//            one 4-byte hs store from the same 48 lanes (three whole 64-byte
//            pieces of the hs slabs).  Segments load 2 rows above and below.
//   tile     rwbench's pattern cut to the image-only instance: 42 x 96 B of
//            u8 per 64x32 tile in 16-byte loads, then img0 and the hs slab run
//   k_pyr_l0 the real image-only kernel (launch_pyr_l0, kLayoutImg)
//   k_pyr_l0s the strip kernel itself, segment lengths and ring depths swept,
//            each compared bit for bit with the tile kernel's img0 and hs
// 64 frames of 1920x1080 and 3840x2160; three timed passes each for the spread.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -I include \
//          -Wno-unused-value -I klt-feature-tracker-acceleration-gpus_amd/csrc -o tools/hipbench/stripbench \
//          tools/hipbench/stripbench.hip
#include "../../klt-feature-tracker-acceleration-gpus_amd/csrc/pyramid.hip"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace kltdev;

typedef float pf4 __attribute__((ext_vector_type(4)));

template <int PF>
__global__ __launch_bounds__(64) void k_strip_pat(const uint8_t *__restrict__ src, float *__restrict__ img0,
                                                  float *__restrict__ hs, int W, int H, int nstrips, int nseg, int seg,
                                                  long fs_hs) {
  const int per = (int)gridDim.x / 8;
  const int t = (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
  if (t >= nstrips * nseg) return;
  const int sg = t / nstrips, sx = t - sg * nstrips;
  const int lane = threadIdx.x, S = sx * 192;
  const int px = S - 32 + 4 * lane, xl = min(max(px, 0), W - 4);
  const int y0 = sg * seg, y1 = min(y0 + seg, H);
  const long plane = (long)W * H;
  src += blockIdx.z * plane;
  img0 += blockIdx.z * plane;
  hs += blockIdx.z * fs_hs;
  const bool useful = lane >= 8 && lane < 56;
  const int X = (S >> 2) + lane - 8;
  unsigned ring[PF];
#pragma unroll
  for (int k = 0; k < PF; ++k)
    ring[k] = *reinterpret_cast<const unsigned *>(src + (unsigned)(min(max(y0 - 2 + k, 0), H - 1) * W + xl));
  for (int yb = y0 - 2; yb < y1 + 2; yb += PF) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const unsigned d = ring[k];
      ring[k] = *reinterpret_cast<const unsigned *>(src + (unsigned)(min(max(yb + k + PF, 0), H - 1) * W + xl));
      const int y = yb + k - 2;  // the row whose outputs are complete once row y+2 has arrived
      if (y >= y0 && y < y1 && useful) {
        const pf4 v = {(float)(d & 0xFF), (float)((d >> 8) & 0xFF), (float)((d >> 16) & 0xFF), (float)(d >> 24)};
        __builtin_nontemporal_store(v, reinterpret_cast<pf4 *>(img0 + (unsigned)(y * W + px)));
        hs[hs_at32(y, X, H)] = v.x + v.w;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_tile_pat(const uint8_t *__restrict__ src, float *__restrict__ img0,
                                                  float *__restrict__ hs, int W, int H, int tiles_x, int tiles_y,
                                                  long fs_hs) {
  const int per = (int)gridDim.x / 8;
  const int t = (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
  if (t >= tiles_x * tiles_y) return;
  const int by = t / tiles_x, bx = t - by * tiles_x;
  const int C0 = bx * 64, R0 = by * 32, tid = threadIdx.x;
  const long plane = (long)W * H;
  src += blockIdx.z * plane;
  img0 += blockIdx.z * plane;
  hs += blockIdx.z * fs_hs;
  __shared__ unsigned u[44 * 24];
  if (tid < 42 * 6) {
    const int r = tid / 6, q = tid - r * 6;
    const int x = min(max(C0 - 12 + 16 * q, 0), W - 16), y = min(max(R0 - 5 + r, 0), H - 1);
    *reinterpret_cast<uint4 *>(&u[r * 24 + 4 * q]) = *reinterpret_cast<const uint4 *>(src + (long)y * W + x);
  }
  __syncthreads();
  const unsigned acc = u[tid] ^ u[tid + 512];
  const int g = tid & 15, rl = tid >> 4;
  const pf4 v = {(float)acc, (float)g, 1.f, 2.f};
  for (int r = rl; r < 32; r += 16)
    if (R0 + r < H) __builtin_nontemporal_store(v, reinterpret_cast<pf4 *>(img0 + (long)(R0 + r) * W + C0 + 4 * g));
  // hs: rows R0..R0+31 of slab bx, 16 floats each, 2 per thread
  const int r = tid >> 3;
  if (R0 + r < H) *reinterpret_cast<float2 *>(hs + ((long)bx * H + R0 + r) * 16 + 2 * (tid & 7)) = make_float2(acc, 1.f);
}

struct Bufs {
  uint8_t *src;
  float *img, *hs;
};
// img0 and hs of frames 0 and F-1
static void fetch(const Bufs &B, long np, long nh, int F, std::vector<float> &v) {
  hipMemcpy(v.data(), B.img, np * 4, hipMemcpyDeviceToHost);
  hipMemcpy(v.data() + np, B.img + (F - 1) * np, np * 4, hipMemcpyDeviceToHost);
  hipMemcpy(v.data() + 2 * np, B.hs, nh * 4, hipMemcpyDeviceToHost);
  hipMemcpy(v.data() + 2 * np + nh, B.hs + (F - 1) * nh, nh * 4, hipMemcpyDeviceToHost);
}

template <class L>
static void timed(const char *name, int W, int H, int F, L launch) {
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  for (int w = 0; w < 3; ++w) launch();
  printf("%-28s %dx%d", name, W, H);
  for (int pass = 0; pass < 3; ++pass) {
    const int reps = 10;
    hipEventRecord(a);
    for (int r = 0; r < reps; ++r) launch();
    hipEventRecord(b);
    if (hipEventSynchronize(b) != hipSuccess) {
      printf(" failed: %s\n", hipGetErrorString(hipGetLastError()));
      exit(1);
    }
    float ms;
    hipEventElapsedTime(&ms, a, b);
    const double us = ms * 1e3 / (reps * F);
    printf("  %.3f us/frame (%.2f TB/s)", us, 6.0 * W * H / (us * 1e-6) / 1e12);
  }
  printf("\n");
  fflush(stdout);
  hipEventDestroy(a);
  hipEventDestroy(b);
}

template <int PF>
static void strip(const Bufs &B, int W, int H, int F, int seg) {
  const int ns = W / 192, nseg = (H + seg - 1) / seg;
  const long nh = hs_size(W / 4, H);
  char name[64];
  snprintf(name, sizeof name, "strip seg %d ring %d", seg, PF);
  timed(name, W, H, F, [&] {
    hipLaunchKernelGGL(k_strip_pat<PF>, dim3(xcd_grid(ns * nseg), 1, F), dim3(64), 0, 0, B.src, B.img, B.hs, W, H, ns,
                       nseg, seg, nh);
  });
}

// the strip kernel at one segment length and ring depth, timed, then its
// planes of frames 0 and F-1 compared with the tile kernel's (want)
template <int PF>
static void run_l0s(const Bufs &B, int W, int H, int F, int seg, const DefTaps &T, const std::vector<float> &want) {
  const int ns = (W + l0s::SW - 1) / l0s::SW, nseg = (H + seg - 1) / seg;
  const long np = (long)W * H, nh = hs_size(W / 4, H);
  hipMemset(B.img, 0xFF, np * F * 4);
  hipMemset(B.hs, 0xFF, nh * F * 4);
  char name[64];
  snprintf(name, sizeof name, "k_pyr_l0s seg %d ring %d", seg, PF);
  timed(name, W, H, F, [&] {
    hipLaunchKernelGGL(k_pyr_l0s<PF>, dim3(xcd_grid(ns * nseg), 1, F), dim3(64), 0, 0, B.src, W, W, H, T, B.img, B.hs,
                       np, np, nh, ns, nseg, seg);
  });
  std::vector<float> got(2 * (np + nh));
  fetch(B, np, nh, F, got);
  printf("    %s\n", memcmp(got.data(), want.data(), got.size() * 4) ? "DIFFERS from the tiles" : "same bits as the tiles");
}

static int run(int W, int H, int F) {
  const long np = (long)W * H, nh = hs_size(W / 4, H);
  Bufs B;
  if (hipMalloc(&B.src, np * F) || hipMalloc(&B.img, np * F * 4) || hipMalloc(&B.hs, nh * F * 4)) {
    fprintf(stderr, "hipMalloc failed\n");
    return 1;
  }
  std::vector<uint8_t> h(np * F);
  for (long i = 0; i < np * F; ++i) h[i] = (uint8_t)((i * 2654435761u) >> 24);
  hipMemcpy(B.src, h.data(), np * F, hipMemcpyHostToDevice);
  DefTaps T;
  for (int i = 0; i < 5; ++i) T.s[i] = 0.2f;
  for (int i = 0; i < 7; ++i) T.g[i] = 1.0f / 7, T.d[i] = (i - 3) * 0.1f;
  for (int i = 0; i < 21; ++i) T.p[i] = 1.0f / 21;
  const int ty = (H + geom::L0_TH - 1) / geom::L0_TH;
  timed("k_pyr_l0 image-only", W, H, F, [&] {
    launch_pyr_l0(0, B.src, W, np, W, H, T, 1, 1, B.img, nullptr, nullptr, B.hs, W / 4, 1, np, nh, F, 0, ty, 0, ty,
                  kLayoutImg);
  });
  std::vector<float> want(2 * (np + nh));
  fetch(B, np, nh, F, want);
  timed("tile pattern 64x32", W, H, F, [&] {
    hipLaunchKernelGGL(k_tile_pat, dim3(xcd_grid((W / 64) * ty), 1, F), dim3(256), 0, 0, B.src, B.img, B.hs, W, H,
                       W / 64, ty, nh);
  });
  for (int seg : {H / 20, H / 10, H / 5}) {
    strip<4>(B, W, H, F, seg);
    strip<8>(B, W, H, F, seg);
    strip<12>(B, W, H, F, seg);
  }
  for (int seg : {H / 40, H / 30, H / 20, H / 15, H / 10, H / 5}) {
    run_l0s<5>(B, W, H, F, seg, T, want);
    run_l0s<10>(B, W, H, F, seg, T, want);
  }
  timed("k_pyr_l0 image-only", W, H, F, [&] {
    launch_pyr_l0(0, B.src, W, np, W, H, T, 1, 1, B.img, nullptr, nullptr, B.hs, W / 4, 1, np, nh, F, 0, ty, 0, ty,
                  kLayoutImg);
  });
  hipFree(B.src);
  hipFree(B.img);
  hipFree(B.hs);
  return 0;
}

int main() {
  if (run(1920, 1080, 64)) return 1;
  return run(3840, 2160, 64);
}
