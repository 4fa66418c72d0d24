// fjgpu_temporal.hip -- the kernel of fjgpu_denoise_temporal (include/fjgpu.h): reprojection of the previous frame's history and the blend
// of the new frame into it.  The arithmetic is fjgpu_temporal_math.h, the same source the host twin of the CPU tests compiles; this file is
// the launch shape around it.
//
//   k_tp_accumulate  one thread per region pixel, blocks of 16 x 16 pixels.  The lanes of a wave are 64 consecutive threads of the block, that
//                    is a patch of 16 x 4 pixels: its own pixels are four runs of 256 bytes of RGBA, and the four-tap gathers of a
//                    slowly moving camera land in a patch of about the same size, so the lanes' taps share cache lines (a wave of 64 x 1
//                    pixels would touch twice as many rows for the same taps).  RGBA is one 16-byte load or store.  No LDS: nothing is read
//                    twice by design -- what the lanes share they share through the cache --, no atomics, no scratch memory; a block talks
//                    to no other.  About 170 bytes per pixel with an albedo: 72 of the current frame, 68 of history and previous guides at
//                    one tap's worth (the other three come from lines the neighbours fetch), 32 written.  fj_tp_pixel issues the loads of
//                    all four taps before it tests any (one round of memory latency per pixel instead of one per test and tap: 0.150 ->
//                    0.094 ms at 1080p, profiles/temporal_pass.txt).
#include <hip/hip_runtime.h>

#include "fjgpu_temporal.h"

namespace {

constexpr int TP_BX = 16, TP_BY = 16;

__global__ void __launch_bounds__(TP_BX * TP_BY) k_tp_accumulate(TpParams k, TpBuffers B)
{
  const int x = k.x0 + (int) (blockIdx.x * TP_BX + threadIdx.x), y = k.y0 + (int) (blockIdx.y * TP_BY + threadIdx.y);
  if (x >= k.x1 || y >= k.y1) return;
  fj_tp_pixel(k, B, x, y);
}

}  // namespace

int launch_tp_accumulate(hipStream_t st, const TpParams &k, const TpBuffers &B)
{
  const int w = k.x1 - k.x0, h = k.y1 - k.y0;
  if (w <= 0 || h <= 0) return 0;
  const dim3 grid((w + TP_BX - 1) / TP_BX, (h + TP_BY - 1) / TP_BY);
  if (grid.y > 65535u) return (int) hipErrorInvalidConfiguration;      // (the entry point refuses a taller region)
  hipLaunchKernelGGL(k_tp_accumulate, grid, dim3(TP_BX, TP_BY), 0, st, k, B);
  return (int) hipGetLastError();
}
