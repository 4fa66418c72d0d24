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
//   k_tp_accumulate_clamped<R>  fjgpu_denoise_temporal_clamped with a clamp, R = 1, 2, 3: described at the kernel
//                    (profiles/temporal_clamp.txt).
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

// the clamped pass: the same block of 16 x 16 pixels, with the records of its tile and a halo of R pixels (RGBA, L, id: FJ_TP_REC words)
// staged in LDS once, because here every value of the current frame IS read (2R + 1)^2 times by design.  The 256 threads write the
// (16 + 2R)^2 records in turn, L once per record; a halo pixel outside the region is not loaded, and fj_tp_clamp tells from the tap's
// coordinates that it does not count, so its record is never read.  Every thread reaches the barrier -- the threads beyond a ragged
// region's edge stage their share like the others and leave after it.  A row of the tile is (16 + 2R) FJ_TP_REC + 1 words: a record is 6
// words, so the 16 lanes of a row read one field from 16 different even banks of the 32 (6 tx mod 32), and the odd row length puts the
// half-wave's second row on the odd ones -- the dword window reads of a wave meet no bank conflict.  7.9, 9.7, 11.7 KB for R = 1, 2, 3.
template <int R>
__global__ void __launch_bounds__(TP_BX * TP_BY) k_tp_accumulate_clamped(TpParams k, TpBuffers B, TpClamp c)
{
  constexpr int T = TP_BX + 2 * R, ROW = T * FJ_TP_REC + 1;
  static_assert(TP_BX == TP_BY, "the tile is square");
  __shared__ float tile[T * ROW];
  const int bx = k.x0 + (int) (blockIdx.x * TP_BX), by = k.y0 + (int) (blockIdx.y * TP_BY);
  for (int i = (int) (threadIdx.y * TP_BX + threadIdx.x); i < T * T; i += TP_BX * TP_BY) {
    const int ry = i / T, rx = i - ry * T;
    const int qx = bx - R + rx, qy = by - R + ry;
    if (qx >= k.x0 && qx < k.x1 && qy >= k.y0 && qy < k.y1) fj_tp_record(k, B, qx, qy, tile + ry * ROW + rx * FJ_TP_REC);
  }
  __syncthreads();
  const int x = bx + (int) threadIdx.x, y = by + (int) threadIdx.y;
  if (x >= k.x1 || y >= k.y1) return;
  fj_tp_pixel_clamped<R>(k, B, c, tile + ((int) threadIdx.y + R) * ROW + ((int) threadIdx.x + R) * FJ_TP_REC, ROW, FJ_TP_REC, x, y);
}

}  // namespace

int launch_tp_accumulate_clamped(hipStream_t st, const TpParams &k, const TpBuffers &B, const TpClamp &c)
{
  const int w = k.x1 - k.x0, h = k.y1 - k.y0;
  if (w <= 0 || h <= 0) return 0;
  const dim3 grid((w + TP_BX - 1) / TP_BX, (h + TP_BY - 1) / TP_BY), block(TP_BX, TP_BY);
  if (grid.y > 65535u) return (int) hipErrorInvalidConfiguration;      // (the entry point refuses a taller region)
  switch (c.radius) {
    case 1: hipLaunchKernelGGL(k_tp_accumulate_clamped<1>, grid, block, 0, st, k, B, c); break;
    case 2: hipLaunchKernelGGL(k_tp_accumulate_clamped<2>, grid, block, 0, st, k, B, c); break;
    case 3: hipLaunchKernelGGL(k_tp_accumulate_clamped<3>, grid, block, 0, st, k, B, c); break;
    default: return (int) hipErrorInvalidValue;                        // (the entry point refuses the radius)
  }
  return (int) hipGetLastError();
}

int launch_tp_accumulate(hipStream_t st, const TpParams &k, const TpBuffers &B)
{
  const int w = k.x1 - k.x0, h = k.y1 - k.y0;
  if (w <= 0 || h <= 0) return 0;
  const dim3 grid((w + TP_BX - 1) / TP_BX, (h + TP_BY - 1) / TP_BY);
  if (grid.y > 65535u) return (int) hipErrorInvalidConfiguration;      // (the entry point refuses a taller region)
  hipLaunchKernelGGL(k_tp_accumulate, grid, dim3(TP_BX, TP_BY), 0, st, k, B);
  return (int) hipGetLastError();
}
