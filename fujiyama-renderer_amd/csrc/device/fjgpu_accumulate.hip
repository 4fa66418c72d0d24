// fjgpu_accumulate.hip -- the kernels of fjgpu_accumulate and fjgpu_accumulate_tile_error (include/fjgpu.h): the running mean of frames
// that differ in their sampler seed, and the error of that mean per tile.  The arithmetic is fjgpu_accum_math.h, the same source the host
// twin of the CPU tests compiles; this file is the launch shape around it.
//
//   k_ac_accumulate  one thread per pixel of a 16 x 16 patch of a listed rectangle; block b is patch b % patches of rectangle b / patches,
//                    `patches` the patch count of the largest rectangle (a block beyond its own rectangle's patches leaves at once).  The
//                    lanes of a wave are a patch of 16 x 4 pixels, as in k_tp_accumulate: four runs of 256 bytes of RGBA.  The new colour
//                    and the mean are one 16-byte load each, the mean one 16-byte store.  64 bytes per pixel (68 with the variance): 16 of
//                    the frame, 24 of the state read and 24 written.  Nothing is read twice: no LDS, no atomics, no scratch; a block talks
//                    to no other, and a pixel outside the rectangles is neither read nor written.
//   k_ac_tile_error  one block of 256 threads per rectangle.  Thread (tx, ty) walks its pixel of every patch of the rectangle and sums
//                    their errors in f64; the sums meet in a butterfly over the wave (__shfl_xor of the two halves of the double, offsets
//                    32 .. 1) and the four waves' results in one LDS step, added left to right by thread 0 -- a fixed order, so the
//                    result does not depend on the schedule and the host twin can restate it.  28 bytes read per pixel, 4 written per tile.
#include <hip/hip_runtime.h>

#include "fjgpu_accumulate.h"

namespace {

constexpr int AC_THREADS = FJ_AC_BX * FJ_AC_BY, AC_WAVES = AC_THREADS / FJ_AC_WAVE;

__global__ void __launch_bounds__(AC_THREADS) k_ac_accumulate(AcBuffers B, const int32_t *rects, uint32_t patches, int xres, int reset)
{
  const uint32_t ri = blockIdx.x / patches, pi = blockIdx.x - ri * patches;
  const int4 r = *(const int4 *) (rects + 4 * (size_t) ri);
  const uint32_t px = (uint32_t) (r.z - r.x + FJ_AC_BX - 1) / FJ_AC_BX, py = (uint32_t) (r.w - r.y + FJ_AC_BY - 1) / FJ_AC_BY;
  if (pi >= px * py) return;
  const uint32_t by = pi / px, bx = pi - by * px;
  const int x = r.x + (int) (bx * FJ_AC_BX + threadIdx.x), y = r.y + (int) (by * FJ_AC_BY + threadIdx.y);
  if (x >= r.z || y >= r.w) return;
  fj_ac_pixel(B, xres, reset, x, y);
}

__device__ __forceinline__ double ac_shfl_xor(double v, int off)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, off, FJ_AC_WAVE);
  hi = __shfl_xor(hi, off, FJ_AC_WAVE);
  return __hiloint2double(hi, lo);
}

__global__ void __launch_bounds__(AC_THREADS) k_ac_tile_error(const float *mean, const float *m2, const float *count, const int32_t *rects,
    int xres, float lum_floor, float *errors)
{
  __shared__ double wave_sum[AC_WAVES];
  __shared__ int wave_short[AC_WAVES];
  const int32_t *rect = rects + 4 * (size_t) blockIdx.x;
  int short_history = 0;
  double s = fj_ac_thread_sum(mean, m2, count, xres, lum_floor, rect, (int) threadIdx.x, (int) threadIdx.y, &short_history);
  for (int off = FJ_AC_WAVE / 2; off >= 1; off >>= 1) {
    s = s + ac_shfl_xor(s, off);
    short_history |= __shfl_xor(short_history, off, FJ_AC_WAVE);
  }
  const int t = (int) (threadIdx.y * FJ_AC_BX + threadIdx.x);
  if ((t & (FJ_AC_WAVE - 1)) == 0) { wave_sum[t / FJ_AC_WAVE] = s; wave_short[t / FJ_AC_WAVE] = short_history; }
  __syncthreads();
  if (t == 0) {
    double total = wave_sum[0];
    int sh = wave_short[0];
    for (int w = 1; w < AC_WAVES; w++) { total = total + wave_sum[w]; sh |= wave_short[w]; }
    errors[blockIdx.x] = fj_ac_tile_result(total, rect, sh);
  }
}

}  // namespace

int launch_ac_accumulate(hipStream_t st, const AcBuffers &B, const int32_t *d_rects, int n_rects, uint32_t max_patches, int xres, int reset)
{
  if (n_rects <= 0 || max_patches == 0) return 0;
  if ((unsigned long long) n_rects * max_patches > 0x7fffffffull) return (int) hipErrorInvalidConfiguration;      // (the entry point refuses it)
  hipLaunchKernelGGL(k_ac_accumulate, dim3((uint32_t) n_rects * max_patches), dim3(FJ_AC_BX, FJ_AC_BY), 0, st, B, d_rects, max_patches, xres, reset);
  return (int) hipGetLastError();
}

int launch_ac_tile_error(hipStream_t st, const float *mean, const float *m2, const float *count, const int32_t *d_rects, int n_rects, int xres,
    float lum_floor, float *d_errors)
{
  if (n_rects <= 0) return 0;
  hipLaunchKernelGGL(k_ac_tile_error, dim3((uint32_t) n_rects), dim3(FJ_AC_BX, FJ_AC_BY), 0, st, mean, m2, count, d_rects, xres, lum_floor, d_errors);
  return (int) hipGetLastError();
}
