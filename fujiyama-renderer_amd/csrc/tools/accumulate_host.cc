// accumulate_host.cc -- validation tool: fjgpu_accumulate and fjgpu_accumulate_tile_error (include/fjgpu.h) as plain loops over HOST arrays,
// every pixel through fj_ac_pixel / fj_ac_thread_sum of device/fjgpu_accum_math.h -- the SAME functions k_ac_accumulate and k_ac_tile_error
// call -- so that tests/test_accumulate_cpu.py can hold the arithmetic against its numpy restatement without a GPU.  Built with the ROCm
// clang++ under -ffp-contract=off.  Not part of the product path.
#include <stdint.h>
#include <math.h>

#include "fjgpu.h"
#include "fjgpu_accum_math.h"

namespace {

// the rectangles of a call: the caller's, or the whole frame; false for what the entries refuse
bool rects_ok(int xres, int yres, const int32_t *rects, int n)
{
  if (xres <= 0 || yres <= 0 || n < 0) return false;
  for (int i = 0; i < n; i++) {
    const int32_t *r = rects + 4 * i;
    if (r[0] < 0 || r[1] < 0 || r[2] > xres || r[3] > yres || r[0] >= r[2] || r[1] >= r[3]) return false;
  }
  return true;
}

}  // namespace

extern "C" {

// the arguments of fjgpu_accumulate on host memory; 0, or -2 (FJGPU_EINVAL) for what it refuses (the overlap tests are the entry's own)
int fj_accumulate_host(int xres, int yres, const int32_t *rects, int n_rects, const float *color, const fjgpu_accum_state *state, int reset,
    float *variance_out)
{
  if (!color || !state || !state->mean || !state->m2 || !state->count) return FJGPU_EINVAL;
  const int32_t whole[4] = {0, 0, xres, yres};
  if (!rects) { rects = whole; n_rects = 1; }
  if (!rects_ok(xres, yres, rects, n_rects)) return FJGPU_EINVAL;
  if (((uintptr_t) color | (uintptr_t) state->mean) & 15u) return FJGPU_EINVAL;
  AcBuffers B;
  B.color = color; B.mean = state->mean; B.m2 = state->m2; B.count = state->count; B.variance_out = variance_out;
  for (int i = 0; i < n_rects; i++) {
    const int32_t *r = rects + 4 * i;
    for (int y = r[1]; y < r[3]; y++)
      for (int x = r[0]; x < r[2]; x++) fj_ac_pixel(B, xres, reset ? 1 : 0, x, y);
  }
  return 0;
}

// the arguments of fjgpu_accumulate_tile_error on host memory: the threads of a block one after the other, then the block's reduction
int fj_accumulate_tile_error_host(int xres, int yres, const int32_t *rects, int n_rects, const fjgpu_accum_state *state, float lum_floor,
    float *errors_out)
{
  if (!state || !state->mean || !state->m2 || !state->count || !errors_out) return FJGPU_EINVAL;
  const int32_t whole[4] = {0, 0, xres, yres};
  if (!rects) { rects = whole; n_rects = 1; }
  if (!rects_ok(xres, yres, rects, n_rects)) return FJGPU_EINVAL;
  if (!(isfinite(lum_floor) && lum_floor > 0.f)) return FJGPU_EINVAL;
  if ((uintptr_t) state->mean & 15u) return FJGPU_EINVAL;
  for (int i = 0; i < n_rects; i++) {
    const int32_t *r = rects + 4 * i;
    double per[FJ_AC_BX * FJ_AC_BY];
    int short_history = 0;
    for (int ty = 0; ty < FJ_AC_BY; ty++)
      for (int tx = 0; tx < FJ_AC_BX; tx++)
        per[ty * FJ_AC_BX + tx] = fj_ac_thread_sum(state->mean, state->m2, state->count, xres, lum_floor, r, tx, ty, &short_history);
    errors_out[i] = fj_ac_tile_result(fj_ac_tile_sum(per), r, short_history);
  }
  return 0;
}

}
