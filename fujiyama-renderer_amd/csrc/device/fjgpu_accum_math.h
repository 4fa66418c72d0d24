// fjgpu_accum_math.h -- the arithmetic of fjgpu_accumulate and fjgpu_accumulate_tile_error (include/fjgpu.h): the running mean of a
// sequence of frames that differ only in their sampler seed, the variance of that mean per pixel, and its reduction to one error per tile.
//
// ONE source for the device kernels (fjgpu_accumulate.hip: k_ac_accumulate, k_ac_tile_error), for the host twin the CPU tests run
// (tools/accumulate_host.cc) and for tests/accumulate_model.py, which restates it in numpy.  f32 under -ffp-contract=off, in the order
// written here; the tile's sum alone is f64.
//
//   state       mean (4), m2, count per pixel; with `reset` the state read counts as zero (what is stored is not looked at)
//   skip        a new pixel with a channel that is not finite changes nothing: the state written is the state read (zero under reset)
//   update      n = count + 1;  mean_k' = mean_k + (x_k - mean_k) / n  for k = r, g, b, a
//               l = l(x.rgb), m = l(mean.rgb) of the mean BEFORE the update (l of fjgpu_denoise_var_math.h);
//               d = l - m;  m' = m + d / n;  m2' = m2 + d * (l - m');  count' = n
//   variance    of the MEAN: v = count' >= 2 ? m2' / (count' * (count' - 1)) : 0     (a skipped pixel: from the state it keeps)
//   pixel error e_p = sqrtf(v) / max(l(mean.rgb), lum_floor); a pixel with count < 2 makes its tile's error +INFINITY
//   tile error  the f64 sum of e_p in the order of fj_ac_tile_sum -- thread t = ty * 16 + tx of 256 sums its pixels (x0 + tx + 16 i,
//               y0 + ty + 16 j), j outer, i inner; a butterfly over each run of 64 threads (offsets 32, 16, .., 1); the four results left to
//               right -- divided by the pixel count in f64 and rounded to f32 once
//
// The luminance mean is NOT a state plane: l is linear, so l(mean) is the mean of the l(x) up to the rounding of the four f32 operations
// of l and of the three channel updates, a few ulp of m.  What that costs was measured on the CPU with tests/accumulate_model.py against a
// model that stores m (tests/test_accumulate_cpu.py, test_luminance_of_the_mean_against_a_stored_luminance_mean: 64 frames of 37 x 23,
// a smooth colour times 1 +- amplitude of uniform noise): the two m2 agree to 1e-6 relative (median 1e-7) at an amplitude of 0.5 and to
// 3e-4 (median 4e-5) at 1e-3 -- the difference is d times an error of m of about 1e-7 m, so it grows as the spread nears f32's
// resolution of the mean, where a stored m is no better known (it carries its own rounding of 64 updates).  Equal frames give d = 0 and
// m2 = 0 exactly either way.  Not worth 8 more bytes per pixel on a pass that moves 64.
#ifndef FJGPU_ACCUM_MATH_H
#define FJGPU_ACCUM_MATH_H

#include <math.h>
#include <stdint.h>

#include "fjgpu_denoise_var_math.h"

#define FJ_AC_BX 16
#define FJ_AC_BY 16
#define FJ_AC_WAVE 64

typedef float ac_v4f __attribute__((ext_vector_type(4)));

// the frames of a call: pointers to pixel (0, 0) of [yres][xres][channels] arrays -- device memory in the kernels, host memory in the twin
struct AcBuffers {
  const float *color;            // [4], 16-byte aligned
  float *mean;                   // [4], 16-byte aligned
  float *m2, *count;             // [1]
  float *variance_out;           // [1] or null
};

FJ_DN_FN bool fj_ac_finite(float v) { return v - v == 0.f; }      // (false for NaN and both infinities)

FJ_DN_FN float fj_ac_variance(float m2, float n) { return n >= 2.f ? m2 / (n * (n - 1.f)) : 0.f; }

// one pixel of fjgpu_accumulate
FJ_DN_FN void fj_ac_pixel(const AcBuffers &B, int xres, int reset, int x, int y)
{
  const size_t p = (size_t) y * (size_t) xres + (size_t) x;
  const ac_v4f c = *(const ac_v4f *) (B.color + 4 * p);
  ac_v4f mean = {0.f, 0.f, 0.f, 0.f};
  float m2 = 0.f, count = 0.f;
  if (!reset) {
    mean = *(const ac_v4f *) (B.mean + 4 * p);
    m2 = B.m2[p];
    count = B.count[p];
  }
  const bool ok = fj_ac_finite(c.x) && fj_ac_finite(c.y) && fj_ac_finite(c.z) && fj_ac_finite(c.w);
  if (ok) {
    const float n = count + 1.f;
    const float l = fj_dnv_luminance(c.x, c.y, c.z);
    const float m = fj_dnv_luminance(mean.x, mean.y, mean.z);
    mean.x = mean.x + (c.x - mean.x) / n;
    mean.y = mean.y + (c.y - mean.y) / n;
    mean.z = mean.z + (c.z - mean.z) / n;
    mean.w = mean.w + (c.w - mean.w) / n;
    const float d = l - m;
    const float m1 = m + d / n;
    m2 = m2 + d * (l - m1);
    count = n;
  }
  if (ok || reset) {
    *(ac_v4f *) (B.mean + 4 * p) = mean;
    B.m2[p] = m2;
    B.count[p] = count;
  }
  if (B.variance_out) B.variance_out[p] = fj_ac_variance(m2, count);
}

// one pixel of fjgpu_accumulate_tile_error: its error, and *short_history |= count < 2
FJ_DN_FN double fj_ac_pixel_error(const float *mean, const float *m2, const float *count, int xres, float lum_floor, int x, int y,
    int *short_history)
{
  const size_t p = (size_t) y * (size_t) xres + (size_t) x;
  const float n = count[p];
  if (!(n >= 2.f)) *short_history = 1;
  const ac_v4f mu = *(const ac_v4f *) (mean + 4 * p);
  const float v = fj_ac_variance(m2[p], n);
  const float l = fj_dnv_luminance(mu.x, mu.y, mu.z);
  return (double) (sqrtf(v) / (l > lum_floor ? l : lum_floor));
}

// what thread (tx, ty) of the tile's block sums: its pixels of every 16 x 16 patch of the rectangle, patches row by row
FJ_DN_FN double fj_ac_thread_sum(const float *mean, const float *m2, const float *count, int xres, float lum_floor, const int32_t *rect,
    int tx, int ty, int *short_history)
{
  double s = 0.;
  for (int y = rect[1] + ty; y < rect[3]; y += FJ_AC_BY)
    for (int x = rect[0] + tx; x < rect[2]; x += FJ_AC_BX) s += fj_ac_pixel_error(mean, m2, count, xres, lum_floor, x, y, short_history);
  return s;
}

// the tile's error from the sum of its block and the verdict of its pixels
FJ_DN_FN float fj_ac_tile_result(double sum, const int32_t *rect, int short_history)
{
  if (short_history) return INFINITY;
  return (float) (sum / (double) ((size_t) (rect[2] - rect[0]) * (size_t) (rect[3] - rect[1])));
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the reduction of the block as a plain loop (the host twin): per[256] are the threads' sums in thread order
static inline double fj_ac_tile_sum(double *per)
{
  double total = 0.;
  for (int w = 0; w < FJ_AC_BX * FJ_AC_BY / FJ_AC_WAVE; w++) {
    double *v = per + w * FJ_AC_WAVE;
    for (int off = FJ_AC_WAVE / 2; off >= 1; off >>= 1) {
      double nxt[FJ_AC_WAVE];
      for (int i = 0; i < FJ_AC_WAVE; i++) nxt[i] = v[i] + v[i ^ off];
      for (int i = 0; i < FJ_AC_WAVE; i++) v[i] = nxt[i];
    }
    total = w == 0 ? v[0] : total + v[0];
  }
  return total;
}
#endif

#endif
