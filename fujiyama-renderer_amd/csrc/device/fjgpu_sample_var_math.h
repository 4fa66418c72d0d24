// fjgpu_sample_var_math.h -- the arithmetic of fjgpu_render_tiles_variance (include/fjgpu.h): the variance of a pixel's filtered estimate
// from the samples of its filter window.  One source for the kernel k_sample_variance (fjgpu_sample_variance.hip) and for the host twin
// of the CPU tests (csrc/tools/sample_variance_host.cc); tests/sample_variance_model.py restates this text in numpy f64.  Compiled with
// -ffp-contract=off.
//
// A pixel p and the npx_x * npx_y samples s of its window -- the samples k_resolve (fjgpu_kernels.hip) reads for p, with its indexing and
// its (u, v):
//   w_s   k_resolve's Gaussian weight in f64: filtx = xres u - (px + .5), filty = yres (1 - v) - (py + .5), xx = 2 filtx / fw,
//         yy = 2 filty / fh, w = exp(-2 (xx xx + yy yy))
//   l_s   (double) fj_dnv_luminance(d), f32 as the filters compute it (fjgpu_denoise_var_math.h); d is the sample's rgb, or with an albedo
//         fj_dn_demodulate(x, fj_dn_albedo_clamp(albedo[p][c], albedo_floor)) per channel -- the PIXEL's albedo, so that the moments
//         describe what fjgpu_denoise_variance and fjgpu_denoise_temporal call luminance
//   pass 1   S0 = sum w,  S1 = sum w l,  m = S1 / S0
//   pass 2   the same samples and weights: S2 = sum w (l - m)^2,  Q = sum w^2       (two passes: no E[l^2] - E[l]^2)
//   e = Q / S0^2  (1 / n for n equal weights),   V = (S2 / S0) e / (1 - e)  -- for n equal weights the unbiased sample variance over n;
//   V = 0 where e >= 1 (one sample); rounded to f32 once; a V that is negative or not finite (a non-finite sample, say) is 0.f.
// All sums are f64; their order is the caller's (the kernel's butterfly, the twin's row-major loop).
#ifndef FJGPU_SAMPLE_VAR_MATH_H
#define FJGPU_SAMPLE_VAR_MATH_H

#include <math.h>
#include <stddef.h>

#include "fjgpu_denoise_var_math.h"

// the frame and filter as k_resolve sees them (the members of ResolveParams)
struct SvFrame {
  int xres, yres, rate_x, rate_y, npx_x, npx_y;
  double fw, fh;
};

FJ_DN_FN double fj_sv_weight(const SvFrame &f, int px, int py, double u, double v)
{
  const double filtx = f.xres * u - (px + .5);
  const double filty = f.yres * (1 - v) - (py + .5);
  const double xx = 2 * filtx / f.fw;
  const double yy = 2 * filty / f.fh;
  return exp(-2 * (xx * xx + yy * yy));
}

// a: the pixel's albedo after fj_dn_albedo_clamp, or null
FJ_DN_FN double fj_sv_luminance(float r, float g, float b, const float *a)
{
  if (a) { r = fj_dn_demodulate(r, a[0]); g = fj_dn_demodulate(g, a[1]); b = fj_dn_demodulate(b, a[2]); }
  return (double) fj_dnv_luminance(r, g, b);
}

FJ_DN_FN void fj_sv_pass1(double &S0, double &S1, double w, double l) { S0 += w; S1 += w * l; }

FJ_DN_FN void fj_sv_pass2(double &S2, double &Q, double w, double l, double m)
{
  const double d = l - m;
  S2 += w * (d * d);
  Q += w * w;
}

FJ_DN_FN float fj_sv_result(double S0, double S2, double Q)
{
  const double e = Q / (S0 * S0);
  if (e >= 1) return 0.f;
  const float V = (float) ((S2 / S0) * e / (1 - e));
  return (V >= 0.f && V <= 3.402823466e+38f) ? V : 0.f;
}

// the whole pixel over arrays, samples in row-major order: `first` is the window's first sample (k_resolve's `base`), `row` the samples per
// row of the tile (TileDesc.nx); s_uv [.][2] f64, s_accum [.][4] f32
FJ_DN_FN float fj_sv_pixel(const SvFrame &f, int px, int py, size_t first, int row, const double *s_uv, const float *s_accum, const float *a)
{
  double S0 = 0, S1 = 0, S2 = 0, Q = 0;
  for (int sy = 0; sy < f.npx_y; sy++)
    for (int sx = 0; sx < f.npx_x; sx++) {
      const size_t s = first + (size_t) sy * row + sx;
      fj_sv_pass1(S0, S1, fj_sv_weight(f, px, py, s_uv[2 * s], s_uv[2 * s + 1]), fj_sv_luminance(s_accum[4 * s], s_accum[4 * s + 1], s_accum[4 * s + 2], a));
    }
  const double m = S1 / S0;
  for (int sy = 0; sy < f.npx_y; sy++)
    for (int sx = 0; sx < f.npx_x; sx++) {
      const size_t s = first + (size_t) sy * row + sx;
      fj_sv_pass2(S2, Q, fj_sv_weight(f, px, py, s_uv[2 * s], s_uv[2 * s + 1]), fj_sv_luminance(s_accum[4 * s], s_accum[4 * s + 1], s_accum[4 * s + 2], a), m);
    }
  return fj_sv_result(S0, S2, Q);
}

#endif
