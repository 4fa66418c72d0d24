// fjgpu_denoise_var_math.h -- the arithmetic of fjgpu_denoise_estimate_variance and fjgpu_denoise_variance (include/fjgpu.h): the a-trous
// filter of fjgpu_denoise_math.h with the edge-stopping function of SVGF (Schied et al., HPG 2017, 4.2 and 4.4) in place of the colour term --
// the luminance distance in units of the local standard deviation, the variance filtered along with the colour -- and the spatial variance
// estimate SVGF falls back to where a pixel has no temporal history, which in a single-frame renderer is every pixel.
//
// ONE source for the device kernels (fjgpu_denoise_variance.hip), for the host twin the CPU tests run (tools/denoise_variance_host.cc) and
// for the constants computed on the host.  f32 under -ffp-contract=off, every sum left to right, one expf per tap, taps dy outer and dx
// inner; tests/denoise_variance_model.py restates it in numpy.  k_n, k_x are those of fj_dn_constants; a tap outside the region is skipped,
// and so is (stop_at_ids) a tap of another instance id.
//
//   l(C) = 0.2126f C.r + 0.7152f C.g + 0.0722f C.b
//
//   estimate, taps q = p + (dx, dy), dx, dy = -3..3:    w = expf(-(d2n k_n + d2x k_x))     (guides only; the centre weighs 1)
//     pass 1   s0 += w; s1 += w l_q;          m = s1 / s0
//     pass 2   d = l_q - m; s2 += w (d d);    V = s2 / s0, V = V > 0 ? V : 0       (same taps, same weights; E[l^2] - E[l]^2 would cancel)
//
//   iteration i, spacing 2^i, colour C and variance V (the estimate or the caller's at i = 0, then the previous iteration's outputs):
//     g   = 3 x 3 average of V at spacing 1, weights k3[dy+1] k3[dx+1], k3 = (1/4, 1/2, 1/4), taps outside the region skipped, the sum
//           divided by the sum of the weights used (no id stop)
//     k_l = 1.f / (sigma_luminance sqrtf(g) + FJ_DN_VAR_EPS);  sigma_luminance <= 0 or +inf: k_l = 0.f, the term is off
//     e   = fabsf(l_q - l_p) k_l + d2n k_n + d2x k_x
//     w   = (h[dy+2] h[dx+2]) expf(-e)
//     sum += w C_q (four channels), wsum += w, vsum += (w w) V_q;     C' = sum / wsum,  V' = vsum / (wsum wsum)
#ifndef FJGPU_DENOISE_VAR_MATH_H
#define FJGPU_DENOISE_VAR_MATH_H

#include "fjgpu_denoise_math.h"

#define FJ_DN_VAR_EPS 1e-6f
#define FJ_DN_VAR_RADIUS 3          // the estimate's window: 7 x 7 taps

FJ_DN_FN float fj_dnv_luminance(float r, float g, float b)
{
  return 0.2126f * r + 0.7152f * g + 0.0722f * b;
}

// ---- the estimate.  A pixel is the guide record of DnPixel with its luminance in `pad`; the colour members are not read.
FJ_DN_FN float fj_dnv_guide_weight(const DnPixel &p, const DnPixel &q, const DnConst &k)
{
  const float d2n = fj_dn_dist2(p.nx, p.ny, p.nz, q.nx, q.ny, q.nz);
  const float d2x = fj_dn_dist2(p.px, p.py, p.pz, q.px, q.py, q.pz);
  return expf(-(d2n * k.kn + d2x * k.kx));
}

FJ_DN_FN void fj_dnv_mean_tap(float &s0, float &s1, const DnPixel &p, const DnPixel &q, const DnConst &k, int stop_at_ids)
{
  if (stop_at_ids && q.id != p.id) return;
  const float w = fj_dnv_guide_weight(p, q, k);
  s0 += w;
  s1 += w * q.pad;
}

FJ_DN_FN void fj_dnv_var_tap(float &s2, float m, const DnPixel &p, const DnPixel &q, const DnConst &k, int stop_at_ids)
{
  if (stop_at_ids && q.id != p.id) return;
  const float w = fj_dnv_guide_weight(p, q, k);
  const float d = q.pad - m;
  s2 += w * (d * d);
}

FJ_DN_FN float fj_dnv_variance(float s2, float s0)
{
  const float v = s2 / s0;
  return v > 0.f ? v : 0.f;
}

// ---- the iterations
FJ_DN_FN float fj_dnv_k3(int k) { return k == 1 ? 0.5f : 0.25f; }

// one tap of g that is inside the region
FJ_DN_FN void fj_dnv_g_tap(float &gs, float &gw, int dx, int dy, float vq)
{
  const float wt = fj_dnv_k3(dy + 1) * fj_dnv_k3(dx + 1);
  gs += wt * vq;
  gw += wt;
}

FJ_DN_FN float fj_dnv_kl(float sigma_luminance, float g)
{
  if (!(sigma_luminance > 0.f) || sigma_luminance == INFINITY) return 0.f;
  return 1.f / (sigma_luminance * sqrtf(g) + FJ_DN_VAR_EPS);
}

// the running sums of one pixel
struct DnvAccum { float r, g, b, a, w, v; };

FJ_DN_FN void fj_dnv_clear(DnvAccum &s) { s.r = s.g = s.b = s.a = s.w = s.v = 0.f; }

// one tap that is inside the region: lp = l(C_p), vq = V_q, kl = k_l of the centre
FJ_DN_FN void fj_dnv_tap(DnvAccum &s, int dx, int dy, const DnPixel &p, float lp, const DnPixel &q, float vq, float kl, const DnConst &k,
    int stop_at_ids)
{
  if (stop_at_ids && q.id != p.id) return;
  const float lq = fj_dnv_luminance(q.r, q.g, q.b);
  const float d2n = fj_dn_dist2(p.nx, p.ny, p.nz, q.nx, q.ny, q.nz);
  const float d2x = fj_dn_dist2(p.px, p.py, p.pz, q.px, q.py, q.pz);
  const float e = fabsf(lq - lp) * kl + d2n * k.kn + d2x * k.kx;
  const float w = (fj_dn_h(dy + 2) * fj_dn_h(dx + 2)) * expf(-e);
  s.r += w * q.r; s.g += w * q.g; s.b += w * q.b; s.a += w * q.a;
  s.w += w;
  s.v += (w * w) * vq;
}

FJ_DN_FN float fj_dnv_variance_out(const DnvAccum &s) { return s.v / (s.w * s.w); }

#endif
