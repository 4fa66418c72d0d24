// fjgpu_denoise_math.h -- the arithmetic of fjgpu_denoise (include/fjgpu.h): the edge-avoiding a-trous wavelet filter of Dammertz, Sewtz,
// Hanika and Lensch (HPG 2010), one tap at a time.
//
// ONE source for the device kernel (fjgpu_denoise.hip: k_dn_atrous), for the host twin the CPU tests run (tools/denoise_host.cc) and for
// the constants fjgpu_denoise computes on the host: whatever is tested without a GPU is what the kernel compiles.  All of it is f32 under
// -ffp-contract=off, every sum left to right; tests/denoise_model.py restates it in numpy.
//
//   h = (1/16, 1/4, 3/8, 1/4, 1/16), iteration i = 0 .. iterations-1 with tap spacing 2^i; for the pixel p and its tap q
//     d2c = (Cq.r-Cp.r)^2 + (Cq.g-Cp.g)^2 + (Cq.b-Cp.b)^2      (d2n, d2x likewise from normal and position)
//     e   = d2c k_c + d2n k_n + d2x k_x                        (k = 0 for a term that is off)
//     w   = (h[dy+2] h[dx+2]) expf(-e)                         ONE expf per tap, of the summed exponent
//     sum += w Cq (all four channels), wsum += w;  out = sum / wsum  (the centre tap contributes 9/64: wsum > 0)
//   k_c = (float) (1 / (sigma_c 2^-i)^2), k_n = (float) (1 / sigma_n^2), k_x = (float) (1 / sigma_x^2): f64 on the host, rounded once.
#ifndef FJGPU_DENOISE_MATH_H
#define FJGPU_DENOISE_MATH_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define FJ_DN_FN __host__ __device__ __forceinline__
#else
#define FJ_DN_FN static inline
#endif

#define FJ_DN_MAX_ITERATIONS 8

// the constants of one iteration
struct DnConst { float kc, kn, kx; };

// a pixel as a tap sees it: the colour, and the 32-byte guide record k_dn_pack writes (two 16-byte halves)
struct DnPixel {
  float r, g, b, a;
  float nx, ny, nz; int32_t id;
  float px, py, pz; float pad;
};

// B3-spline tap weights; every product h[j] h[i] is exact in f32
FJ_DN_FN float fj_dn_h(int k)
{
  return k == 2 ? 0.375f : ((k == 1 || k == 3) ? 0.25f : 0.0625f);
}

// 1 / sigma^2 as the filter multiplies it; sigma <= 0 or +inf: the term is off (0).  The f64 quotient is capped at FLT_MAX so that
// a tiny sigma cannot turn the centre tap's 0 * k into NaN.  (NaN sigmas are refused before this is called.)
FJ_DN_FN float fj_dn_k(double sigma)
{
  if (!(sigma > 0) || sigma == (double) INFINITY) return 0.f;
  const double k = 1. / (sigma * sigma);
  return (float) (k < 3.4028234663852886e38 ? k : 3.4028234663852886e38);
}

// iteration i: only the colour sigma shrinks, sigma_c 2^-i (the image gets smoother, its edges have to be kept by a tighter term)
FJ_DN_FN DnConst fj_dn_constants(float sigma_color, float sigma_normal, float sigma_position, int i)
{
  DnConst c;
  c.kc = fj_dn_k((double) sigma_color * ldexp(1., -i));
  c.kn = fj_dn_k((double) sigma_normal);
  c.kx = fj_dn_k((double) sigma_position);
  return c;
}

FJ_DN_FN float fj_dn_dist2(float ax, float ay, float az, float bx, float by, float bz)
{
  const float dx = bx - ax, dy = by - ay, dz = bz - az;
  return dx * dx + dy * dy + dz * dz;
}

// weight of the tap q of the pixel p; hw = h[dy+2] * h[dx+2]
FJ_DN_FN float fj_dn_weight(float hw, const DnPixel &p, const DnPixel &q, const DnConst &k)
{
  const float d2c = fj_dn_dist2(p.r, p.g, p.b, q.r, q.g, q.b);
  const float d2n = fj_dn_dist2(p.nx, p.ny, p.nz, q.nx, q.ny, q.nz);
  const float d2x = fj_dn_dist2(p.px, p.py, p.pz, q.px, q.py, q.pz);
  const float e = d2c * k.kc + d2n * k.kn + d2x * k.kx;
  return hw * expf(-e);
}

// the running sums of one pixel
struct DnAccum { float r, g, b, a, w; };

FJ_DN_FN void fj_dn_clear(DnAccum &s) { s.r = s.g = s.b = s.a = s.w = 0.f; }

// one tap that is inside the region; stop_at_ids: a tap of another instance id weighs 0 (it is skipped)
FJ_DN_FN void fj_dn_tap(DnAccum &s, int dx, int dy, const DnPixel &p, const DnPixel &q, const DnConst &k, int stop_at_ids)
{
  if (stop_at_ids && q.id != p.id) return;
  const float w = fj_dn_weight(fj_dn_h(dy + 2) * fj_dn_h(dx + 2), p, q, k);
  s.r += w * q.r; s.g += w * q.g; s.b += w * q.b; s.a += w * q.a;
  s.w += w;
}

// ---- albedo demodulation (fjgpu_denoise_albedo): the filter runs on colour / albedo, the albedo is multiplied back afterwards.  Each of the
// three is ONE correctly rounded f32 operation per value (a NaN albedo takes the floor)
FJ_DN_FN float fj_dn_albedo_clamp(float albedo, float albedo_floor) { return albedo > albedo_floor ? albedo : albedo_floor; }
FJ_DN_FN float fj_dn_demodulate(float c, float a) { return c / a; }
FJ_DN_FN float fj_dn_remodulate(float f, float a) { return f * a; }

#endif
