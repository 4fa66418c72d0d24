// denoise_host.cc -- validation tool: the filter of fjgpu_denoise (include/fjgpu.h) as a plain loop over HOST arrays, every tap through
// device/fjgpu_denoise_math.h -- the SAME source k_dn_atrous compiles -- so that tests/test_denoise_cpu.py can hold the arithmetic against
// its numpy restatement without a GPU.  Built with the ROCm clang++ under -ffp-contract=off.  Not part of the product path.
#include <stdint.h>
#include <math.h>
#include <vector>

#include "fjgpu.h"
#include "fjgpu_denoise_math.h"

extern "C" {

// the arguments of fjgpu_denoise on host memory; 0, or -2 (FJGPU_EINVAL) for what fjgpu_denoise refuses
int fj_denoise_host(const fjgpu_denoise_desc *d, const float *color_in, const float *normal, const float *position, const int32_t *ids,
    float *color_out)
{
  if (!d || !color_in || !color_out) return FJGPU_EINVAL;
  if (d->xres <= 0 || d->yres <= 0 || d->region[0] < 0 || d->region[1] < 0 || d->region[2] > d->xres || d->region[3] > d->yres ||
      d->region[0] >= d->region[2] || d->region[1] >= d->region[3])
    return FJGPU_EINVAL;
  if (d->iterations < 1 || d->iterations > FJ_DN_MAX_ITERATIONS) return FJGPU_EINVAL;
  if (isnan(d->sigma_color) || isnan(d->sigma_normal) || isnan(d->sigma_position)) return FJGPU_EINVAL;
  const int x0 = d->region[0], y0 = d->region[1], w = d->region[2] - x0, h = d->region[3] - y0;
  const int stop = (d->stop_at_ids && ids) ? 1 : 0;
  // the region as the kernel's taps see it: colour and guide record per pixel
  std::vector<DnPixel> cur((size_t) w * h), nxt((size_t) w * h);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const size_t at = (size_t) (y0 + y) * d->xres + (x0 + x);
      DnPixel &p = cur[(size_t) y * w + x];
      p.r = color_in[4 * at]; p.g = color_in[4 * at + 1]; p.b = color_in[4 * at + 2]; p.a = color_in[4 * at + 3];
      p.nx = normal ? normal[3 * at] : 0.f; p.ny = normal ? normal[3 * at + 1] : 0.f; p.nz = normal ? normal[3 * at + 2] : 0.f;
      p.px = position ? position[3 * at] : 0.f; p.py = position ? position[3 * at + 1] : 0.f; p.pz = position ? position[3 * at + 2] : 0.f;
      p.id = ids ? ids[4 * at] : 0;
      p.pad = 0.f;
    }
  nxt = cur;
  for (int i = 0; i < d->iterations; i++) {
    const int s = 1 << i;
    const DnConst k = fj_dn_constants(d->sigma_color, normal ? d->sigma_normal : 0.f, position ? d->sigma_position : 0.f, i);
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        const DnPixel &p = cur[(size_t) y * w + x];
        DnAccum a;
        fj_dn_clear(a);
        for (int dy = -2; dy <= 2; dy++) {
          const int qy = y + s * dy;
          if (qy < 0 || qy >= h) continue;
          for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= w) continue;
            fj_dn_tap(a, dx, dy, p, cur[(size_t) qy * w + qx], k, stop);
          }
        }
        DnPixel &o = nxt[(size_t) y * w + x];
        o.r = a.r / a.w; o.g = a.g / a.w; o.b = a.b / a.w; o.a = a.a / a.w;
      }
    cur.swap(nxt);
    // (the guides of nxt are those of cur: both started as the same records, only colours are written)
  }
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const size_t at = (size_t) (y0 + y) * d->xres + (x0 + x);
      const DnPixel &p = cur[(size_t) y * w + x];
      color_out[4 * at] = p.r; color_out[4 * at + 1] = p.g; color_out[4 * at + 2] = p.b; color_out[4 * at + 3] = p.a;
    }
  return 0;
}

// the arguments of fjgpu_denoise_albedo on host memory: the region's rgb divided by the clamped albedo, the loop above, the albedo multiplied
// back -- the three steps through the functions k_dn_demodulate / k_dn_remodulate compile.  albedo NULL: fj_denoise_host.
int fj_denoise_albedo_host(const fjgpu_denoise_desc *d, const float *color_in, const float *normal, const float *position, const int32_t *ids,
    const float *albedo, float albedo_floor, float *color_out)
{
  if (!albedo) return fj_denoise_host(d, color_in, normal, position, ids, color_out);
  if (!(isfinite(albedo_floor) && albedo_floor > 0)) return FJGPU_EINVAL;
  if (!d || !color_in || !color_out) return FJGPU_EINVAL;
  if (d->xres <= 0 || d->yres <= 0 || d->region[0] < 0 || d->region[1] < 0 || d->region[2] > d->xres || d->region[3] > d->yres ||
      d->region[0] >= d->region[2] || d->region[1] >= d->region[3])
    return FJGPU_EINVAL;
  // a frame-sized copy whose region is demodulated (only the region is read by the loop)
  std::vector<float> dem((size_t) d->xres * d->yres * 4);
  for (int y = d->region[1]; y < d->region[3]; y++)
    for (int x = d->region[0]; x < d->region[2]; x++) {
      const size_t at = (size_t) y * d->xres + x;
      for (int k = 0; k < 3; k++) dem[4 * at + k] = fj_dn_demodulate(color_in[4 * at + k], fj_dn_albedo_clamp(albedo[3 * at + k], albedo_floor));
      dem[4 * at + 3] = color_in[4 * at + 3];
    }
  if (const int e = fj_denoise_host(d, dem.data(), normal, position, ids, color_out)) return e;
  for (int y = d->region[1]; y < d->region[3]; y++)
    for (int x = d->region[0]; x < d->region[2]; x++) {
      const size_t at = (size_t) y * d->xres + x;
      for (int k = 0; k < 3; k++) color_out[4 * at + k] = fj_dn_remodulate(color_out[4 * at + k], fj_dn_albedo_clamp(albedo[3 * at + k], albedo_floor));
    }
  return 0;
}

// the constants of iteration i as fjgpu_denoise passes them to the kernel: out[3] = k_c, k_n, k_x
void fj_denoise_host_constants(float sigma_color, float sigma_normal, float sigma_position, int i, float *out)
{
  const DnConst k = fj_dn_constants(sigma_color, sigma_normal, sigma_position, i);
  out[0] = k.kc; out[1] = k.kn; out[2] = k.kx;
}

}
