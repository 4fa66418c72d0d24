// denoise_variance_host.cc -- validation tool: fjgpu_denoise_estimate_variance and fjgpu_denoise_variance (include/fjgpu.h) as plain loops
// over HOST arrays, every tap through device/fjgpu_denoise_var_math.h -- the SAME source k_dn_variance and k_dn_atrous_var compile -- so that
// tests/test_denoise_variance_cpu.py can hold the arithmetic against its numpy restatement without a GPU.  Built with the ROCm clang++ under
// -ffp-contract=off.  Not part of the product path.
#include <stdint.h>
#include <math.h>
#include <vector>

#include "fjgpu.h"
#include "fjgpu_denoise_var_math.h"

namespace {

bool bad_frame(const fjgpu_denoise_desc *d)
{
  return d->xres <= 0 || d->yres <= 0 || d->region[0] < 0 || d->region[1] < 0 || d->region[2] > d->xres || d->region[3] > d->yres ||
         d->region[0] >= d->region[2] || d->region[1] >= d->region[3];
}

// the region as the kernels' taps see it: colour and guide record per pixel, the colour's luminance in `pad`
std::vector<DnPixel> gather(const fjgpu_denoise_desc *d, const float *color, const float *normal, const float *position, const int32_t *ids)
{
  const int x0 = d->region[0], y0 = d->region[1], w = d->region[2] - x0, h = d->region[3] - y0;
  std::vector<DnPixel> px((size_t) w * h);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const size_t at = (size_t) (y0 + y) * d->xres + (x0 + x);
      DnPixel &p = px[(size_t) y * w + x];
      p.r = color[4 * at]; p.g = color[4 * at + 1]; p.b = color[4 * at + 2]; p.a = color[4 * at + 3];
      p.nx = normal ? normal[3 * at] : 0.f; p.ny = normal ? normal[3 * at + 1] : 0.f; p.nz = normal ? normal[3 * at + 2] : 0.f;
      p.px = position ? position[3 * at] : 0.f; p.py = position ? position[3 * at + 1] : 0.f; p.pz = position ? position[3 * at + 2] : 0.f;
      p.id = ids ? ids[4 * at] : 0;
      p.pad = fj_dnv_luminance(p.r, p.g, p.b);
    }
  return px;
}

// the estimate over gathered pixels -> V [h][w]
std::vector<float> estimate(const std::vector<DnPixel> &px, int w, int h, const DnConst &k, int stop)
{
  const int R = FJ_DN_VAR_RADIUS;
  std::vector<float> V((size_t) w * h);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const DnPixel &p = px[(size_t) y * w + x];
      float s0 = 0.f, s1 = 0.f, s2 = 0.f;
      for (int dy = -R; dy <= R; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -R; dx <= R; dx++) {
          const int qx = x + dx;
          if (qx < 0 || qx >= w) continue;
          fj_dnv_mean_tap(s0, s1, p, px[(size_t) qy * w + qx], k, stop);
        }
      }
      const float m = s1 / s0;
      for (int dy = -R; dy <= R; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -R; dx <= R; dx++) {
          const int qx = x + dx;
          if (qx < 0 || qx >= w) continue;
          fj_dnv_var_tap(s2, m, p, px[(size_t) qy * w + qx], k, stop);
        }
      }
      V[(size_t) y * w + x] = fj_dnv_variance(s2, s0);
    }
  return V;
}

}  // namespace

extern "C" {

// the arguments of fjgpu_denoise_estimate_variance on host memory; 0, or -2 (FJGPU_EINVAL) for what it refuses
int fj_denoise_estimate_variance_host(const fjgpu_denoise_desc *d, const float *color, const float *normal, const float *position,
    const int32_t *ids, float *variance_out)
{
  if (!d || !color || !variance_out) return FJGPU_EINVAL;
  if (bad_frame(d)) return FJGPU_EINVAL;
  if (isnan(d->sigma_color) || isnan(d->sigma_normal) || isnan(d->sigma_position)) return FJGPU_EINVAL;
  const int x0 = d->region[0], y0 = d->region[1], w = d->region[2] - x0, h = d->region[3] - y0;
  const int stop = (d->stop_at_ids && ids) ? 1 : 0;
  const DnConst k = fj_dn_constants(0.f, normal ? d->sigma_normal : 0.f, position ? d->sigma_position : 0.f, 0);
  const std::vector<float> V = estimate(gather(d, color, normal, position, ids), w, h, k, stop);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) variance_out[(size_t) (y0 + y) * d->xres + (x0 + x)] = V[(size_t) y * w + x];
  return 0;
}

// the arguments of fjgpu_denoise_variance on host memory (variance_out may be NULL)
int fj_denoise_variance_host(const fjgpu_denoise_desc *d, float sigma_luminance, const float *color_in, const float *normal,
    const float *position, const int32_t *ids, const float *albedo, float albedo_floor, const float *variance_in, float *color_out,
    float *variance_out)
{
  if (albedo && !(isfinite(albedo_floor) && albedo_floor > 0)) return FJGPU_EINVAL;
  if (!d || !color_in || !color_out) return FJGPU_EINVAL;
  if (bad_frame(d)) return FJGPU_EINVAL;
  if (d->iterations < 1 || d->iterations > FJ_DN_MAX_ITERATIONS) return FJGPU_EINVAL;
  if (isnan(d->sigma_color) || isnan(d->sigma_normal) || isnan(d->sigma_position) || isnan(sigma_luminance)) return FJGPU_EINVAL;
  if (variance_out && (variance_out == variance_in || variance_out == color_in || variance_out == color_out)) return FJGPU_EINVAL;
  const int x0 = d->region[0], y0 = d->region[1], w = d->region[2] - x0, h = d->region[3] - y0;
  const int stop = (d->stop_at_ids && ids) ? 1 : 0;
  const DnConst k = fj_dn_constants(0.f, normal ? d->sigma_normal : 0.f, position ? d->sigma_position : 0.f, 0);

  // demodulated copy of the frame's region (albedo NULL: the frame itself)
  std::vector<float> dem;
  const float *src = color_in;
  if (albedo) {
    dem.assign((size_t) d->xres * d->yres * 4, 0.f);
    for (int y = y0; y < y0 + h; y++)
      for (int x = x0; x < x0 + w; x++) {
        const size_t at = (size_t) y * d->xres + x;
        for (int c = 0; c < 3; c++) dem[4 * at + c] = fj_dn_demodulate(color_in[4 * at + c], fj_dn_albedo_clamp(albedo[3 * at + c], albedo_floor));
        dem[4 * at + 3] = color_in[4 * at + 3];
      }
    src = dem.data();
  }
  std::vector<DnPixel> cur = gather(d, src, normal, position, ids), nxt;
  std::vector<float> V, Vn((size_t) w * h);
  if (variance_in) {
    V.resize((size_t) w * h);
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) V[(size_t) y * w + x] = variance_in[(size_t) (y0 + y) * d->xres + (x0 + x)];
  } else {
    V = estimate(cur, w, h, k, stop);
  }
  nxt = cur;
  for (int i = 0; i < d->iterations; i++) {
    const int s = 1 << i;
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        const DnPixel &p = cur[(size_t) y * w + x];
        float gs = 0.f, gw = 0.f;
        for (int dy = -1; dy <= 1; dy++) {
          const int qy = y + dy;
          if (qy < 0 || qy >= h) continue;
          for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= w) continue;
            fj_dnv_g_tap(gs, gw, dx, dy, V[(size_t) qy * w + qx]);
          }
        }
        const float kl = fj_dnv_kl(sigma_luminance, gs / gw);
        const float lp = fj_dnv_luminance(p.r, p.g, p.b);
        DnvAccum a;
        fj_dnv_clear(a);
        for (int dy = -2; dy <= 2; dy++) {
          const int qy = y + s * dy;
          if (qy < 0 || qy >= h) continue;
          for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= w) continue;
            fj_dnv_tap(a, dx, dy, p, lp, cur[(size_t) qy * w + qx], V[(size_t) qy * w + qx], kl, k, stop);
          }
        }
        DnPixel &o = nxt[(size_t) y * w + x];
        o.r = a.r / a.w; o.g = a.g / a.w; o.b = a.b / a.w; o.a = a.a / a.w;
        Vn[(size_t) y * w + x] = fj_dnv_variance_out(a);
      }
    cur.swap(nxt);
    V.swap(Vn);
  }
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const size_t at = (size_t) (y0 + y) * d->xres + (x0 + x);
      const DnPixel &p = cur[(size_t) y * w + x];
      color_out[4 * at] = p.r; color_out[4 * at + 1] = p.g; color_out[4 * at + 2] = p.b; color_out[4 * at + 3] = p.a;
      if (albedo)
        for (int c = 0; c < 3; c++) color_out[4 * at + c] = fj_dn_remodulate(color_out[4 * at + c], fj_dn_albedo_clamp(albedo[3 * at + c], albedo_floor));
      if (variance_out) variance_out[(size_t) (y0 + y) * d->xres + (x0 + x)] = V[(size_t) y * w + x];
    }
  return 0;
}

// k_l as the kernel computes it from sigma_luminance and the pixel's g
float fj_denoise_variance_host_kl(float sigma_luminance, float g) { return fj_dnv_kl(sigma_luminance, g); }

// l(C) as the kernels compute it
float fj_denoise_variance_host_luminance(float r, float g, float b) { return fj_dnv_luminance(r, g, b); }

}
