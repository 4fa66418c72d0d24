// sample_variance_host.cc -- validation tool: the variance pass of fjgpu_render_tiles_variance (include/fjgpu.h) as a plain loop over HOST
// arrays of samples, every pixel through fj_sv_pixel of device/fjgpu_sample_var_math.h -- the header k_sample_variance compiles -- so that
// tests/test_sample_variance_cpu.py can hold the arithmetic against its numpy restatement without a GPU.  Built with the ROCm clang++ under
// -ffp-contract=off.  Not part of the product path.
#include <stdint.h>
#include <math.h>

#include "fjgpu.h"
#include "fjgpu_sample_var_math.h"

extern "C" {

// what k_sample_variance reads of ResolveParams (fjgpu_kernels.h) ...
struct fj_sv_host_frame {
  int32_t xres, yres, rate_x, rate_y, npx_x, npx_y;
  double fw, fh;
};

// ... and of one TileDesc: the pixel rectangle, the samples per row and the tile's first sample slot in s_uv / s_accum
struct fj_sv_host_tile {
  int32_t xmin, ymin, xmax, ymax;
  int32_t nx, ny;
  uint32_t sample_offset;
  int32_t pad;
};

// the variance of the pixels of n_tiles tiles: s_uv [.][2] f64 and s_accum [.][4] f32 as the beauty pass holds them at its resolve; albedo
// [yres][xres][3] or NULL; variance [yres][xres], pixels outside the tiles untouched.  0, or -2 (FJGPU_EINVAL) for what the entry point refuses
// and for a tile whose window would leave its samples.
int fj_sample_variance_host(const fj_sv_host_frame *frame, const fj_sv_host_tile *tiles, int n_tiles, const double *s_uv, const float *s_accum,
    const float *albedo, float albedo_floor, float *variance)
{
  if (!frame || !tiles || !s_uv || !s_accum || !variance) return FJGPU_EINVAL;
  if (albedo && !(isfinite(albedo_floor) && albedo_floor > 0)) return FJGPU_EINVAL;
  SvFrame f;
  f.xres = frame->xres; f.yres = frame->yres; f.rate_x = frame->rate_x; f.rate_y = frame->rate_y; f.npx_x = frame->npx_x; f.npx_y = frame->npx_y;
  f.fw = frame->fw; f.fh = frame->fh;
  if (f.xres <= 0 || f.yres <= 0 || f.rate_x <= 0 || f.rate_y <= 0 || f.npx_x <= 0 || f.npx_y <= 0) return FJGPU_EINVAL;
  for (int t = 0; t < n_tiles; t++) {
    const fj_sv_host_tile &T = tiles[t];
    const int tw = T.xmax - T.xmin, th = T.ymax - T.ymin;
    if (T.xmin < 0 || T.ymin < 0 || T.xmax > f.xres || T.ymax > f.yres || tw <= 0 || th <= 0) return FJGPU_EINVAL;
    if ((tw - 1) * f.rate_x + f.npx_x > T.nx || (th - 1) * f.rate_y + f.npx_y > T.ny) return FJGPU_EINVAL;
    for (int py = T.ymin; py < T.ymax; py++)
      for (int px = T.xmin; px < T.xmax; px++) {
        const size_t at = (size_t) py * f.xres + px;
        const size_t base = (size_t) T.sample_offset + (size_t) (py - T.ymin) * f.rate_y * T.nx + (size_t) (px - T.xmin) * f.rate_x;
        float a[3];
        if (albedo)
          for (int c = 0; c < 3; c++) a[c] = fj_dn_albedo_clamp(albedo[3 * at + c], albedo_floor);
        variance[at] = fj_sv_pixel(f, px, py, base, T.nx, s_uv, s_accum, albedo ? a : nullptr);
      }
  }
  return 0;
}

// the pieces, for the tests that hold the model against them one by one
double fj_sample_variance_host_weight(const fj_sv_host_frame *frame, int px, int py, double u, double v)
{
  SvFrame f;
  f.xres = frame->xres; f.yres = frame->yres; f.rate_x = frame->rate_x; f.rate_y = frame->rate_y; f.npx_x = frame->npx_x; f.npx_y = frame->npx_y;
  f.fw = frame->fw; f.fh = frame->fh;
  return fj_sv_weight(f, px, py, u, v);
}

float fj_sample_variance_host_result(double S0, double S2, double Q) { return fj_sv_result(S0, S2, Q); }

}
