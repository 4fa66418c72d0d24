// fjgpu_sample_variance.hip -- the kernel of fjgpu_render_tiles_variance (include/fjgpu.h): the variance of every pixel's filtered estimate
// from the per-sample radiances the beauty pass holds when it resolves a batch.  The arithmetic is fjgpu_sample_var_math.h, the same source
// the host twin of the CPU tests compiles; this file is the data movement around it.
//
//   k_sample_variance  k_resolve's sibling (fjgpu_kernels.hip) on k_resolve's grid: one wave per pixel, the lanes take the npx_x * npx_y
//                      samples of the pixel's window in row-major order, so a load instruction reads whole window rows -- 16 bytes of (u, v)
//                      and 16 bytes of radiance per lane.  Two passes (mean, then squared deviations and squared weights with the same
//                      weights), each reduced by an f64 butterfly that leaves the same bits in every lane.  A window of up to 64 samples
//                      keeps its lane's weight and luminance in registers between the passes; a larger one reads its samples again.  Lane 0
//                      writes one float.  No LDS, no atomics, no scratch memory; a wave talks to no other.
#include <hip/hip_runtime.h>

#include "fjgpu_sample_variance.h"
#include "fjgpu_sample_var_math.h"

namespace {

constexpr int SV_BLOCK = 256;

__device__ __forceinline__ double sv_wave_sum(double x)
{
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

__global__ void __launch_bounds__(SV_BLOCK) k_sample_variance(ResolveParams rp, const TileDesc *tiles, const double *s_uv,
    const float4 *s_accum, const float *albedo, float albedo_floor, float *variance)
{
  const TileDesc T = tiles[blockIdx.y];
  const int tw = T.xmax - T.xmin, th = T.ymax - T.ymin;
  const int k = blockIdx.x * (SV_BLOCK / 64) + (threadIdx.x >> 6);     // pixel of this wave
  if (k >= tw * th) return;
  const unsigned lane = __lane_id();
  const int px = T.xmin + k % tw, py = T.ymin + k / tw;
  const size_t at = (size_t) py * rp.xres + px;
  const size_t base = (size_t) T.sample_offset + (size_t) (py - T.ymin) * rp.rate_y * T.nx + (size_t) (px - T.xmin) * rp.rate_x;
  const int nwin = rp.npx_x * rp.npx_y;
  SvFrame f;
  f.xres = rp.xres; f.yres = rp.yres; f.rate_x = rp.rate_x; f.rate_y = rp.rate_y; f.npx_x = rp.npx_x; f.npx_y = rp.npx_y;
  f.fw = rp.fw; f.fh = rp.fh;
  float a[3] = {0.f, 0.f, 0.f};
  if (albedo)
    for (int c = 0; c < 3; c++) a[c] = fj_dn_albedo_clamp(albedo[3 * at + c], albedo_floor);
  // sample w of the window: its weight and its luminance
  auto sample = [&](int w, double &wgt, double &lum) {
    const int sy = w / rp.npx_x, sx = w - sy * rp.npx_x;
    const size_t s = base + (size_t) sy * T.nx + sx;
    const double2 uv = reinterpret_cast<const double2 *>(s_uv)[s];
    const float4 d = s_accum[s];
    wgt = fj_sv_weight(f, px, py, uv.x, uv.y);
    lum = fj_sv_luminance(d.x, d.y, d.z, albedo ? a : nullptr);
  };
  double S0 = 0, S1 = 0, S2 = 0, Q = 0;
  if (nwin <= 64) {                      // (uniform over the grid)
    double wgt = 0, lum = 0;
    const bool mine = (int) lane < nwin;
    if (mine) { sample((int) lane, wgt, lum); fj_sv_pass1(S0, S1, wgt, lum); }
    S0 = sv_wave_sum(S0);
    S1 = sv_wave_sum(S1);
    const double m = S1 / S0;
    if (mine) fj_sv_pass2(S2, Q, wgt, lum, m);
  } else {
    for (int w = (int) lane; w < nwin; w += 64) {
      double wgt, lum;
      sample(w, wgt, lum);
      fj_sv_pass1(S0, S1, wgt, lum);
    }
    S0 = sv_wave_sum(S0);
    S1 = sv_wave_sum(S1);
    const double m = S1 / S0;
    for (int w = (int) lane; w < nwin; w += 64) {
      double wgt, lum;
      sample(w, wgt, lum);
      fj_sv_pass2(S2, Q, wgt, lum, m);
    }
  }
  S2 = sv_wave_sum(S2);
  Q = sv_wave_sum(Q);
  if (lane == 0) variance[at] = fj_sv_result(S0, S2, Q);
}

}  // namespace

int launch_sample_variance(hipStream_t st, const ResolveParams &rp, const TileDesc *d_tiles, int n_tiles, int max_tile_pixels,
    const double *s_uv, const float *s_accum, const float *albedo, float albedo_floor, float *variance)
{
  if (n_tiles <= 0 || max_tile_pixels <= 0) return 0;
  const dim3 grid((max_tile_pixels + SV_BLOCK / 64 - 1) / (SV_BLOCK / 64), n_tiles);      // k_resolve's grid: one wave per pixel
  hipLaunchKernelGGL(k_sample_variance, grid, dim3(SV_BLOCK), 0, st, rp, d_tiles, s_uv, reinterpret_cast<const float4 *>(s_accum), albedo,
                     albedo_floor, variance);
  return (int) hipGetLastError();
}
