// fjgpu_denoise_variance.hip -- the kernels of fjgpu_denoise_estimate_variance and fjgpu_denoise_variance (include/fjgpu.h): a spatial
// variance estimate of a beauty frame's luminance under the AOV guides, and the a-trous iterations whose luminance term is scaled by the local
// standard deviation and which filter the variance along with the colour.  The arithmetic is fjgpu_denoise_var_math.h, the same source the
// host twin of the CPU tests compiles; this file is the data movement around it.  Blocks of 64 x 4 pixels, one pixel per lane, a wave = 64
// consecutive pixels of one row (the shape of k_dn_atrous); no atomics, no scratch memory; a block talks to no other.
//
//   k_dn_pack_var    k_dn_pack's 32-byte guide record with the luminance of the pixel's colour in the record's pad slot.
//   k_dn_variance    the estimate: 49 taps in two passes (mean, then squared deviations with the same weights) from an LDS-staged footprint
//                    of the block, halo 3: 70 x 10 guide records as two planes of 16-byte slots, consecutive lanes on consecutive slots.
//   k_dn_atrous_var  one launch per iteration, every spacing from global memory: colour, guide record and one f32 of the ping-ponged
//                    variance plane per tap, the 3 x 3 variance average of the centre in front.  Writes colour and variance.
//   k_dn_atrous_var_tile<S>  the iterations of spacing S = 1 and 2 from an LDS-staged footprint, k_dn_atrous_tile's layout with the variance
//                    as a fourth plane of 4-byte slots (profiles/denoise_variance.txt: what it saves).  Same statements per tap, same order: same bits.
#include <hip/hip_runtime.h>

#include "fjgpu_denoise_variance.h"

namespace {

#define FJ_GLOBAL __attribute__((address_space(1)))
#define FJ_LDS __attribute__((address_space(3)))
typedef float dn_v4f __attribute__((ext_vector_type(4)));

constexpr int DN_BX = 64, DN_BY = 4;
constexpr int VR = FJ_DN_VAR_RADIUS;
constexpr int VTW = DN_BX + 2 * VR, VTH = DN_BY + 2 * VR;       // 70 x 10

// the iterations of spacing 1 and 2 from an LDS-staged tile (EXTRA=-DFJ_DNV_LDS_TILE=0: every iteration through k_dn_atrous_var, same bits)
#ifndef FJ_DNV_LDS_TILE
#define FJ_DNV_LDS_TILE 1
#endif

__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_pack_var(const float *color_, int color_stride, const float *normal_,
    const float *position_, const int32_t *ids_, int xres, int xmin, int ymin, int w, int h, float *guide_)
{
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const FJ_GLOBAL dn_v4f *color = (const FJ_GLOBAL dn_v4f *) color_;
  const FJ_GLOBAL float *normal = (const FJ_GLOBAL float *) normal_;
  const FJ_GLOBAL float *position = (const FJ_GLOBAL float *) position_;
  const FJ_GLOBAL int32_t *ids = (const FJ_GLOBAL int32_t *) ids_;
  FJ_GLOBAL dn_v4f *guide = (FJ_GLOBAL dn_v4f *) guide_;
  const size_t at = (size_t) (ymin + y) * (size_t) xres + (size_t) (xmin + x);
  const dn_v4f c = color[(size_t) y * (size_t) color_stride + (size_t) x];
  dn_v4f a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
  if (normal) { a.x = normal[3 * at]; a.y = normal[3 * at + 1]; a.z = normal[3 * at + 2]; }
  if (ids) a.w = __int_as_float(ids[4 * at]);
  if (position) { b.x = position[3 * at]; b.y = position[3 * at + 1]; b.z = position[3 * at + 2]; }
  b.w = fj_dnv_luminance(c.x, c.y, c.z);
  const size_t to = (size_t) y * (size_t) w + (size_t) x;
  guide[2 * to] = a;
  guide[2 * to + 1] = b;
}

__device__ __forceinline__ DnPixel dnv_record(const dn_v4f a, const dn_v4f b)
{
  DnPixel p;
  p.r = p.g = p.b = p.a = 0.f;
  p.nx = a.x; p.ny = a.y; p.nz = a.z; p.id = __float_as_int(a.w);
  p.px = b.x; p.py = b.y; p.pz = b.z; p.pad = b.w;
  return p;
}

__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_variance(const float *guide_, float *var_, int var_stride, int w, int h,
    int stop_at_ids, DnConst k)
{
  __shared__ dn_v4f s_a_[VTW * VTH], s_b_[VTW * VTH];
  FJ_LDS dn_v4f *s_a = (FJ_LDS dn_v4f *) s_a_;
  FJ_LDS dn_v4f *s_b = (FJ_LDS dn_v4f *) s_b_;
  const FJ_GLOBAL dn_v4f *guide = (const FJ_GLOBAL dn_v4f *) guide_;
  FJ_GLOBAL float *var = (FJ_GLOBAL float *) var_;
  const int x0 = blockIdx.x * DN_BX - VR, y0 = blockIdx.y * DN_BY - VR;
  for (int i = threadIdx.y * DN_BX + threadIdx.x; i < VTW * VTH; i += DN_BX * DN_BY) {
    const int gx = x0 + i % VTW, gy = y0 + i / VTW;
    if (gx < 0 || gx >= w || gy < 0 || gy >= h) continue;      // (never read: the taps test the same coordinates)
    const size_t g = (size_t) gy * (size_t) w + (size_t) gx;
    s_a[i] = guide[2 * g];
    s_b[i] = guide[2 * g + 1];
  }
  __syncthreads();
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const int ci = (threadIdx.y + VR) * VTW + threadIdx.x + VR;
  const DnPixel p = dnv_record(s_a[ci], s_b[ci]);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int dy = -VR; dy <= VR; dy++) {
    const int qy = y + dy;
    if (qy < 0 || qy >= h) continue;             // uniform over the wave: a wave is one row
#pragma unroll
    for (int dx = -VR; dx <= VR; dx++) {
      const int qx = x + dx;
      if (qx < 0 || qx >= w) continue;
      const int qi = ci + dy * VTW + dx;
      fj_dnv_mean_tap(s0, s1, p, dnv_record(s_a[qi], s_b[qi]), k, stop_at_ids);
    }
  }
  const float m = s1 / s0;
#pragma unroll
  for (int dy = -VR; dy <= VR; dy++) {
    const int qy = y + dy;
    if (qy < 0 || qy >= h) continue;
#pragma unroll
    for (int dx = -VR; dx <= VR; dx++) {
      const int qx = x + dx;
      if (qx < 0 || qx >= w) continue;
      const int qi = ci + dy * VTW + dx;
      fj_dnv_var_tap(s2, m, p, dnv_record(s_a[qi], s_b[qi]), k, stop_at_ids);
    }
  }
  var[(size_t) y * (size_t) var_stride + (size_t) x] = fj_dnv_variance(s2, s0);
}

__device__ __forceinline__ DnPixel dnv_load(const FJ_GLOBAL dn_v4f *src, size_t at, const FJ_GLOBAL dn_v4f *guide, size_t g)
{
  const dn_v4f c = src[at], a = guide[2 * g], b = guide[2 * g + 1];
  DnPixel p;
  p.r = c.x; p.g = c.y; p.b = c.z; p.a = c.w;
  p.nx = a.x; p.ny = a.y; p.nz = a.z; p.id = __float_as_int(a.w);
  p.px = b.x; p.py = b.y; p.pz = b.z; p.pad = 0.f;
  return p;
}

__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_atrous_var(const float *src_, int src_stride, const float *guide_, const float *vin_,
    int vin_stride, float *dst_, int dst_stride, float *vout_, int vout_stride, int w, int h, int spacing, int stop_at_ids,
    float sigma_luminance, DnConst k)
{
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const FJ_GLOBAL dn_v4f *src = (const FJ_GLOBAL dn_v4f *) src_;
  const FJ_GLOBAL dn_v4f *guide = (const FJ_GLOBAL dn_v4f *) guide_;
  const FJ_GLOBAL float *vin = (const FJ_GLOBAL float *) vin_;
  FJ_GLOBAL dn_v4f *dst = (FJ_GLOBAL dn_v4f *) dst_;
  FJ_GLOBAL float *vout = (FJ_GLOBAL float *) vout_;
  float gs = 0.f, gw = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = y + dy;
    if (qy < 0 || qy >= h) continue;             // uniform over the wave: a wave is one row
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = x + dx;
      if (qx < 0 || qx >= w) continue;
      fj_dnv_g_tap(gs, gw, dx, dy, vin[(size_t) qy * (size_t) vin_stride + (size_t) qx]);
    }
  }
  const float kl = fj_dnv_kl(sigma_luminance, gs / gw);
  const DnPixel p = dnv_load(src, (size_t) y * (size_t) src_stride + (size_t) x, guide, (size_t) y * (size_t) w + (size_t) x);
  const float lp = fj_dnv_luminance(p.r, p.g, p.b);
  DnvAccum s;
  fj_dnv_clear(s);
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + spacing * dy;
    if (qy < 0 || qy >= h) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + spacing * dx;
      if (qx < 0 || qx >= w) continue;
      const DnPixel q = dnv_load(src, (size_t) qy * (size_t) src_stride + (size_t) qx, guide, (size_t) qy * (size_t) w + (size_t) qx);
      fj_dnv_tap(s, dx, dy, p, lp, q, vin[(size_t) qy * (size_t) vin_stride + (size_t) qx], kl, k, stop_at_ids);
    }
  }
  dn_v4f o;
  o.x = s.r / s.w; o.y = s.g / s.w; o.z = s.b / s.w; o.w = s.a / s.w;
  dst[(size_t) y * (size_t) dst_stride + (size_t) x] = o;
  vout[(size_t) y * (size_t) vout_stride + (size_t) x] = fj_dnv_variance_out(s);
}

#if FJ_DNV_LDS_TILE
// The same iteration for spacing S = 1 or 2 with the block's footprint -- (64 + 4 S) x (4 + 4 S) pixels: colour and both guide halves as three
// planes of 16-byte slots, the variance as a plane of 4-byte slots -- staged in LDS.  The 3 x 3 average of the centre's variance reads the same
// plane (halo 2 S >= 1).
template <int S>
__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_atrous_var_tile(const float *src_, int src_stride, const float *guide_, const float *vin_,
    int vin_stride, float *dst_, int dst_stride, float *vout_, int vout_stride, int w, int h, int stop_at_ids, float sigma_luminance, DnConst k)
{
  constexpr int TW = DN_BX + 4 * S, TH = DN_BY + 4 * S;
  __shared__ dn_v4f s_c_[TH * TW], s_a_[TH * TW], s_b_[TH * TW];
  __shared__ float s_v_[TH * TW];
  FJ_LDS dn_v4f *s_c = (FJ_LDS dn_v4f *) s_c_;
  FJ_LDS dn_v4f *s_a = (FJ_LDS dn_v4f *) s_a_;
  FJ_LDS dn_v4f *s_b = (FJ_LDS dn_v4f *) s_b_;
  FJ_LDS float *s_v = (FJ_LDS float *) s_v_;
  const FJ_GLOBAL dn_v4f *src = (const FJ_GLOBAL dn_v4f *) src_;
  const FJ_GLOBAL dn_v4f *guide = (const FJ_GLOBAL dn_v4f *) guide_;
  const FJ_GLOBAL float *vin = (const FJ_GLOBAL float *) vin_;
  FJ_GLOBAL dn_v4f *dst = (FJ_GLOBAL dn_v4f *) dst_;
  FJ_GLOBAL float *vout = (FJ_GLOBAL float *) vout_;
  const int x0 = blockIdx.x * DN_BX - 2 * S, y0 = blockIdx.y * DN_BY - 2 * S;
  for (int i = threadIdx.y * DN_BX + threadIdx.x; i < TW * TH; i += DN_BX * DN_BY) {
    const int gx = x0 + i % TW, gy = y0 + i / TW;
    if (gx < 0 || gx >= w || gy < 0 || gy >= h) continue;      // (never read: the taps test the same coordinates)
    const size_t g = (size_t) gy * (size_t) w + (size_t) gx;
    s_c[i] = src[(size_t) gy * (size_t) src_stride + (size_t) gx];
    s_a[i] = guide[2 * g];
    s_b[i] = guide[2 * g + 1];
    s_v[i] = vin[(size_t) gy * (size_t) vin_stride + (size_t) gx];
  }
  __syncthreads();
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  auto at = [&](int i) {
    const dn_v4f c = s_c[i], a = s_a[i], b = s_b[i];
    DnPixel p;
    p.r = c.x; p.g = c.y; p.b = c.z; p.a = c.w;
    p.nx = a.x; p.ny = a.y; p.nz = a.z; p.id = __float_as_int(a.w);
    p.px = b.x; p.py = b.y; p.pz = b.z; p.pad = 0.f;
    return p;
  };
  const int ci = (threadIdx.y + 2 * S) * TW + threadIdx.x + 2 * S;
  float gs = 0.f, gw = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = y + dy;
    if (qy < 0 || qy >= h) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = x + dx;
      if (qx < 0 || qx >= w) continue;
      fj_dnv_g_tap(gs, gw, dx, dy, s_v[ci + dy * TW + dx]);
    }
  }
  const float kl = fj_dnv_kl(sigma_luminance, gs / gw);
  const DnPixel p = at(ci);
  const float lp = fj_dnv_luminance(p.r, p.g, p.b);
  DnvAccum s;
  fj_dnv_clear(s);
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + S * dy;
    if (qy < 0 || qy >= h) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + S * dx;
      if (qx < 0 || qx >= w) continue;
      const int qi = ci + S * dy * TW + S * dx;
      fj_dnv_tap(s, dx, dy, p, lp, at(qi), s_v[qi], kl, k, stop_at_ids);
    }
  }
  dn_v4f o;
  o.x = s.r / s.w; o.y = s.g / s.w; o.z = s.b / s.w; o.w = s.a / s.w;
  dst[(size_t) y * (size_t) dst_stride + (size_t) x] = o;
  vout[(size_t) y * (size_t) vout_stride + (size_t) x] = fj_dnv_variance_out(s);
}
#endif

bool dnv_grid(int w, int h, dim3 *grid)
{
  *grid = dim3((w + DN_BX - 1) / DN_BX, (h + DN_BY - 1) / DN_BY);
  return grid->y <= 65535u;      // (blocks of rows are grid.y: the entry points refuse a taller region)
}

}  // namespace

int launch_dn_pack_var(hipStream_t st, const float *color, int color_stride, const float *normal, const float *position, const int32_t *ids,
    int xres, int xmin, int ymin, int w, int h, float *guide)
{
  if (w <= 0 || h <= 0) return 0;
  dim3 grid;
  if (!dnv_grid(w, h, &grid)) return (int) hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_dn_pack_var, grid, dim3(DN_BX, DN_BY), 0, st, color, color_stride, normal, position, ids, xres, xmin, ymin, w, h, guide);
  return (int) hipGetLastError();
}

int launch_dn_variance(hipStream_t st, const float *guide, float *variance, int variance_stride, int w, int h, int stop_at_ids, DnConst k)
{
  if (w <= 0 || h <= 0) return 0;
  dim3 grid;
  if (!dnv_grid(w, h, &grid)) return (int) hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_dn_variance, grid, dim3(DN_BX, DN_BY), 0, st, guide, variance, variance_stride, w, h, stop_at_ids, k);
  return (int) hipGetLastError();
}

int launch_dn_atrous_var(hipStream_t st, const float *src, int src_stride, const float *guide, const float *vin, int vin_stride,
    float *dst, int dst_stride, float *vout, int vout_stride, int w, int h, int spacing, int stop_at_ids, float sigma_luminance, DnConst k)
{
  if (w <= 0 || h <= 0) return 0;
  dim3 grid;
  if (!dnv_grid(w, h, &grid)) return (int) hipErrorInvalidConfiguration;
#if FJ_DNV_LDS_TILE
  if (spacing == 1)
    hipLaunchKernelGGL(k_dn_atrous_var_tile<1>, grid, dim3(DN_BX, DN_BY), 0, st, src, src_stride, guide, vin, vin_stride, dst, dst_stride, vout,
                       vout_stride, w, h, stop_at_ids, sigma_luminance, k);
  else if (spacing == 2)
    hipLaunchKernelGGL(k_dn_atrous_var_tile<2>, grid, dim3(DN_BX, DN_BY), 0, st, src, src_stride, guide, vin, vin_stride, dst, dst_stride, vout,
                       vout_stride, w, h, stop_at_ids, sigma_luminance, k);
  else
#endif
  hipLaunchKernelGGL(k_dn_atrous_var, grid, dim3(DN_BX, DN_BY), 0, st, src, src_stride, guide, vin, vin_stride, dst, dst_stride, vout,
                     vout_stride, w, h, spacing, stop_at_ids, sigma_luminance, k);
  return (int) hipGetLastError();
}
