// fjgpu_denoise.hip -- the kernels of fjgpu_denoise (include/fjgpu.h): an edge-avoiding a-trous wavelet filter over a beauty frame,
// guided by the first-hit AOV pass's normal, position and instance id.  The arithmetic of a tap is fjgpu_denoise_math.h, the same
// source the host twin of the CPU tests compiles; this file is the data movement around it.
//
//   k_dn_pack    one lane per region pixel: normal (12 B), position (12 B) and ids[0] of the caller's frame-sized buffers -> one 32-byte
//                guide record, two 16-byte stores.  A tap of the filter then costs three 16-byte loads (colour, two guide halves),
//                consecutive lanes at consecutive records.
//   k_dn_atrous  one launch per iteration.  Blocks of 64 x 4 pixels, one pixel per lane, a wave = 64 consecutive pixels of one row: a tap
//                row is a contiguous 1 KB colour read (and 2 KB of guide) per wave, and "is this tap row inside the region" is uniform over
//                the wave.  The centre pixel stays in registers.  No atomics, no scratch memory; a block talks to no other.
//   k_dn_atrous_tile<S>  the iterations of spacing S = 1 and 2, whose taps overlap inside a block, from an LDS-staged footprint (half the
//                time of k_dn_atrous at those spacings on an MI355X, profiles/denoise_pass.txt; larger spacings reuse nothing inside a block).
//   k_dn_demodulate, k_dn_remodulate  fjgpu_denoise_albedo: one lane per region pixel, rgb divided by the clamped albedo into a scratch frame
//                before the iterations, multiplied by it in color_out after them.  One frame moved each; not fused into their neighbours.
#include <hip/hip_runtime.h>

#include "fjgpu_denoise.h"

namespace {

// (see fjgpu_dev_math.h: a pointer the compiler takes for generic becomes FLAT loads; these arrays are global memory)
#define FJ_GLOBAL __attribute__((address_space(1)))
typedef float dn_v4f __attribute__((ext_vector_type(4)));

constexpr int DN_BX = 64, DN_BY = 4;

// the iterations of spacing 1 and 2 from an LDS-staged tile (EXTRA=-DFJ_DN_LDS_TILE=0: every iteration through k_dn_atrous, same bits)
#ifndef FJ_DN_LDS_TILE
#define FJ_DN_LDS_TILE 1
#endif

__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_pack(const float *normal_, const float *position_, const int32_t *ids_,
    int xres, int xmin, int ymin, int w, int h, float *guide_)
{
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const FJ_GLOBAL float *normal = (const FJ_GLOBAL float *) normal_;
  const FJ_GLOBAL float *position = (const FJ_GLOBAL float *) position_;
  const FJ_GLOBAL int32_t *ids = (const FJ_GLOBAL int32_t *) ids_;
  FJ_GLOBAL dn_v4f *guide = (FJ_GLOBAL dn_v4f *) guide_;
  const size_t at = (size_t) (ymin + y) * (size_t) xres + (size_t) (xmin + x);
  dn_v4f a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
  if (normal) { a.x = normal[3 * at]; a.y = normal[3 * at + 1]; a.z = normal[3 * at + 2]; }
  if (ids) a.w = __int_as_float(ids[4 * at]);
  if (position) { b.x = position[3 * at]; b.y = position[3 * at + 1]; b.z = position[3 * at + 2]; }
  const size_t to = (size_t) y * (size_t) w + (size_t) x;
  guide[2 * to] = a;
  guide[2 * to + 1] = b;
}

__device__ __forceinline__ DnPixel dn_load(const FJ_GLOBAL dn_v4f *src, size_t at, const FJ_GLOBAL dn_v4f *guide, size_t g)
{
  const dn_v4f c = src[at], a = guide[2 * g], b = guide[2 * g + 1];
  DnPixel p;
  p.r = c.x; p.g = c.y; p.b = c.z; p.a = c.w;
  p.nx = a.x; p.ny = a.y; p.nz = a.z; p.id = __float_as_int(a.w);
  p.px = b.x; p.py = b.y; p.pz = b.z; p.pad = 0.f;
  return p;
}

__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_atrous(const float *src_, int src_stride, const float *guide_, float *dst_, int dst_stride,
    int w, int h, int spacing, int stop_at_ids, DnConst k)
{
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const FJ_GLOBAL dn_v4f *src = (const FJ_GLOBAL dn_v4f *) src_;
  const FJ_GLOBAL dn_v4f *guide = (const FJ_GLOBAL dn_v4f *) guide_;
  FJ_GLOBAL dn_v4f *dst = (FJ_GLOBAL dn_v4f *) dst_;
  const DnPixel p = dn_load(src, (size_t) y * (size_t) src_stride + (size_t) x, guide, (size_t) y * (size_t) w + (size_t) x);
  DnAccum s;
  fj_dn_clear(s);
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + spacing * dy;
    if (qy < 0 || qy >= h) continue;             // uniform over the wave: a wave is one row
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + spacing * dx;
      if (qx < 0 || qx >= w) continue;
      const DnPixel q = dn_load(src, (size_t) qy * (size_t) src_stride + (size_t) qx, guide, (size_t) qy * (size_t) w + (size_t) qx);
      fj_dn_tap(s, dx, dy, p, q, k, stop_at_ids);
    }
  }
  dn_v4f o;
  o.x = s.r / s.w; o.y = s.g / s.w; o.z = s.b / s.w; o.w = s.a / s.w;
  dst[(size_t) y * (size_t) dst_stride + (size_t) x] = o;
}

__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_demodulate(const float *src_, int src_stride, const float *albedo_, int xres, int xmin, int ymin,
    float albedo_floor, float *dst_, int dst_stride, int w, int h)
{
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const FJ_GLOBAL float *al = (const FJ_GLOBAL float *) albedo_ + 3 * ((size_t) (ymin + y) * (size_t) xres + (size_t) (xmin + x));
  dn_v4f c = ((const FJ_GLOBAL dn_v4f *) src_)[(size_t) y * (size_t) src_stride + (size_t) x];
  c.x = fj_dn_demodulate(c.x, fj_dn_albedo_clamp(al[0], albedo_floor));
  c.y = fj_dn_demodulate(c.y, fj_dn_albedo_clamp(al[1], albedo_floor));
  c.z = fj_dn_demodulate(c.z, fj_dn_albedo_clamp(al[2], albedo_floor));
  ((FJ_GLOBAL dn_v4f *) dst_)[(size_t) y * (size_t) dst_stride + (size_t) x] = c;
}

__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_remodulate(float *color_, int stride, const float *albedo_, int xres, int xmin, int ymin,
    float albedo_floor, int w, int h)
{
  const int x = blockIdx.x * DN_BX + threadIdx.x, y = blockIdx.y * DN_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const FJ_GLOBAL float *al = (const FJ_GLOBAL float *) albedo_ + 3 * ((size_t) (ymin + y) * (size_t) xres + (size_t) (xmin + x));
  FJ_GLOBAL dn_v4f *p = (FJ_GLOBAL dn_v4f *) color_ + ((size_t) y * (size_t) stride + (size_t) x);
  dn_v4f c = *p;
  c.x = fj_dn_remodulate(c.x, fj_dn_albedo_clamp(al[0], albedo_floor));
  c.y = fj_dn_remodulate(c.y, fj_dn_albedo_clamp(al[1], albedo_floor));
  c.z = fj_dn_remodulate(c.z, fj_dn_albedo_clamp(al[2], albedo_floor));
  *p = c;
}

#if FJ_DN_LDS_TILE
// The same iteration for spacing S = 1 or 2 with the block's footprint -- (64 + 4 S) x (4 + 4 S) pixels, colour and both guide halves as three
// planes of 16-byte slots -- staged in LDS: consecutive lanes read consecutive slots (ds_read_b128 without bank conflicts), every pixel of
// the footprint crosses the memory system once per block instead of up to 25 times.  Same statements per tap, same order: same bits.
template <int S>
__global__ void __launch_bounds__(DN_BX * DN_BY) k_dn_atrous_tile(const float *src_, int src_stride, const float *guide_, float *dst_, int dst_stride,
    int w, int h, int stop_at_ids, DnConst k)
{
  constexpr int TW = DN_BX + 4 * S, TH = DN_BY + 4 * S;
  __shared__ dn_v4f s_c[TH * TW], s_a[TH * TW], s_b[TH * TW];
  const FJ_GLOBAL dn_v4f *src = (const FJ_GLOBAL dn_v4f *) src_;
  const FJ_GLOBAL dn_v4f *guide = (const FJ_GLOBAL dn_v4f *) guide_;
  FJ_GLOBAL dn_v4f *dst = (FJ_GLOBAL dn_v4f *) dst_;
  const int x0 = blockIdx.x * DN_BX - 2 * S, y0 = blockIdx.y * DN_BY - 2 * S;
  for (int i = threadIdx.y * DN_BX + threadIdx.x; i < TW * TH; i += DN_BX * DN_BY) {
    const int gx = x0 + i % TW, gy = y0 + i / TW;
    if (gx < 0 || gx >= w || gy < 0 || gy >= h) continue;      // (never read: the taps test the same coordinates)
    const size_t g = (size_t) gy * (size_t) w + (size_t) gx;
    s_c[i] = src[(size_t) gy * (size_t) src_stride + (size_t) gx];
    s_a[i] = guide[2 * g];
    s_b[i] = guide[2 * g + 1];
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
  const DnPixel p = at(ci);
  DnAccum s;
  fj_dn_clear(s);
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + S * dy;
    if (qy < 0 || qy >= h) continue;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + S * dx;
      if (qx < 0 || qx >= w) continue;
      fj_dn_tap(s, dx, dy, p, at(ci + S * dy * TW + S * dx), k, stop_at_ids);
    }
  }
  dn_v4f o;
  o.x = s.r / s.w; o.y = s.g / s.w; o.z = s.b / s.w; o.w = s.a / s.w;
  dst[(size_t) y * (size_t) dst_stride + (size_t) x] = o;
}
#endif

}  // namespace

// (blocks of rows are grid.y, at most 65535 of them: fjgpu_denoise refuses a taller region)
int launch_dn_pack(hipStream_t st, const float *normal, const float *position, const int32_t *ids, int xres, int xmin, int ymin,
    int w, int h, float *guide)
{
  if (w <= 0 || h <= 0) return 0;
  const dim3 grid((w + DN_BX - 1) / DN_BX, (h + DN_BY - 1) / DN_BY);
  if (grid.y > 65535u) return (int) hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_dn_pack, grid, dim3(DN_BX, DN_BY), 0, st, normal, position, ids, xres, xmin, ymin, w, h, guide);
  return (int) hipGetLastError();
}

int launch_dn_atrous(hipStream_t st, const float *src, int src_stride, const float *guide, float *dst, int dst_stride,
    int w, int h, int spacing, int stop_at_ids, DnConst k)
{
  if (w <= 0 || h <= 0) return 0;
  const dim3 grid((w + DN_BX - 1) / DN_BX, (h + DN_BY - 1) / DN_BY);
  if (grid.y > 65535u) return (int) hipErrorInvalidConfiguration;
#if FJ_DN_LDS_TILE
  if (spacing == 1) hipLaunchKernelGGL(k_dn_atrous_tile<1>, grid, dim3(DN_BX, DN_BY), 0, st, src, src_stride, guide, dst, dst_stride, w, h, stop_at_ids, k);
  else if (spacing == 2) hipLaunchKernelGGL(k_dn_atrous_tile<2>, grid, dim3(DN_BX, DN_BY), 0, st, src, src_stride, guide, dst, dst_stride, w, h, stop_at_ids, k);
  else
#endif
  hipLaunchKernelGGL(k_dn_atrous, grid, dim3(DN_BX, DN_BY), 0, st, src, src_stride, guide, dst, dst_stride, w, h, spacing, stop_at_ids, k);
  return (int) hipGetLastError();
}

int launch_dn_demodulate(hipStream_t st, const float *src, int src_stride, const float *albedo, int xres, int xmin, int ymin,
    float albedo_floor, float *dst, int dst_stride, int w, int h)
{
  if (w <= 0 || h <= 0) return 0;
  const dim3 grid((w + DN_BX - 1) / DN_BX, (h + DN_BY - 1) / DN_BY);
  if (grid.y > 65535u) return (int) hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_dn_demodulate, grid, dim3(DN_BX, DN_BY), 0, st, src, src_stride, albedo, xres, xmin, ymin, albedo_floor, dst, dst_stride, w, h);
  return (int) hipGetLastError();
}

int launch_dn_remodulate(hipStream_t st, float *color, int stride, const float *albedo, int xres, int xmin, int ymin,
    float albedo_floor, int w, int h)
{
  if (w <= 0 || h <= 0) return 0;
  const dim3 grid((w + DN_BX - 1) / DN_BX, (h + DN_BY - 1) / DN_BY);
  if (grid.y > 65535u) return (int) hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(k_dn_remodulate, grid, dim3(DN_BX, DN_BY), 0, st, color, stride, albedo, xres, xmin, ymin, albedo_floor, w, h);
  return (int) hipGetLastError();
}
