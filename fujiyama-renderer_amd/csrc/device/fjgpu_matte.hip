// fjgpu_matte.hip -- the kernel of fjgpu_render_aov_matte (include/fjgpu.h): per pixel the `ranks` keys (instance or shader) with the
// greatest share of the pixel, and those shares, from the hit records and the (u, v) table the AOV pass holds after a batch's closest-hit
// walk.  The definition is fjgpu_matte_math.h, the same source the host twin of the CPU tests compiles; this file is the data movement
// around it.
//
//   k_aov_matte<kFiltered>  on k_resolve's grid (fjgpu_kernels.hip): one wave per pixel, the lanes take the samples of the pixel's window in
//                      row-major order -- the filter window with k_resolve's weights, or the pixel's own samples with weight 1 -- so a
//                      load instruction reads whole window rows.  Each lane computes the key and the weight of its first MT_KEEP samples
//                      once and keeps them in registers (the shader key costs the dependent gather hit -> instance -> face group ->
//                      shader slot); only a window of more than 64 MT_KEEP samples reads the rest again in every pass.  The key loop is
//                      wave-uniform: a butterfly takes the smallest key above the last one, a second one adds the lanes' f64 sums of that
//                      key's weights, every lane inserts the pair into its own copy of the ranked list (the same bits in every lane: no
//                      broadcast), lane 0 writes the pixel.  distinct x two passes over ceil(window / 64) samples per lane.
//                      No LDS, no atomics, no scratch memory, no cap on the number of keys; a wave talks to no other.
#include <hip/hip_runtime.h>

#include "fjgpu.h"
#include "fjgpu_matte.h"
#include "fjgpu_matte_math.h"

static_assert(FJ_MT_MAX_RANKS == FJGPU_MATTE_MAX_RANKS && FJ_MT_KEY_INSTANCE == FJGPU_MATTE_KEY_INSTANCE && FJ_MT_KEY_SHADER == FJGPU_MATTE_KEY_SHADER,
              "fjgpu_matte_math.h restates the constants of include/fjgpu.h");

namespace {

#define FJ_GLOBAL __attribute__((address_space(1)))
#define FJ_G(T, ptr) ((const FJ_GLOBAL T *) (ptr))

constexpr int MT_BLOCK = 256;
constexpr int MT_KEEP = 4;          // samples per lane whose key and weight stay in registers: windows of up to 256 samples are read once

__device__ __forceinline__ double mt_wave_sum(double x)
{
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

__device__ __forceinline__ int32_t mt_wave_min(int32_t x)
{
  for (int off = 32; off > 0; off >>= 1) { const int32_t o = __shfl_xor(x, off); x = o < x ? o : x; }
  return x;
}

template <bool kFiltered>
__global__ void __launch_bounds__(MT_BLOCK) k_aov_matte(const DInstance *instances, ResolveParams rp, MatteParams mp, const TileDesc *tiles,
    const double *s_uv, const DHit *hits)
{
  const TileDesc T = tiles[blockIdx.y];
  const int tw = T.xmax - T.xmin, th = T.ymax - T.ymin;
  const int k = blockIdx.x * (MT_BLOCK / 64) + (threadIdx.x >> 6);     // pixel of this wave
  if (k >= tw * th) return;
  const int lane = (int) __lane_id();
  const int px = T.xmin + k % tw, py = T.ymin + k / tw;
  const size_t at = (size_t) py * rp.xres + px;
  // the window: k_resolve's, or k_aov_reduce's own samples (the same window without its margin)
  const int nwx = kFiltered ? rp.npx_x : rp.rate_x, nwy = kFiltered ? rp.npx_y : rp.rate_y;
  const int x0 = (px - T.xmin) * rp.rate_x + (kFiltered ? 0 : mp.margin_x), y0 = (py - T.ymin) * rp.rate_y + (kFiltered ? 0 : mp.margin_y);
  const size_t first = (size_t) T.sample_offset + (size_t) y0 * T.nx + (size_t) x0;
  const int nwin = nwx * nwy;
  SvFrame f;
  f.xres = rp.xres; f.yres = rp.yres; f.rate_x = rp.rate_x; f.rate_y = rp.rate_y; f.npx_x = rp.npx_x; f.npx_y = rp.npx_y;
  f.fw = rp.fw; f.fh = rp.fh;
  const bool by_shader = mp.key == FJ_MT_KEY_SHADER;

  auto slot_of = [&](int w) {
    const int sy = w / nwx, sx = w - sy * nwx;
    return first + (size_t) sy * T.nx + sx;
  };
  // the key of sample w (fjgpu_matte_math.h): with the statements k_aov_reduce uses for ids[0] and ids[3] (fjgpu_dev_aov.h), restated
  auto key_of = [&](int w) -> int32_t {
    const FJ_GLOBAL DHit *hp = FJ_G(DHit, hits) + slot_of(w);
    const int inst = hp->inst;
    if (inst < 0) return -1;
    if (!by_shader) return inst;
    const FJ_GLOBAL DInstance *I = FJ_G(DInstance, instances) + inst;
    int sg = 0;                                                      // (a curve hit: the shading group is 0)
    if (I->sh_type != FJ_PRIMSET_CURVE && I->sh_face_group) sg = FJ_G(int32_t, I->sh_face_group)[hp->prim];
    return fj_mt_shader_key(sg, I->n_shaders, I->shaders);
  };
  auto weight_of = [&](int w) -> double {
    if (!kFiltered) return 1.;
    const double2 uv = reinterpret_cast<const double2 *>(s_uv)[slot_of(w)];
    return fj_sv_weight(f, px, py, uv.x, uv.y);
  };

  int32_t kk[MT_KEEP];
  double kw[MT_KEEP];
  double W = 0;
#pragma unroll
  for (int j = 0; j < MT_KEEP; j++) {
    const int w = lane + 64 * j;
    kk[j] = -1; kw[j] = 0.;
    if (w < nwin) { kk[j] = key_of(w); kw[j] = weight_of(w); W += kw[j]; }
  }
  const bool tail = nwin > 64 * MT_KEEP;                               // (uniform over the grid)
  if (tail)
    for (int w = lane + 64 * MT_KEEP; w < nwin; w += 64) W += weight_of(w);
  W = mt_wave_sum(W);

  MtList L;
  fj_mt_clear(L);
  double R = 0;
  int32_t last = -1;
  int n = 0;
  for (;;) {
    int32_t key = INT32_MAX;
#pragma unroll
    for (int j = 0; j < MT_KEEP; j++)
      if (kk[j] > last && kk[j] < key) key = kk[j];
    if (tail)
      for (int w = lane + 64 * MT_KEEP; w < nwin; w += 64) {
        const int32_t k2 = key_of(w);
        if (k2 > last && k2 < key) key = k2;
      }
    key = mt_wave_min(key);
    if (key == INT32_MAX) break;                                       // (the same in every lane)
    double A = 0;
#pragma unroll
    for (int j = 0; j < MT_KEEP; j++)
      if (kk[j] == key) A += kw[j];
    if (tail)
      for (int w = lane + 64 * MT_KEEP; w < nwin; w += 64)
        if (key_of(w) == key) A += weight_of(w);
    A = mt_wave_sum(A);
    fj_mt_insert(L, mp.ranks, key, A, R);
    n++;
    last = key;
  }
  if (lane != 0) return;
  fj_mt_write(L, mp.ranks, kFiltered ? 1 : 0, W, nwin, R, n, mp.ids + at * (size_t) mp.ranks, mp.coverage + at * (size_t) mp.ranks,
              mp.rest ? mp.rest + at : nullptr, mp.distinct ? mp.distinct + at : nullptr);
}

}  // namespace

int launch_aov_matte(hipStream_t st, const DInstance *instances, const ResolveParams &rp, const MatteParams &mp, const TileDesc *d_tiles,
    int n_tiles, int max_tile_pixels, const double *s_uv, const DHit *hits)
{
  if (n_tiles <= 0 || max_tile_pixels <= 0) return 0;
  const dim3 grid((max_tile_pixels + MT_BLOCK / 64 - 1) / (MT_BLOCK / 64), n_tiles);      // k_resolve's grid: one wave per pixel
  if (mp.filtered) hipLaunchKernelGGL(k_aov_matte<true>, grid, dim3(MT_BLOCK), 0, st, instances, rp, mp, d_tiles, s_uv, hits);
  else hipLaunchKernelGGL(k_aov_matte<false>, grid, dim3(MT_BLOCK), 0, st, instances, rp, mp, d_tiles, s_uv, hits);
  return (int) hipGetLastError();
}
