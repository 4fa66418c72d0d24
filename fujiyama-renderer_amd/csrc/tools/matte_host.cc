// matte_host.cc -- validation tool: the matte pass of fjgpu_render_aov_matte (include/fjgpu.h) as a plain loop over HOST arrays of samples,
// every pixel through fj_mt_pixel of device/fjgpu_matte_math.h -- the header k_aov_matte compiles -- so that tests/test_matte_cpu.py can
// hold the definition against its numpy restatement without a GPU.  Built with the ROCm clang++ under -ffp-contract=off.  Not part of the
// product path.
#include <stdint.h>

#include "fjgpu.h"
#include "fjgpu_matte_math.h"

static_assert(FJ_MT_MAX_RANKS == FJGPU_MATTE_MAX_RANKS && FJ_MT_KEY_INSTANCE == FJGPU_MATTE_KEY_INSTANCE && FJ_MT_KEY_SHADER == FJGPU_MATTE_KEY_SHADER,
              "fjgpu_matte_math.h restates the constants of include/fjgpu.h");

extern "C" {

// what k_aov_matte reads of ResolveParams and MatteParams (fjgpu_kernels.h, fjgpu_matte.h) ...
struct fj_mt_host_frame {
  int32_t xres, yres, rate_x, rate_y, npx_x, npx_y;
  double fw, fh;
  int32_t margin_x, margin_y;
};

// ... and of one TileDesc: the pixel rectangle, the samples per row and the tile's first sample slot in s_uv / keys
struct fj_mt_host_tile {
  int32_t xmin, ymin, xmax, ymax;
  int32_t nx, ny;
  uint32_t sample_offset;
  int32_t pad;
};

// the mattes of the pixels of n_tiles tiles: s_uv [.][2] f64 as the AOV pass holds it after a batch's sample generation (may be NULL with
// filtered = 0), keys [.] the key of every sample (-1: not ranked); ids / coverage [yres][xres][ranks], rest / distinct [yres][xres] or NULL,
// pixels outside the tiles untouched.  0, or -2 (FJGPU_EINVAL) for what the entry point refuses and for a tile whose window would leave its
// samples.
int fj_matte_host(const fj_mt_host_frame *frame, const fj_mt_host_tile *tiles, int n_tiles, int filtered, int ranks, const double *s_uv,
    const int32_t *keys, int32_t *ids, float *coverage, float *rest, int32_t *distinct)
{
  if (!frame || !tiles || !keys || !ids || !coverage || (filtered && !s_uv)) return FJGPU_EINVAL;
  if (ranks < 1 || ranks > FJGPU_MATTE_MAX_RANKS) return FJGPU_EINVAL;
  SvFrame f;
  f.xres = frame->xres; f.yres = frame->yres; f.rate_x = frame->rate_x; f.rate_y = frame->rate_y; f.npx_x = frame->npx_x; f.npx_y = frame->npx_y;
  f.fw = frame->fw; f.fh = frame->fh;
  if (f.xres <= 0 || f.yres <= 0 || f.rate_x <= 0 || f.rate_y <= 0 || f.npx_x <= 0 || f.npx_y <= 0) return FJGPU_EINVAL;
  if (frame->margin_x < 0 || frame->margin_y < 0 || f.npx_x != f.rate_x + 2 * frame->margin_x || f.npx_y != f.rate_y + 2 * frame->margin_y) return FJGPU_EINVAL;
  for (int t = 0; t < n_tiles; t++) {
    const fj_mt_host_tile &T = tiles[t];
    const int tw = T.xmax - T.xmin, th = T.ymax - T.ymin;
    if (T.xmin < 0 || T.ymin < 0 || T.xmax > f.xres || T.ymax > f.yres || tw <= 0 || th <= 0) return FJGPU_EINVAL;
    if ((tw - 1) * f.rate_x + f.npx_x > T.nx || (th - 1) * f.rate_y + f.npx_y > T.ny) return FJGPU_EINVAL;
    for (int py = T.ymin; py < T.ymax; py++)
      for (int px = T.xmin; px < T.xmax; px++) {
        const size_t at = (size_t) py * f.xres + px;
        const int x0 = (px - T.xmin) * f.rate_x + (filtered ? 0 : frame->margin_x), y0 = (py - T.ymin) * f.rate_y + (filtered ? 0 : frame->margin_y);
        const size_t first = (size_t) T.sample_offset + (size_t) y0 * T.nx + (size_t) x0;
        fj_mt_pixel(f, filtered ? 1 : 0, ranks, px, py, first, T.nx, s_uv, keys, ids + at * ranks, coverage + at * ranks, rest ? rest + at : nullptr,
                    distinct ? distinct + at : nullptr);
      }
  }
  return 0;
}

// the slot rule, for the tests that hold the model's against it
int32_t fj_matte_host_shader_key(int sg, int n_shaders, const int32_t *shaders) { return fj_mt_shader_key(sg, n_shaders, shaders); }

}
