// fjgpu_matte.h -- launcher of the id/coverage matte kernel (fjgpu_matte.hip); the C entry point fjgpu_render_aov_matte is in
// fjgpu_api.hip, beside the AOV pass whose batches it reads
#ifndef FJGPU_MATTE_H
#define FJGPU_MATTE_H

#include <hip/hip_runtime.h>

#include "fjgpu_kernels.h"

struct MatteParams {           // fjgpu_render_aov_matte: the kernel's view of the call (fjgpu_matte_desc, fjgpu_matte_buffers)
  int32_t key, ranks, filtered;
  int32_t margin_x, margin_y, pad;
  int32_t *ids;                // DEVICE [yres][xres][ranks]
  float *coverage;             // DEVICE [yres][xres][ranks]
  float *rest;                 // DEVICE [yres][xres] or null
  int32_t *distinct;           // DEVICE [yres][xres] or null
};

// a batch of the AOV pass after its closest-hit walk -- launch_resolve's frame parameters and tiles, the batch's (u, v) table and hit
// records -- -> the ranked keys and shares of every listed tile's pixels (fjgpu_matte_math.h).  Returns 0 or the hipError_t of the launch.
int launch_aov_matte(hipStream_t st, const DInstance *instances, const ResolveParams &rp, const MatteParams &mp, const TileDesc *d_tiles,
    int n_tiles, int max_tile_pixels, const double *s_uv, const DHit *hits);

#endif
