// fjgpu_sample_variance.h -- launcher of the sample-variance kernel (fjgpu_sample_variance.hip); the C entry point
// fjgpu_render_tiles_variance is in fjgpu_frame.hip, beside the beauty pass whose batches it reads
#ifndef FJGPU_SAMPLE_VARIANCE_H
#define FJGPU_SAMPLE_VARIANCE_H

#include <hip/hip_runtime.h>

#include "fjgpu_kernels.h"

// launch_resolve's view of a batch (fjgpu_kernels.h: the same parameters, tiles, (u, v) table and f32 RGBA samples) -> the variance of every
// listed tile's pixels, variance [yres][xres] f32.  albedo: DEVICE [yres][xres][3] f32 of which the same pixels are read, or null.
// Returns 0 or the hipError_t of the launch.
int launch_sample_variance(hipStream_t st, const ResolveParams &rp, const TileDesc *d_tiles, int n_tiles, int max_tile_pixels,
    const double *s_uv, const float *s_accum, const float *albedo, float albedo_floor, float *variance);

#endif
