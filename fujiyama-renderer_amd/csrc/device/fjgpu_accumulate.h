// fjgpu_accumulate.h -- launchers of the frame accumulation's kernels (fjgpu_accumulate.hip); the C entry points fjgpu_accumulate and
// fjgpu_accumulate_tile_error are in fjgpu_image_api.hip
#ifndef FJGPU_ACCUMULATE_H
#define FJGPU_ACCUMULATE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fjgpu_accum_math.h"

// one launch over the n_rects rectangles (xmin ymin xmax ymax, DEVICE, 16-byte aligned, each inside the frame and not empty, no two
// overlapping) of at most max_patches 16 x 16 patches each; every buffer of `B` is DEVICE memory, pixel (0, 0) of the frame.
// n_rects * max_patches <= 2^31 - 1.  Returns 0 or the hipError_t of the launch.
int launch_ac_accumulate(hipStream_t st, const AcBuffers &B, const int32_t *d_rects, int n_rects, uint32_t max_patches, int xres, int reset);

// one block per rectangle: d_errors[i] = the error of rectangle i
int launch_ac_tile_error(hipStream_t st, const float *mean, const float *m2, const float *count, const int32_t *d_rects, int n_rects, int xres,
    float lum_floor, float *d_errors);

#endif
