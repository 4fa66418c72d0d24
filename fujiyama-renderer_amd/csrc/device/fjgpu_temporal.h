// fjgpu_temporal.h -- launcher of the temporal accumulation's kernel (fjgpu_temporal.hip); the C entry points fjgpu_denoise_temporal and
// fjgpu_denoise_temporal_clamped are in fjgpu_image_api.hip
#ifndef FJGPU_TEMPORAL_H
#define FJGPU_TEMPORAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fjgpu_temporal_math.h"

// one launch over the region of `k`: every buffer of `B` is DEVICE memory, pixel (0, 0) of the frame; no output may overlap an input.
// Returns 0 or the hipError_t of the launch.
int launch_tp_accumulate(hipStream_t st, const TpParams &k, const TpBuffers &B);

// the same with the history clipped to the box of the current frame's window (c.radius 1..3; c.amount DEVICE memory or null)
int launch_tp_accumulate_clamped(hipStream_t st, const TpParams &k, const TpBuffers &B, const TpClamp &c);

#endif
