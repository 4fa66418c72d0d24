// fjgpu_denoise.h -- launchers of the denoiser's kernels (fjgpu_denoise.hip); the C entry point fjgpu_denoise is in fjgpu_image_api.hip
#ifndef FJGPU_DENOISE_H
#define FJGPU_DENOISE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fjgpu_denoise_math.h"

// the region (w x h pixels, corner (xmin, ymin)) of frame-sized guide buffers (xres pixels per row; any may be NULL: zeros) -> one
// 32-byte record per region pixel, rows of w records.  Returns 0 or the hipError_t of the launch.
int launch_dn_pack(hipStream_t st, const float *normal, const float *position, const int32_t *ids, int xres, int xmin, int ymin,
    int w, int h, float *guide);

// one filter iteration over the region: src / dst point at the region's first pixel in buffers of src_stride / dst_stride pixels per row
// (RGBA f32); src and dst must not overlap.  Returns 0 or the hipError_t of the launch.
int launch_dn_atrous(hipStream_t st, const float *src, int src_stride, const float *guide, float *dst, int dst_stride,
    int w, int h, int spacing, int stop_at_ids, DnConst k);

// albedo demodulation around the iterations (fjgpu_denoise_albedo).  `albedo` is frame-sized ([.][xres][3]); (xmin, ymin) the region's corner.
// demodulate: the region of src (src_stride pixels per row, pointing at the region's first pixel) -> dst (dst_stride), rgb divided by the
// clamped albedo, alpha copied; src and dst must not overlap.  remodulate: rgb of the region of `color` multiplied by it, in place.
int launch_dn_demodulate(hipStream_t st, const float *src, int src_stride, const float *albedo, int xres, int xmin, int ymin,
    float albedo_floor, float *dst, int dst_stride, int w, int h);
int launch_dn_remodulate(hipStream_t st, float *color, int stride, const float *albedo, int xres, int xmin, int ymin,
    float albedo_floor, int w, int h);

#endif
