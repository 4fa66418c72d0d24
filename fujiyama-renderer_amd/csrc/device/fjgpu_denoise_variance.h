// fjgpu_denoise_variance.h -- launchers of the variance-guided denoiser's kernels (fjgpu_denoise_variance.hip); the C entry points
// fjgpu_denoise_estimate_variance and fjgpu_denoise_variance are in fjgpu_image_api.hip
#ifndef FJGPU_DENOISE_VARIANCE_H
#define FJGPU_DENOISE_VARIANCE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fjgpu_denoise_var_math.h"

// launch_dn_pack (fjgpu_denoise.h) with the luminance of `color` in the record's pad slot.  color points at the region's first pixel in a
// buffer of color_stride pixels per row (RGBA f32, 16-byte aligned).  Every launcher here returns 0 or the hipError_t of the launch.
int launch_dn_pack_var(hipStream_t st, const float *color, int color_stride, const float *normal, const float *position, const int32_t *ids,
    int xres, int xmin, int ymin, int w, int h, float *guide);

// the spatial variance estimate of the region from launch_dn_pack_var's records -> variance (f32, variance_stride values per row, pointing
// at the region's first pixel)
int launch_dn_variance(hipStream_t st, const float *guide, float *variance, int variance_stride, int w, int h, int stop_at_ids, DnConst k);

// one variance-guided iteration over the region: src / dst as launch_dn_atrous's, vin / vout the variance planes (f32, their own strides,
// pointing at the region's first pixel).  Neither output may overlap an input.
int launch_dn_atrous_var(hipStream_t st, const float *src, int src_stride, const float *guide, const float *vin, int vin_stride,
    float *dst, int dst_stride, float *vout, int vout_stride, int w, int h, int spacing, int stop_at_ids, float sigma_luminance, DnConst k);

#endif
