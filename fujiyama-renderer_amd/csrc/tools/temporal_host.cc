// temporal_host.cc -- validation tool: fjgpu_denoise_temporal and fjgpu_denoise_temporal_clamped (include/fjgpu.h) as plain loops over HOST
// arrays, every pixel through fj_tp_pixel / fj_tp_pixel_clamped of device/fjgpu_temporal_math.h -- the SAME functions k_tp_accumulate and
// k_tp_accumulate_clamped call -- so that tests/test_temporal_cpu.py and tests/test_temporal_clamp_cpu.py can hold the arithmetic against
// its numpy restatements without a GPU.  Built with the ROCm clang++ under -ffp-contract=off.  Not part of the product path.
#include <stdint.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "fjgpu.h"
#include "fjgpu_temporal_math.h"

extern "C" {

// the arguments of fjgpu_denoise_temporal_clamped on host memory; 0, or -2 (FJGPU_EINVAL) for what it refuses (the overlap tests are the
// entry's own).  With a clamp the window's records (fj_tp_record: RGBA, L, id) of the region are written first, as the kernel's blocks
// write their tiles, and fj_tp_clamp reads them through the strides of the frame.
int fj_denoise_temporal_clamped_host(const fjgpu_temporal_desc *d, const fjgpu_temporal_clamp *clamp, const float *color, const float *position,
    const float *normal, const int32_t *ids, const float *albedo, const float *variance_spatial, const fjgpu_view *prev_view, const float *prev_position, const float *prev_normal,
    const int32_t *prev_ids, const fjgpu_temporal_history *prev, const fjgpu_temporal_history *next, float *variance_out)
{
  if (!d || !color || !position || !normal || !ids) return FJGPU_EINVAL;
  if (!next || !next->color || !next->moments || !next->length) return FJGPU_EINVAL;
  if (prev && (!prev->color || !prev->moments || !prev->length || !prev_view || !prev_position || !prev_normal || !prev_ids)) return FJGPU_EINVAL;
  if (d->xres <= 0 || d->yres <= 0 || d->region[0] < 0 || d->region[1] < 0 || d->region[2] > d->xres || d->region[3] > d->yres ||
      d->region[0] >= d->region[2] || d->region[1] >= d->region[3])
    return FJGPU_EINVAL;
  if (isnan(d->alpha_min) || isnan(d->max_history) || isnan(d->tol_position) || isnan(d->cos_normal) || isnan(d->min_history_variance) ||
      isnan(d->albedo_floor))
    return FJGPU_EINVAL;
  if (!(d->alpha_min > 0.f && d->alpha_min <= 1.f) || !(d->max_history >= 1.f)) return FJGPU_EINVAL;
  if (albedo && !(isfinite(d->albedo_floor) && d->albedo_floor > 0)) return FJGPU_EINVAL;
  if (prev && (prev_view->xres <= 0 || prev_view->yres <= 0)) return FJGPU_EINVAL;
  if (((uintptr_t) color | (uintptr_t) next->color | (uintptr_t) (prev ? prev->color : nullptr)) & 15u) return FJGPU_EINVAL;
  if (clamp && (clamp->radius < 1 || clamp->radius > FJ_TP_CLAMP_MAX_RADIUS || !(isfinite(clamp->gamma) && clamp->gamma > 0.f))) return FJGPU_EINVAL;

  TpParams k;
  memset(&k, 0, sizeof(k));
  if (prev) {
    memcpy(k.w2c, prev_view->world_to_camera, sizeof(k.w2c));
    k.uv_size[0] = prev_view->uv_size[0]; k.uv_size[1] = prev_view->uv_size[1];
    k.view_xres = prev_view->xres; k.view_yres = prev_view->yres;
  }
  k.xres = d->xres; k.yres = d->yres;
  k.x0 = d->region[0]; k.y0 = d->region[1]; k.x1 = d->region[2]; k.y1 = d->region[3];
  k.alpha_min = d->alpha_min; k.max_history = d->max_history;
  k.min_history_variance = d->min_history_variance; k.albedo_floor = d->albedo_floor;
  fj_tp_terms(d->tol_position, d->cos_normal, &k);
  TpBuffers B;
  memset(&B, 0, sizeof(B));
  B.color = color; B.position = position; B.normal = normal; B.ids = ids; B.albedo = albedo; B.variance_spatial = variance_spatial;
  if (prev) {
    B.prev_position = prev_position; B.prev_normal = prev_normal; B.prev_ids = prev_ids;
    B.prev_color = prev->color; B.prev_moments = prev->moments; B.prev_length = prev->length;
  }
  B.next_color = next->color; B.next_moments = next->moments; B.next_length = next->length;
  B.variance_out = variance_out;
  if (!clamp) {
    for (int y = k.y0; y < k.y1; y++)
      for (int x = k.x0; x < k.x1; x++) fj_tp_pixel(k, B, x, y);
    return 0;
  }
  TpClamp c;
  c.radius = clamp->radius; c.stop_at_ids = clamp->stop_at_ids ? 1 : 0; c.gamma = clamp->gamma; c.amount = clamp->amount;
  const int row = k.xres * FJ_TP_REC;
  std::vector<float> records((size_t) k.yres * (size_t) row);
  for (int y = k.y0; y < k.y1; y++)
    for (int x = k.x0; x < k.x1; x++) fj_tp_record(k, B, x, y, records.data() + (size_t) y * row + (size_t) x * FJ_TP_REC);
  for (int y = k.y0; y < k.y1; y++)
    for (int x = k.x0; x < k.x1; x++) {
      const float *centre = records.data() + (size_t) y * row + (size_t) x * FJ_TP_REC;
      if (c.radius == 1) fj_tp_pixel_clamped<1>(k, B, c, centre, row, FJ_TP_REC, x, y);
      else if (c.radius == 2) fj_tp_pixel_clamped<2>(k, B, c, centre, row, FJ_TP_REC, x, y);
      else fj_tp_pixel_clamped<3>(k, B, c, centre, row, FJ_TP_REC, x, y);
    }
  return 0;
}

// the arguments of fjgpu_denoise_temporal: the call above without a clamp
int fj_denoise_temporal_host(const fjgpu_temporal_desc *d, const float *color, const float *position, const float *normal, const int32_t *ids,
    const float *albedo, const float *variance_spatial, const fjgpu_view *prev_view, const float *prev_position, const float *prev_normal,
    const int32_t *prev_ids, const fjgpu_temporal_history *prev, const fjgpu_temporal_history *next, float *variance_out)
{
  return fj_denoise_temporal_clamped_host(d, nullptr, color, position, normal, ids, albedo, variance_spatial, prev_view, prev_position, prev_normal,
                                          prev_ids, prev, next, variance_out);
}

// sizeof of the structs the Python face mirrors, as the header's compiler lays them out
int fj_temporal_host_sizeof(const char *name)
{
  if (!strcmp(name, "fj_xform_sample")) return (int) sizeof(fj_xform_sample);
  if (!strcmp(name, "fj_xform_desc")) return (int) sizeof(fj_xform_desc);
  if (!strcmp(name, "fj_camera_desc")) return (int) sizeof(fj_camera_desc);
  if (!strcmp(name, "fjgpu_view")) return (int) sizeof(fjgpu_view);
  if (!strcmp(name, "fjgpu_temporal_history")) return (int) sizeof(fjgpu_temporal_history);
  if (!strcmp(name, "fjgpu_temporal_desc")) return (int) sizeof(fjgpu_temporal_desc);
  if (!strcmp(name, "fjgpu_temporal_clamp")) return (int) sizeof(fjgpu_temporal_clamp);
  return -1;
}

// the projection alone: (fx, fy) of the world point (x, y, z) through `view`; 1 visible and finite, 0 not
int fj_temporal_host_project(const fjgpu_view *view, float x, float y, float z, double *fxy)
{
  TpParams k;
  memset(&k, 0, sizeof(k));
  memcpy(k.w2c, view->world_to_camera, sizeof(k.w2c));
  k.uv_size[0] = view->uv_size[0]; k.uv_size[1] = view->uv_size[1];
  k.view_xres = view->xres; k.view_yres = view->yres;
  return fj_tp_project(k, x, y, z, &fxy[0], &fxy[1]) ? 1 : 0;
}

}
