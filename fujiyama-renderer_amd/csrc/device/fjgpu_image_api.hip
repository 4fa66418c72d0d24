// fjgpu_image_api.hip -- C ABI of libfjgpu.so (include/fjgpu.h), the image-space passes: entry points that take a device index,
// frame-sized DEVICE buffers and a small description, and no fjgpu_scene.  Each one is its refusals, its transient buffers and a handful
// of launches (fjgpu_denoise.hip, fjgpu_denoise_variance.hip, fjgpu_temporal.hip, fjgpu_accumulate.hip) inside one shared call frame, ImageCall.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "fjgpu.h"
#include "fjgpu_accumulate.h"
#include "fjgpu_api_common.h"
#include "fjgpu_denoise.h"
#include "fjgpu_denoise_variance.h"
#include "fjgpu_temporal.h"

namespace {

using fjgpu::fail;
using fjgpu::DeviceBuffers;

// ---- the region checks every entry point makes, each message under the caller's prefix `f`; 0 or the error.  Two calls, because other
// refusals of the caller (iterations, NaN, alignment) stand between the rectangle and the row limit, and the order is part of the ABI.
int check_region(const std::string &f, int xres, int yres, const int32_t *region)
{
  if (xres <= 0 || yres <= 0) return fail(FJGPU_EINVAL, f + ": resolution must be positive");
  if (region[0] < 0 || region[1] < 0 || region[2] > xres || region[3] > yres || region[0] >= region[2] || region[1] >= region[3])
    return fail(FJGPU_EINVAL, f + ": region must be a non-empty rectangle inside the frame");
  return 0;
}

// (a launch covers 4 rows per block of its y grid in the filters, 16 in the temporal pass: max_rows = 65535 * that)
int check_rows(const std::string &f, const int32_t *region, int max_rows)
{
  if (region[3] - region[1] > max_rows) return fail(FJGPU_EINVAL, f + ": a region of more than " + std::to_string(max_rows) + " rows");
  return 0;
}

const int FILTER_MAX_ROWS = 65535 * 4, TEMPORAL_MAX_ROWS = 65535 * 16;

// ---- the frame of a call, after its refusals: device, stream, events around the launches, the synchronise, the timings and the error
// returns named after the entry point.  An entry point goes
//   ImageCall call(name, hip_stream);  open(device);  its allocations;  start(n_events);
//   mark(0);  call.rc = launch ...;  mark(1);  ... (every launch behind `if (!call.rc)`)
//   return call.finish(stats, batches, total, gen, resolve);      -- which pair of marks feeds which field of fjgpu_stats
struct ImageCall {
  struct Span { int from = -1, to = -1; };      // a pair of marks; the default feeds nothing
  const std::string f;
  const hipStream_t st;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int rc = 0;      // 0, the hipError_t of a launch, or -1: hipGetLastError() knows

  ImageCall(const char *name, void *hip_stream) : f(name), st(static_cast<hipStream_t>(hip_stream)) {}
  ~ImageCall() { release(); }
  ImageCall(const ImageCall &) = delete;
  ImageCall &operator=(const ImageCall &) = delete;

  int open(int device) const
  {
    if (fjgpu_device_count() < 1) return fail(FJGPU_ENODEV, f + ": no HIP device is visible");
    HIP_TRY(hipSetDevice(device));
    return 0;
  }
  void start(int n_events) { for (int k = 0; k < n_events && !rc; k++) if (hipEventCreate(&ev[k]) != hipSuccess) rc = -1; }
  void mark(int k) const { if (ev[k]) (void) hipEventRecord(ev[k], st); }
  void release() { for (hipEvent_t &e : ev) if (e) { (void) hipEventDestroy(e); e = nullptr; } }
  int finish(fjgpu_stats *stats, uint32_t batches, Span total, Span gen, Span resolve)
  {
    const hipError_t se = hipStreamSynchronize(st);      // (also before the caller's transient buffers go away)
    fjgpu_stats acc;
    std::memset(&acc, 0, sizeof(acc));
    if (rc == 0 && se == hipSuccess) {
      float ms = 0;
      if (gen.from >= 0 && hipEventElapsedTime(&ms, ev[gen.from], ev[gen.to]) == hipSuccess) acc.gen_ms = ms;
      if (resolve.from >= 0 && hipEventElapsedTime(&ms, ev[resolve.from], ev[resolve.to]) == hipSuccess) acc.resolve_ms = ms;
      if (hipEventElapsedTime(&ms, ev[total.from], ev[total.to]) == hipSuccess) acc.total_ms = ms;
      acc.batches = batches;
    }
    release();
    if (rc) return fail(FJGPU_ENODEV, f + ": HIP failure: " + hipGetErrorString(rc > 0 ? (hipError_t) rc : hipGetLastError()));
    if (se != hipSuccess) return fail(FJGPU_ENODEV, f + ": stream synchronize: " + hipGetErrorString(se));
    if (stats) *stats = acc;
    return 0;
  }
};

// ---- what iteration 0 of a filter reads: colour / albedo where there is an albedo, staged in `scratch` (the frame iteration 0 does not
// write: iteration 1 is the first to); a copy of the region there for a single iteration in place (that launch would read pixels other
// blocks have written); else the caller's frame.  `color` points at the region's first pixel.
struct Staged { const float *src; int stride; int rc; };

Staged stage_input(hipStream_t st, const fjgpu_denoise_desc *d, const float *color, const float *albedo, float albedo_floor,
    bool one_iteration_in_place, float *scratch)
{
  const int w = d->region[2] - d->region[0], h = d->region[3] - d->region[1];
  if (albedo) return {scratch, w, launch_dn_demodulate(st, color, d->xres, albedo, d->xres, d->region[0], d->region[1], albedo_floor, scratch, w, w, h)};
  if (one_iteration_in_place)
    return {scratch, w, hipMemcpy2DAsync(scratch, (size_t) w * 16, color, (size_t) d->xres * 16, (size_t) w * 16, (size_t) h,
                                         hipMemcpyDeviceToDevice, st) != hipSuccess ? -1 : 0};
  return {color, d->xres, 0};
}

// the refusals the variance family shares, each naming `f`; 0 or the error
int dnv_check(const std::string &f, const fjgpu_denoise_desc *d, const float *color, bool with_iterations)
{
  if (const int e = check_region(f, d->xres, d->yres, d->region)) return e;
  if (with_iterations && (d->iterations < 1 || d->iterations > FJ_DN_MAX_ITERATIONS)) return fail(FJGPU_EINVAL, f + ": iterations must be 1..8");
  if (std::isnan(d->sigma_color) || std::isnan(d->sigma_normal) || std::isnan(d->sigma_position)) return fail(FJGPU_EINVAL, f + ": a sigma is NaN");
  if ((uintptr_t) color & 15u) return fail(FJGPU_EINVAL, f + ": colour buffers must be 16-byte aligned");
  return check_rows(f, d->region, FILTER_MAX_ROWS);
}

// fjgpu_denoise_estimate_variance, of the frame divided by its albedo where there is one: then the first stage of fjgpu_denoise_variance
// with an albedo (the same launches in the same order) with the estimate as the result -- the spatial fallback of fjgpu_denoise_temporal,
// whose moments are those of the demodulated luminance.
int estimate_variance(const char *name, int device, const fjgpu_denoise_desc *d, const float *color, const float *normal, const float *position,
    const int32_t *ids, const float *albedo, float albedo_floor, float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  ImageCall call(name, hip_stream);
  const std::string &f = call.f;
  if (albedo && !(std::isfinite(albedo_floor) && albedo_floor > 0)) return fail(FJGPU_EINVAL, f + ": albedo_floor must be finite and > 0");
  if (!d || !color || !variance_out) return fail(FJGPU_EINVAL, f + ": null argument (desc, color and variance_out are required)");
  if (const int e = dnv_check(f, d, color, false)) return e;
  if ((const void *) variance_out == (const void *) color || (albedo && (const void *) variance_out == (const void *) albedo))
    return fail(FJGPU_EINVAL, f + (albedo ? ": variance_out must not be the colour or the albedo buffer" : ": variance_out must not be the colour buffer"));
  if (const int e = call.open(device)) return e;
  const int w = d->region[2] - d->region[0], h = d->region[3] - d->region[1];
  const size_t npx = (size_t) w * (size_t) h;
  const int stop = (d->stop_at_ids && ids) ? 1 : 0;
  DeviceBuffers W;
  float *d_guide, *d_dem = nullptr;
  if (W.alloc(npx * 8, &d_guide) || (albedo && W.alloc(npx * 4, &d_dem))) return fail(FJGPU_ENOMEM, f + ": device allocation failed");
  call.start(2);
  const size_t origin = (size_t) d->region[1] * (size_t) d->xres + (size_t) d->region[0];
  if (!call.rc) {
    call.mark(0);
    const Staged in = stage_input(call.st, d, color + origin * 4, albedo, albedo_floor, false, d_dem);
    call.rc = in.rc;
    if (!call.rc) call.rc = launch_dn_pack_var(call.st, in.src, in.stride, normal, position, ids, d->xres, d->region[0], d->region[1], w, h, d_guide);
    if (!call.rc) call.rc = launch_dn_variance(call.st, d_guide, variance_out + origin, d->xres, w, h, stop,
                                               fj_dn_constants(0.f, normal ? d->sigma_normal : 0.f, position ? d->sigma_position : 0.f, 0));
    call.mark(1);
  }
  return call.finish(stats, 0, {0, 1}, {0, 1}, {});
}

bool tp_overlap(const void *a, size_t na, const void *b, size_t nb)
{
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// ---- the rectangle list of the accumulation's two entries: n_rects >= 0 rectangles inside the frame, none empty (rects NULL: the whole
// frame, n_rects is not read).  *list: the rectangles to upload; *max_patches: the 16 x 16 patches of the largest.
int ac_check_rects(const std::string &f, int xres, int yres, const int32_t *rects, int n_rects, std::vector<int32_t> *list, uint32_t *max_patches)
{
  if (xres <= 0 || yres <= 0) return fail(FJGPU_EINVAL, f + ": resolution must be positive");
  if (rects && n_rects < 0) return fail(FJGPU_EINVAL, f + ": n_rects is negative");
  if (rects) list->assign(rects, rects + 4 * (size_t) n_rects);
  else *list = {0, 0, xres, yres};
  *max_patches = 0;
  for (size_t i = 0; i < list->size(); i += 4) {
    const int32_t *r = list->data() + i;
    if (r[0] < 0 || r[1] < 0 || r[2] > xres || r[3] > yres || r[0] >= r[2] || r[1] >= r[3])
      return fail(FJGPU_EINVAL, f + ": rect " + std::to_string(i / 4) + " must be a non-empty rectangle inside the frame");
    const unsigned long long n = (unsigned long long) ((r[2] - r[0] + FJ_AC_BX - 1) / FJ_AC_BX) * (unsigned long long) ((r[3] - r[1] + FJ_AC_BY - 1) / FJ_AC_BY);
    if (n > 0x7fffffffull) return fail(FJGPU_EINVAL, f + ": a rect of more than 2^31 - 1 patches of 16 x 16 pixels");
    *max_patches = std::max(*max_patches, (uint32_t) n);
  }
  return 0;
}

}  // namespace

extern "C" {

// ---- denoiser (fjgpu_denoise.hip, fjgpu_denoise_math.h).  Shaped like the AOV pass: no scene, transient buffers per call -- two RGBA frames
// of the region for the iterations to ping-pong between and one 32-byte guide record per region pixel.  Iteration 0 reads color_in and the
// last one writes color_out, every other end of an iteration is a scratch frame, so color_out may be color_in: with two or more iterations
// no launch reads what it writes, and a single iteration in place filters a copy of the region.
// (the refusals keep fjgpu_denoise's name in their messages, whichever of the two entry points was called: with albedo NULL they are the same call)
int fjgpu_denoise_albedo(int device, const fjgpu_denoise_desc *d, const float *color_in, const float *normal, const float *position,
    const int32_t *ids, const float *albedo, float albedo_floor, float *color_out, void *hip_stream, fjgpu_stats *stats)
{
  ImageCall call("fjgpu_denoise", hip_stream);
  const std::string &f = call.f;
  if (albedo && !(std::isfinite(albedo_floor) && albedo_floor > 0)) return fail(FJGPU_EINVAL, "fjgpu_denoise_albedo: albedo_floor must be finite and > 0");
  if (!d || !color_in || !color_out) return fail(FJGPU_EINVAL, f + ": null argument (desc, color_in and color_out are required)");
  if (const int e = check_region(f, d->xres, d->yres, d->region)) return e;
  if (d->iterations < 1 || d->iterations > FJ_DN_MAX_ITERATIONS) return fail(FJGPU_EINVAL, f + ": iterations must be 1..8");
  if (std::isnan(d->sigma_color) || std::isnan(d->sigma_normal) || std::isnan(d->sigma_position)) return fail(FJGPU_EINVAL, f + ": a sigma is NaN");
  if (((uintptr_t) color_in | (uintptr_t) color_out) & 15u) return fail(FJGPU_EINVAL, f + ": color_in and color_out must be 16-byte aligned");
  if (const int e = check_rows(f, d->region, FILTER_MAX_ROWS)) return e;
  if (const int e = call.open(device)) return e;
  const int w = d->region[2] - d->region[0], h = d->region[3] - d->region[1];
  const size_t npx = (size_t) w * (size_t) h;
  const int n_it = d->iterations;
  const int stop = (d->stop_at_ids && ids) ? 1 : 0;

  DeviceBuffers W;
  float *d_frame[2], *d_guide;
  if (W.alloc(npx * 4, &d_frame[0]) || W.alloc(npx * 4, &d_frame[1]) || W.alloc(npx * 8, &d_guide))
    return fail(FJGPU_ENOMEM, f + ": device allocation failed");

  call.start(3);      // call start, guide pack (and demodulation) done, iterations done
  const size_t origin = ((size_t) d->region[1] * (size_t) d->xres + (size_t) d->region[0]) * 4;
  Staged in = {color_in + origin, d->xres, 0};
  if (!call.rc) {
    call.mark(0);
    call.rc = launch_dn_pack(call.st, normal, position, ids, d->xres, d->region[0], d->region[1], w, h, d_guide);
    call.mark(1);
  }
  if (!call.rc) {
    in = stage_input(call.st, d, color_in + origin, albedo, albedo_floor, n_it == 1 && color_in == color_out, d_frame[1]);
    call.rc = in.rc;
    if (albedo) call.mark(1);      // (gen_ms: the guide pack and this copy)
  }
  for (int i = 0; i < n_it && !call.rc; i++) {      // iteration i reads `in`, and what it wrote is the next one's
    const bool last = i == n_it - 1;
    float *dst = last ? color_out + origin : d_frame[i & 1];
    const int dst_stride = last ? d->xres : w;
    call.rc = launch_dn_atrous(call.st, in.src, in.stride, d_guide, dst, dst_stride, w, h, 1 << i, stop,
                               fj_dn_constants(d->sigma_color, normal ? d->sigma_normal : 0.f, position ? d->sigma_position : 0.f, i));
    in.src = dst; in.stride = dst_stride;
  }
  if (!call.rc && albedo) call.rc = launch_dn_remodulate(call.st, color_out + origin, d->xres, albedo, d->xres, d->region[0], d->region[1], albedo_floor, w, h);
  call.mark(2);
  return call.finish(stats, (uint32_t) n_it, {0, 2}, {0, 1}, {1, 2});
}

int fjgpu_denoise(int device, const fjgpu_denoise_desc *d, const float *color_in, const float *normal, const float *position,
    const int32_t *ids, float *color_out, void *hip_stream, fjgpu_stats *stats)
{
  return fjgpu_denoise_albedo(device, d, color_in, normal, position, ids, nullptr, 0.f, color_out, hip_stream, stats);
}

// ---- variance-guided denoiser (fjgpu_denoise_variance.hip, fjgpu_denoise_var_math.h).  fjgpu_denoise's shape and scratch, plus two f32
// planes of the region: the estimate (or nothing, where the caller brings a variance) lands in one, the iterations ping-pong between them.
int fjgpu_denoise_estimate_variance(int device, const fjgpu_denoise_desc *d, const float *color, const float *normal, const float *position,
    const int32_t *ids, float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  return estimate_variance("fjgpu_denoise_estimate_variance", device, d, color, normal, position, ids, nullptr, 0.f, variance_out, hip_stream, stats);
}

// (without an albedo it is the plain entry point, and answers with that name)
int fjgpu_denoise_estimate_variance_albedo(int device, const fjgpu_denoise_desc *d, const float *color, const float *normal, const float *position,
    const int32_t *ids, const float *albedo, float albedo_floor, float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  return estimate_variance(albedo ? "fjgpu_denoise_estimate_variance_albedo" : "fjgpu_denoise_estimate_variance", device, d, color, normal,
                           position, ids, albedo, albedo_floor, variance_out, hip_stream, stats);
}

int fjgpu_denoise_variance(int device, const fjgpu_denoise_desc *d, float sigma_luminance, const float *color_in, const float *normal,
    const float *position, const int32_t *ids, const float *albedo, float albedo_floor, const float *variance_in, float *color_out,
    float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  ImageCall call("fjgpu_denoise_variance", hip_stream);
  const std::string &f = call.f;
  if (albedo && !(std::isfinite(albedo_floor) && albedo_floor > 0)) return fail(FJGPU_EINVAL, f + ": albedo_floor must be finite and > 0");
  if (!d || !color_in || !color_out) return fail(FJGPU_EINVAL, f + ": null argument (desc, color_in and color_out are required)");
  if (const int e = dnv_check(f, d, (const float *) ((uintptr_t) color_in | (uintptr_t) color_out), true)) return e;
  if (std::isnan(sigma_luminance)) return fail(FJGPU_EINVAL, f + ": sigma_luminance is NaN");
  if (variance_out && ((const void *) variance_out == (const void *) variance_in || (const void *) variance_out == (const void *) color_in ||
                       (const void *) variance_out == (const void *) color_out))
    return fail(FJGPU_EINVAL, f + ": variance_out must not be variance_in or a colour buffer");
  if (variance_in && ((const void *) variance_in == (const void *) color_out)) return fail(FJGPU_EINVAL, f + ": variance_in must not be color_out");
  if (const int e = call.open(device)) return e;
  const int w = d->region[2] - d->region[0], h = d->region[3] - d->region[1];
  const size_t npx = (size_t) w * (size_t) h;
  const int n_it = d->iterations;
  const int stop = (d->stop_at_ids && ids) ? 1 : 0;
  const DnConst k = fj_dn_constants(0.f, normal ? d->sigma_normal : 0.f, position ? d->sigma_position : 0.f, 0);

  DeviceBuffers W;
  float *d_frame[2], *d_guide, *d_var[2];
  if (W.alloc(npx * 4, &d_frame[0]) || W.alloc(npx * 4, &d_frame[1]) || W.alloc(npx * 8, &d_guide) || W.alloc(npx, &d_var[0]) ||
      W.alloc(npx, &d_var[1]))
    return fail(FJGPU_ENOMEM, f + ": device allocation failed");

  call.start(3);      // call start, pack / demodulation / estimate done, iterations done
  const size_t origin = (size_t) d->region[1] * (size_t) d->xres + (size_t) d->region[0];
  Staged in = {color_in + origin * 4, d->xres, 0};
  if (!call.rc) {
    call.mark(0);
    in = stage_input(call.st, d, color_in + origin * 4, albedo, albedo_floor, n_it == 1 && color_in == color_out, d_frame[1]);
    call.rc = in.rc;
  }
  const float *vin = variance_in ? variance_in + origin : d_var[0];
  int vin_stride = variance_in ? d->xres : w;
  if (!call.rc && variance_in) {
    call.rc = launch_dn_pack(call.st, normal, position, ids, d->xres, d->region[0], d->region[1], w, h, d_guide);
  } else if (!call.rc) {
    // the estimate is of the frame the iterations filter: the demodulated one where there is an albedo
    call.rc = launch_dn_pack_var(call.st, in.src, in.stride, normal, position, ids, d->xres, d->region[0], d->region[1], w, h, d_guide);
    if (!call.rc) call.rc = launch_dn_variance(call.st, d_guide, d_var[0], w, w, h, stop, k);
  }
  call.mark(1);
  for (int i = 0; i < n_it && !call.rc; i++) {
    const bool last = i == n_it - 1;
    float *dst = last ? color_out + origin * 4 : d_frame[i & 1];
    const int dst_stride = last ? d->xres : w;
    // iteration i reads d_var[i & 1] (iteration 0: that or the caller's plane) and writes the other
    float *vout = (last && variance_out) ? variance_out + origin : d_var[(i + 1) & 1];
    const int vout_stride = (last && variance_out) ? d->xres : w;
    call.rc = launch_dn_atrous_var(call.st, in.src, in.stride, d_guide, vin, vin_stride, dst, dst_stride, vout, vout_stride, w, h, 1 << i, stop,
                                   sigma_luminance, k);
    in.src = dst; in.stride = dst_stride;
    vin = vout; vin_stride = vout_stride;
  }
  if (!call.rc && albedo) call.rc = launch_dn_remodulate(call.st, color_out + origin * 4, d->xres, albedo, d->xres, d->region[0], d->region[1], albedo_floor, w, h);
  call.mark(2);
  return call.finish(stats, (uint32_t) n_it, {0, 2}, {0, 1}, {1, 2});
}

// ---- temporal accumulation (fjgpu_temporal.hip, fjgpu_temporal_math.h).  One launch, no scratch: every refusal is decided before a device call.
// The clamp's refusals come after those of the unclamped entry, which keeps its order.
// `name`: the entry point called; `clamp` NULL: fjgpu_denoise_temporal, whichever of the two it was
static int temporal(const char *name, int device, const fjgpu_temporal_desc *d, const fjgpu_temporal_clamp *clamp, const float *color,
    const float *position, const float *normal, const int32_t *ids, const float *albedo, const float *variance_spatial,
    const fjgpu_view *prev_view, const float *prev_position, const float *prev_normal, const int32_t *prev_ids,
    const fjgpu_temporal_history *prev, const fjgpu_temporal_history *next, float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  ImageCall call(name, hip_stream);
  const std::string &f = call.f;
  if (!d || !color) return fail(FJGPU_EINVAL, f + ": null argument (desc and color are required)");
  if (!position || !normal || !ids) return fail(FJGPU_EINVAL, f + ": null guide (position, normal and ids are required: without them there is nothing to reproject)");
  if (!next || !next->color || !next->moments || !next->length) return fail(FJGPU_EINVAL, f + ": null history (next and its three buffers are required)");
  if (prev && (!prev->color || !prev->moments || !prev->length)) return fail(FJGPU_EINVAL, f + ": null history (prev is set, so are its three buffers)");
  if (prev && (!prev_view || !prev_position || !prev_normal || !prev_ids))
    return fail(FJGPU_EINVAL, f + ": null previous frame (prev is set: prev_view, prev_position, prev_normal and prev_ids are required)");
  if (const int e = check_region(f, d->xres, d->yres, d->region)) return e;
  if (std::isnan(d->alpha_min) || std::isnan(d->max_history) || std::isnan(d->tol_position) || std::isnan(d->cos_normal) ||
      std::isnan(d->min_history_variance) || std::isnan(d->albedo_floor))
    return fail(FJGPU_EINVAL, f + ": a parameter is NaN");
  if (!(d->alpha_min > 0.f && d->alpha_min <= 1.f)) return fail(FJGPU_EINVAL, f + ": alpha_min must be in (0, 1]");
  if (!(d->max_history >= 1.f)) return fail(FJGPU_EINVAL, f + ": max_history must be >= 1");
  if (albedo && !(std::isfinite(d->albedo_floor) && d->albedo_floor > 0)) return fail(FJGPU_EINVAL, f + ": albedo_floor must be finite and > 0");
  if (prev && (prev_view->xres <= 0 || prev_view->yres <= 0)) return fail(FJGPU_EINVAL, f + ": prev_view's resolution must be positive");
  if (((uintptr_t) color | (uintptr_t) next->color | (uintptr_t) (prev ? prev->color : nullptr)) & 15u)
    return fail(FJGPU_EINVAL, f + ": colour buffers must be 16-byte aligned");
  if (const int e = check_rows(f, d->region, TEMPORAL_MAX_ROWS)) return e;
  {
    const size_t px = (size_t) d->xres * (size_t) d->yres * sizeof(float);
    const struct { const void *p; size_t n; } outs[4] = {{next->color, 4 * px}, {next->moments, 2 * px}, {next->length, px}, {variance_out, px}};
    const struct { const void *p; size_t n; } ins[12] = {{color, 4 * px}, {position, 3 * px}, {normal, 3 * px}, {ids, 4 * px}, {albedo, 3 * px},
        {variance_spatial, px}, {prev ? prev_position : nullptr, 3 * px}, {prev ? prev_normal : nullptr, 3 * px}, {prev ? prev_ids : nullptr, 4 * px},
        {prev ? prev->color : nullptr, 4 * px}, {prev ? prev->moments : nullptr, 2 * px}, {prev ? prev->length : nullptr, px}};
    for (int a = 0; a < 4; a++) {
      for (int b = 0; b < 12; b++)
        if (tp_overlap(outs[a].p, outs[a].n, ins[b].p, ins[b].n))
          return fail(FJGPU_EINVAL, f + ": an output buffer (next, variance_out) overlaps prev or an input");
      for (int b = a + 1; b < 4; b++)
        if (tp_overlap(outs[a].p, outs[a].n, outs[b].p, outs[b].n)) return fail(FJGPU_EINVAL, f + ": output buffers (next, variance_out) overlap each other");
    }
  }
  if (clamp) {
    if (clamp->radius < 1 || clamp->radius > FJ_TP_CLAMP_MAX_RADIUS) return fail(FJGPU_EINVAL, f + ": clamp radius must be 1..3");
    if (!(std::isfinite(clamp->gamma) && clamp->gamma > 0.f)) return fail(FJGPU_EINVAL, f + ": clamp gamma must be finite and > 0");
    const size_t px = (size_t) d->xres * (size_t) d->yres * sizeof(float);
    const struct { const void *p; size_t n; } others[16] = {{color, 4 * px}, {position, 3 * px}, {normal, 3 * px}, {ids, 4 * px}, {albedo, 3 * px},
        {variance_spatial, px}, {prev ? prev_position : nullptr, 3 * px}, {prev ? prev_normal : nullptr, 3 * px}, {prev ? prev_ids : nullptr, 4 * px},
        {prev ? prev->color : nullptr, 4 * px}, {prev ? prev->moments : nullptr, 2 * px}, {prev ? prev->length : nullptr, px},
        {next->color, 4 * px}, {next->moments, 2 * px}, {next->length, px}, {variance_out, px}};
    for (int b = 0; b < 16; b++)
      if (tp_overlap(clamp->amount, px, others[b].p, others[b].n))
        return fail(FJGPU_EINVAL, f + ": the clamp's amount overlaps an input, prev, next or variance_out");
  }
  if (const int e = call.open(device)) return e;

  TpParams k;
  std::memset(&k, 0, sizeof(k));
  if (prev) {
    std::memcpy(k.w2c, prev_view->world_to_camera, sizeof(k.w2c));
    k.uv_size[0] = prev_view->uv_size[0]; k.uv_size[1] = prev_view->uv_size[1];
    k.view_xres = prev_view->xres; k.view_yres = prev_view->yres;
  }
  k.xres = d->xres; k.yres = d->yres;
  k.x0 = d->region[0]; k.y0 = d->region[1]; k.x1 = d->region[2]; k.y1 = d->region[3];
  k.alpha_min = d->alpha_min; k.max_history = d->max_history;
  k.min_history_variance = d->min_history_variance; k.albedo_floor = d->albedo_floor;
  fj_tp_terms(d->tol_position, d->cos_normal, &k);
  TpBuffers B;
  std::memset(&B, 0, sizeof(B));
  B.color = color; B.position = position; B.normal = normal; B.ids = ids; B.albedo = albedo; B.variance_spatial = variance_spatial;
  if (prev) {
    B.prev_position = prev_position; B.prev_normal = prev_normal; B.prev_ids = prev_ids;
    B.prev_color = prev->color; B.prev_moments = prev->moments; B.prev_length = prev->length;
  }
  B.next_color = next->color; B.next_moments = next->moments; B.next_length = next->length;
  B.variance_out = variance_out;

  call.start(2);
  if (!call.rc) {
    call.mark(0);
    if (clamp) {
      TpClamp c;
      c.radius = clamp->radius; c.stop_at_ids = clamp->stop_at_ids ? 1 : 0; c.gamma = clamp->gamma; c.amount = clamp->amount;
      call.rc = launch_tp_accumulate_clamped(call.st, k, B, c);
    } else {
      call.rc = launch_tp_accumulate(call.st, k, B);
    }
    call.mark(1);
  }
  return call.finish(stats, 1, {0, 1}, {}, {0, 1});
}

int fjgpu_denoise_temporal(int device, const fjgpu_temporal_desc *d, const float *color, const float *position, const float *normal,
    const int32_t *ids, const float *albedo, const float *variance_spatial, const fjgpu_view *prev_view, const float *prev_position,
    const float *prev_normal, const int32_t *prev_ids, const fjgpu_temporal_history *prev, const fjgpu_temporal_history *next,
    float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  return temporal("fjgpu_denoise_temporal", device, d, nullptr, color, position, normal, ids, albedo, variance_spatial, prev_view, prev_position,
                  prev_normal, prev_ids, prev, next, variance_out, hip_stream, stats);
}

int fjgpu_denoise_temporal_clamped(int device, const fjgpu_temporal_desc *d, const fjgpu_temporal_clamp *clamp, const float *color,
    const float *position, const float *normal, const int32_t *ids, const float *albedo, const float *variance_spatial,
    const fjgpu_view *prev_view, const float *prev_position, const float *prev_normal, const int32_t *prev_ids,
    const fjgpu_temporal_history *prev, const fjgpu_temporal_history *next, float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  return temporal("fjgpu_denoise_temporal_clamped", device, d, clamp, color, position, normal, ids, albedo, variance_spatial, prev_view,
                  prev_position, prev_normal, prev_ids, prev, next, variance_out, hip_stream, stats);
}

// ---- progressive accumulation (fjgpu_accumulate.hip, fjgpu_accum_math.h).  One launch each; the only transient buffers are the rectangle
// list and, for the errors, one float per rectangle.  Every refusal is decided before a device call.
int fjgpu_accumulate(int device, int xres, int yres, const int32_t *rects, int n_rects, const float *color, const fjgpu_accum_state *state,
    int reset, float *variance_out, void *hip_stream, fjgpu_stats *stats)
{
  ImageCall call("fjgpu_accumulate", hip_stream);
  const std::string &f = call.f;
  if (!color || !state || !state->mean || !state->m2 || !state->count)
    return fail(FJGPU_EINVAL, f + ": null argument (color, state and its mean, m2 and count are required)");
  std::vector<int32_t> list;
  uint32_t max_patches = 0;
  if (const int e = ac_check_rects(f, xres, yres, rects, n_rects, &list, &max_patches)) return e;
  {
    const size_t px = (size_t) xres * (size_t) yres * sizeof(float);
    const struct { const void *p; size_t n; } planes[3] = {{state->mean, 4 * px}, {state->m2, px}, {state->count, px}};
    for (int a = 0; a < 3; a++)
      if (tp_overlap(color, 4 * px, planes[a].p, planes[a].n)) return fail(FJGPU_EINVAL, f + ": color overlaps a plane of the state");
    for (int a = 0; a < 3; a++)
      if (tp_overlap(variance_out, px, planes[a].p, planes[a].n)) return fail(FJGPU_EINVAL, f + ": variance_out overlaps a plane of the state");
    for (int a = 0; a < 3; a++)
      for (int b = a + 1; b < 3; b++)
        if (tp_overlap(planes[a].p, planes[a].n, planes[b].p, planes[b].n)) return fail(FJGPU_EINVAL, f + ": the planes of the state overlap each other");
    if (tp_overlap(variance_out, px, color, 4 * px)) return fail(FJGPU_EINVAL, f + ": variance_out overlaps color");
  }
  if (((uintptr_t) color | (uintptr_t) state->mean) & 15u) return fail(FJGPU_EINVAL, f + ": color and the state's mean must be 16-byte aligned");
  const int n = (int) (list.size() / 4);
  if ((unsigned long long) n * max_patches > 0x7fffffffull) return fail(FJGPU_EINVAL, f + ": more than 2^31 - 1 blocks (rects times the patches of the largest): split the list");
  if (const int e = call.open(device)) return e;
  fjgpu_stats none;
  std::memset(&none, 0, sizeof(none));
  if (n == 0) { if (stats) *stats = none; return 0; }
  DeviceBuffers W;
  const int32_t *d_rects = nullptr;
  if (W.upload(list.data(), list.size(), &d_rects)) return fail(FJGPU_ENOMEM, f + ": device allocation failed");
  AcBuffers B;
  B.color = color; B.mean = state->mean; B.m2 = state->m2; B.count = state->count; B.variance_out = variance_out;
  call.start(2);
  if (!call.rc) {
    call.mark(0);
    call.rc = launch_ac_accumulate(call.st, B, d_rects, n, max_patches, xres, reset ? 1 : 0);
    call.mark(1);
  }
  return call.finish(stats, 1, {0, 1}, {}, {0, 1});
}

int fjgpu_accumulate_tile_error(int device, int xres, int yres, const int32_t *rects, int n_rects, const fjgpu_accum_state *state,
    float lum_floor, float *errors_out, void *hip_stream, fjgpu_stats *stats)
{
  ImageCall call("fjgpu_accumulate_tile_error", hip_stream);
  const std::string &f = call.f;
  if (!state || !state->mean || !state->m2 || !state->count || !errors_out)
    return fail(FJGPU_EINVAL, f + ": null argument (state, its mean, m2 and count, and errors_out are required)");
  std::vector<int32_t> list;
  uint32_t max_patches = 0;
  if (const int e = ac_check_rects(f, xres, yres, rects, n_rects, &list, &max_patches)) return e;
  if (!(std::isfinite(lum_floor) && lum_floor > 0.f)) return fail(FJGPU_EINVAL, f + ": lum_floor must be finite and > 0");
  if ((uintptr_t) state->mean & 15u) return fail(FJGPU_EINVAL, f + ": the state's mean must be 16-byte aligned");
  if (const int e = call.open(device)) return e;
  const int n = (int) (list.size() / 4);
  fjgpu_stats none;
  std::memset(&none, 0, sizeof(none));
  if (n == 0) { if (stats) *stats = none; return 0; }
  DeviceBuffers W;
  const int32_t *d_rects = nullptr;
  float *d_err = nullptr;
  if (W.upload(list.data(), list.size(), &d_rects) || W.alloc((size_t) n, &d_err)) return fail(FJGPU_ENOMEM, f + ": device allocation failed");
  call.start(2);
  if (!call.rc) {
    call.mark(0);
    call.rc = launch_ac_tile_error(call.st, state->mean, state->m2, state->count, d_rects, n, xres, lum_floor, d_err);
    if (!call.rc && hipMemcpyAsync(errors_out, d_err, sizeof(float) * (size_t) n, hipMemcpyDeviceToHost, call.st) != hipSuccess) call.rc = -1;
    call.mark(1);
  }
  return call.finish(stats, 1, {0, 1}, {}, {0, 1});
}

}  // extern "C"
