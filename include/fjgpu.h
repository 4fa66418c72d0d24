/* fjgpu.h -- C ABI of the MI355X ray-intersection + integrator core
 * (libfjgpu.so, hand-written HIP for gfx950).
 *
 * This is the compute half of the drop-in boundary.  In the reference the
 * whole path lives behind one call,
 *     Renderer::RenderScene()            src/fj_renderer.cc:667-684
 * reached from SiRenderScene()           src/fj_scene_interface.cc:247-278
 * after prepare_render() has computed bounds, created the implicit groups and
 * built the accelerators (same file :1204-1222).  A maintainer of the
 * reference binds these entry points at exactly that spot:
 *
 *   fjgpu_scene_create   replaces build_accelerators()       src/fj_scene_interface.cc:1161-1202
 *                        (GridAccelerator::build             src/fj_grid_accelerator.cc:69-160,
 *                         BVHAccelerator::build              src/fj_bvh_accelerator.cc:79-107)
 *   fjgpu_render_tiles   replaces execute_rendering()'s      src/fj_renderer.cc:747-791
 *                        MtRunParallelLoop(render_tile)      src/fj_renderer.cc:1098-1121
 *                        i.e. FixedGridSampler::generate_samples, Camera::GetRay,
 *                        SlTrace / SlIlluminance / the shader plugins,
 *                        reconstruct_image + apply_pixel_filter, FrameBuffer::SetColor
 *   fjgpu_trace          exposes Accelerator::Intersect      src/fj_accelerator.cc:94-113
 *                        for ray batches (parity tests, SlSurfaceRayIntersect users)
 *
 * Plain pointers and sizes only; no C++ or torch types; no globals besides the
 * last-error string; every function returns 0 or a negative FJGPU_E* code.
 * There is no CPU fallback: without a GPU every compute call fails loudly.
 */
#ifndef FJGPU_H
#define FJGPU_H

#include <stdint.h>
#include "fj_scene_desc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  FJGPU_OK = 0,
  FJGPU_ENODEV = -1,        /* no HIP device / HIP runtime error */
  FJGPU_EINVAL = -2,        /* malformed description */
  FJGPU_EUNSUPPORTED = -3,  /* feature outside the device path (named in the error string) */
  FJGPU_ENOMEM = -4
};

typedef struct fjgpu_scene fjgpu_scene;

/* Per-launch device counters, summed over the call (all optional to read) */
typedef struct fjgpu_stats {
  fj_ray_counts rays;          /* same events the reference would count */
  uint64_t nodes_visited;      /* BLAS nodes fetched (128 B each: a 4-wide node) */
  uint64_t prims_tested;       /* triangle tests (36 B each: f32 vertices, or 72 B as f64) / curve tests */
  uint64_t insts_tested;       /* instance boxes tested (48 B each) */
  uint64_t rays_traced;        /* rays entering a trace kernel (closest + shadow) */
  uint64_t shadow_traversed;   /* shadow rays that survived the instance-box cull and walked a BLAS */
  double   trace_ms;           /* HIP-event time of the trace kernels (closest + shadow) */
  double   shade_ms;           /* shading / queue kernels */
  double   gen_ms;             /* sample + camera-ray generation */
  double   resolve_ms;         /* pixel filter */
  double   total_ms;           /* first launch -> last kernel done */
  uint32_t trace_launches;
  uint32_t batches;
  /* the traversal side per kernel (trace_ms is their sum), so that one kernel's HIP-event time
   * can be set against its own algorithmic bytes and against rocprofv3's average for it */
  double   closest_ms;         /* k_trace_closest launches */
  double   light_loop_ms;      /* k_shadow_cull launches (SlIlluminance light loop + instance-box cull) */
  double   shadow_walk_ms;     /* k_shadow_anyhit / k_shadow_trace launches */
  uint64_t shadow_nodes;       /* BLAS nodes fetched by the shadow walk alone (counting instantiation) */
  uint64_t shadow_prims;       /* triangle / curve tests of the shadow walk alone */
  uint64_t shadow_insts;       /* instance boxes tested by the shadow walk alone */
  uint32_t closest_launches, light_loop_launches, shadow_walk_launches;
  uint32_t interrupted;        /* 1: the batch callback asked to stop; the batches after that one were not rendered */
  double   sort_ms;            /* ray-queue sort in front of the closest-hit walk (option "ray_sort"; part of closest_ms) */
  uint64_t rays_sorted;        /* rays that went through it */
} fjgpu_stats;

/* Number of visible HIP devices (0 when there is none). */
int fjgpu_device_count(void);

/* Build the device scene on HIP device `device`: BLAS per mesh / curve set,
 * instance table with precomputed matrices, groups, lights, shaders and
 * textures resident in HBM.  The description is copied. */
int fjgpu_scene_create(const fj_scene_desc *desc, int device, fjgpu_scene **out);
void fjgpu_scene_destroy(fjgpu_scene *scene);

/* Tiling of a frame exactly as Tiler::GenerateTiles (src/fj_tiler.cc:56-113). */
int fjgpu_tile_count(const fj_render_desc *render);
int fjgpu_tile_rect(const fj_render_desc *render, int tile_id, int32_t rect[4]);

/* Render the listed tiles (NULL = all tiles of the render region) into a
 * DEVICE framebuffer `d_framebuffer` of xres*yres*4 float32 (RGBA, row-major,
 * the layout of FrameBuffer, src/fj_framebuffer.cc:130-133); pixels of tiles
 * not listed are left untouched.  Work is enqueued on `hip_stream`
 * (a hipStream_t passed as void*, NULL = default stream) and the call returns
 * after the stream has been synchronised. */
int fjgpu_render_tiles(fjgpu_scene *scene, const fj_render_desc *render,
    const int32_t *tile_ids, int n_tiles,
    float *d_framebuffer, void *hip_stream, fjgpu_stats *stats);

/* fjgpu_render_tiles plus a SAMPLE VARIANCE buffer: for every pixel of the listed tiles the variance of the luminance of the pixel's
 * filtered estimate, taken from the per-sample radiances the beauty pass holds when it resolves a batch -- the variance_in of
 * fjgpu_denoise_variance and the variance_spatial of fjgpu_denoise_temporal from the samples themselves, not from the finished frame.
 * The framebuffer, the ray counts and the stats are fjgpu_render_tiles's (same body, same launches; one more kernel per batch right after
 * the resolve, its time in resolve_ms).  csrc/device/fjgpu_sample_var_math.h is the one source of the arithmetic.  For pixel p, over the
 * window samples s the pixel filter reads for p (reconstruct_image / apply_pixel_filter: rate + 2 margin per axis), sums in f64:
 *   w_s = the filter's Gaussian weight of s for p, exp(-2 (xx xx + yy yy)) in f64;
 *   l_s = l(d), f32, l as in fjgpu_denoise_variance; d = the sample's rgb, or with d_albedo d_k = x_k / a'_k per channel with
 *         a'_k = albedo[p]_k > albedo_floor ? albedo[p]_k : albedo_floor -- the PIXEL's albedo (fjgpu_denoise_albedo's statements), so the
 *         result describes the demodulated luminance those two consumers work with;
 *   pass 1: S0 = sum w, S1 = sum w l, m = S1 / S0;    pass 2, same samples and weights: S2 = sum w (l - m)^2, Q = sum w^2;
 *   e = Q / S0^2 (1 / n for n equal weights);   V = (S2 / S0) e / (1 - e) -- for n equal weights the unbiased sample variance divided by n;
 *   V = 0 where e >= 1 (one sample); rounded to f32 once; a V that is negative or not finite (a non-finite sample) is written as 0.f.
 * d_variance is a DEVICE [yres][xres] f32 buffer; pixels of tiles not listed are left untouched in it.  d_albedo (may be NULL; then
 * albedo_floor is ignored) is a DEVICE [yres][xres][3] f32 buffer (fjgpu_render_aov_albedo's) of which only listed tiles' pixels are read.
 * Scenes with motion, a moving camera and area lights are served: their accumulators are the same.  If the call has to be repeated because
 * split shadow rays overflowed their queue (see "split_shadow"), the variance is written again with the frame.
 * Errors, before any device work, every message starting "fjgpu_render_tiles_variance:": FJGPU_EINVAL for a NULL scene, render, framebuffer
 * or variance, for an albedo_floor that is not finite and > 0 where d_albedo is set, and for a d_variance that overlaps the framebuffer or
 * the albedo; FJGPU_EUNSUPPORTED for the adaptive sampler (its resolved samples are interpolated, not independent).  Everything else is
 * fjgpu_render_tiles's. */
int fjgpu_render_tiles_variance(fjgpu_scene *scene, const fj_render_desc *render, const int32_t *tile_ids, int n_tiles,
    float *d_framebuffer, const float *d_albedo /* DEVICE [yres][xres][3] or NULL */, float albedo_floor,
    float *d_variance /* DEVICE [yres][xres] f32 */, void *hip_stream, fjgpu_stats *stats);

/* Batch callback.  fjgpu_render_tiles cuts its tile list into BATCHES (as many tiles as the wavefront
 * queues hold: a whole 1080p / 64 spp frame is one batch, option "batch_tiles"); `fn` is called on the
 * calling host thread each time a batch is complete on the device -- the tiles' pixels are final in the
 * device framebuffer -- with the ids of its tiles.  This is where the host side fires the reference's
 * per-sample `sample_done` hook, once per batch (CbReportSampleDone in integrate_samples,
 * src/fj_renderer.cc:1061-1096; a host call per sample is infeasible, SURVEY 8b "Threading").  A nonzero
 * return stops the call after this batch, like the reference's worker pool after a CALLBACK_INTERRUPT
 * (render_tile -> LoopStatus::Cancel, src/fj_renderer.cc:1098-1121): the remaining tiles are not rendered,
 * the call returns 0 and stats->interrupted is 1.  fn = NULL removes it.  (If a call has to be repeated
 * because split shadow rays overflowed their queue -- see "split_shadow" -- its batches are reported again.) */
typedef int (*fjgpu_batch_fn)(void *user, int device, const int32_t *tile_ids, int n_tiles);
int fjgpu_set_batch_callback(fjgpu_scene *scene, fjgpu_batch_fn fn, void *user);

/* Convenience: all tiles, result copied to a HOST buffer (xres*yres*4 floats). */
int fjgpu_render_frame(fjgpu_scene *scene, const fj_render_desc *render,
    float *h_framebuffer, fjgpu_stats *stats);

/* The same scene resident on several devices of this process: the host-side build (BLAS,
 * matrices, light samples) runs once, the result is uploaded to every device in `devices`.
 * out[n_devices]; on failure nothing is left allocated. */
int fjgpu_scene_create_multi(const fj_scene_desc *desc, const int *devices, int n_devices, fjgpu_scene **out);

/* One frame on the devices of `scenes` (replicas of one scene, fjgpu_scene_create_multi) -- the
 * reference's worker pool with GPUs for workers (execute_rendering, src/fj_renderer.cc:747-791;
 * MtRunParallelLoop, src/fj_multi_thread.cc:86-132).  Tile k of `tile_ids` (NULL = all tiles of
 * the render region) is rendered by scenes[k % n_scenes] on that device's own host thread; each
 * device packs its finished tiles into one slab, which crosses xGMI as one peer copy into
 * scenes[0]'s device; the assembled frame is copied to the HOST buffer once.  Pixels of tiles not
 * listed are 0.  stats: NULL or [n_scenes], one entry per device. */
int fjgpu_render_frame_multi(fjgpu_scene *const *scenes, int n_scenes, const fj_render_desc *render,
    const int32_t *tile_ids, int n_tiles, float *h_framebuffer, fjgpu_stats *stats);

/* Tile slabs of the multi-process split (one process per GPU, bench.py / distributed.py: tile t belongs to rank t % N and
 * the finished tiles travel to rank 0 in ONE exchange): pack copies the rectangles rects[k] = (xmin, ymin, xmax, ymax)
 * (DEVICE array, n_tiles x 4 int32) of the DEVICE framebuffer d_fb (xres pixels per row, RGBA f32) into d_slab, tile k at
 * pixel k * tile_px, rows of the rectangle's own width; unpack is the inverse (a rectangle of zero area is skipped: padding
 * entries of the shorter ranks).  One kernel launch each on `hip_stream`; no synchronisation. */
int fjgpu_pack_tiles(const float *d_fb, int xres, const int32_t *d_rects, int n_tiles, int tile_px, float *d_slab, void *hip_stream);
int fjgpu_unpack_tiles(float *d_fb, int xres, const int32_t *d_rects, int n_tiles, int tile_px, const float *d_slab, void *hip_stream);

/* Closest hit of n rays against group `group` (HOST arrays; copied in/out).
 * rays [n][8] = orig xyz, dir xyz, tmin, tmax.  out_t [n] (DBL_MAX on miss),
 * out_ids [n][2] = instance, primitive (-1 on miss), out_uv [n][2] = barycentric
 * u, v of the hit (may be NULL). */
int fjgpu_trace(fjgpu_scene *scene, int group, int n, const double *rays,
    double *out_t, int32_t *out_ids, double *out_uv, fjgpu_stats *stats);

/* First-hit AOV pass: the geometry behind every pixel -- depth for compositing, ids for mattes, position / normal / uv as
 * feature buffers, what lies under a pixel for picking.  Static scenes with the fixed-grid sampler only.
 *
 * Tiles, tile ids, the render region and "pixels of tiles not listed are left untouched" are exactly those of
 * fjgpu_render_tiles.  The samples are the beauty pass's own: a tile has nx * ny of them, rate * size + 2 * margin per axis
 * (FixedGridSampler::generate_samples, src/fj_fixed_grid_sampler.cc:33-84), sample k = y * nx + x takes draw k of the jitter
 * table and the same (u, v), and its camera ray is the static camera's (Camera::GetRay, src/fj_camera.cc:79-110).  ALL samples
 * of a tile are traced, the filter margin included, so stats->rays.camera equals the beauty pass's camera count for those tiles.
 * Only a pixel's OWN samples enter its reduction: for pixel (px, py) of a tile with corner (xmin, ymin) the rate_x * rate_y
 * samples with x in [margin_x + (px - xmin) * rate_x, ... + rate_x) and y likewise.  The NEAREST sample is the own sample
 * with the smallest t; on equal t the smallest k wins.  Its attributes are computed with the statements the shading kernel
 * uses for a hit (trace_surface's SurfaceInput setup):
 *   depth     (float) t
 *   position  Pw = M (M^-1 o + t M^-1 d), the instance's matrices (ObjectInstance::RayIntersect, src/fj_object_instance.cc:213-243)
 *   normal    normalize(M . ((1-u-v) n0 + u n1 + v n2)) from the mesh's per-corner normals where it has them, else its point
 *             normals (compute_shading_normal, src/fj_mesh.cc:108-120); NOT face-forwarded; zero for a mesh without normals
 *   uv        the f32 texture coordinates of Mesh::ray_intersect (src/fj_mesh.cc:285-290); zero for a mesh without them
 *   ids       instance, primitive, shading group (the face's group, 0 without face groups), shader index by the slot rule of
 *             ObjectInstance::GetShader (src/fj_object_instance.cc:177-191): a group out of range or an unassigned slot gives
 *             slot 0; -1 only if slot 0 is unassigned
 *   coverage  (float) hits / (float) samples among the pixel's own samples
 * A hit on a curve writes normal and uv zero, as Curve::ray_intersect leaves them (src/fj_curve.cc:211-229), the curve's index
 * in its set as the primitive and shading group 0.  A pixel none of whose own samples hits gets depth +INFINITY, ids -1 and
 * zeros elsewhere.
 *
 * The call allocates its buffers per call and frees them before it returns; it touches neither the scene's work arena nor its
 * options nor its call counters: beauty renders before and after it give the same pixels and counts.  The tile list is cut into
 * batches of at most "aov_batch_samples" samples (fjgpu_set_option; default, and 0: 4 M; a batch holds at least one tile).
 * Work is enqueued on `hip_stream` and the call returns after the stream has been synchronised.  stats (may be NULL):
 * rays.camera, gen_ms (sample generation), closest_ms = trace_ms (the closest-hit walk), resolve_ms (the reduction),
 * total_ms, batches, closest_launches; the traversal counters with option "count_nodes".
 * Errors: FJGPU_EUNSUPPORTED, the reason named in the error string, for the adaptive sampler, for a time-sampled camera and
 * for a scene with motion (query "has_motion"); FJGPU_EINVAL when every buffer pointer is NULL or an argument is NULL. */
typedef struct fjgpu_aov_buffers {   /* DEVICE pointers, row-major xres*yres, NULL = not wanted */
  float   *depth;      /* [1]  (float) t of the nearest sample, +INFINITY where no sample hits   */
  float   *position;   /* [3]  world-space hit point                                             */
  float   *normal;     /* [3]  interpolated shading normal in world space (not face-forwarded)   */
  float   *uv;         /* [2]  texture coordinates of the hit                                    */
  int32_t *ids;        /* [4]  instance, primitive, shading group (face group), shader index     */
  float   *coverage;   /* [1]  hits / samples among the pixel's own samples                      */
} fjgpu_aov_buffers;
int fjgpu_render_aov(fjgpu_scene *scene, const fj_render_desc *render, const int32_t *tile_ids, int n_tiles,
    const fjgpu_aov_buffers *buffers, void *hip_stream, fjgpu_stats *stats);

/* fjgpu_render_aov plus an ALBEDO buffer: the surface colour of a pixel without light, what a compositor expects next to depth and
 * normal and what fjgpu_denoise_albedo divides a beauty frame by.  One camera-ray generation and one closest-hit walk per batch serve
 * both: `buffers` (may be NULL, or all-NULL) is written as by fjgpu_render_aov, d_albedo (DEVICE [yres][xres][3] f32, may be NULL) gets
 * the MEAN over the pixel's own rate_x * rate_y samples of the per-sample albedo a, a miss counting 0 (so a silhouette pixel against the
 * empty background holds coverage x surface, as its beauty value does; a pixel no sample of which hits gets 0 0 0).  Per sample, f32,
 * every product one multiply, with the statements the shading kernel uses: shader by the slot rule above; tex(i) = the nearest-tap
 * Texture::Lookup of texture i at the hit's f32 texture coordinates (0, 0 on a curve or a mesh without uv), NO_TEXTURE_COLOR included;
 * Cd = 1 1 1 on a mesh, the lerp of the piece's end colours on a curve.
 *   no shader / unknown type   NO_SHADER_COLOR = 0.5 1 0
 *   ConstantShader             diffuse * tex(texture) where it has one, else diffuse
 *   PlasticShader              diffuse * tex(diffuse_map), or diffuse
 *   PathtracingShader          (Cd * tex(diffuse_map)) * diffuse
 *   HairShader                 Cd * diffuse
 *   GlassShader                1 1 1
 * The sum is taken in f64 and divided by the sample count in f64, rounded to f32 once: a pixel whose samples share one albedo holds
 * exactly that value, any other the f64 mean within one f32 ulp.
 * Everything else is fjgpu_render_aov's: tiles, region, untouched pixels, batches, transient buffers, stats (resolve_ms covers both
 * reductions) and the refusals.  FJGPU_EINVAL, the message naming fjgpu_render_aov_albedo, when neither a member of `buffers` nor
 * d_albedo is set. */
int fjgpu_render_aov_albedo(fjgpu_scene *scene, const fj_render_desc *render, const int32_t *tile_ids, int n_tiles,
    const fjgpu_aov_buffers *buffers /* may be NULL */, float *d_albedo /* DEVICE [yres][xres][3], may be NULL */,
    void *hip_stream, fjgpu_stats *stats);

/* Ranked id/coverage mattes (Cryptomatte-style): per pixel the `ranks` keys with the greatest share of the pixel and those shares, so
 * that a compositor can isolate an object at the beauty frame's anti-aliased edges.  The AOV pass's camera rays and closest-hit walk,
 * then one reduction over the hit records.  For a pixel p, samples s with a key k_s and a weight w_s:
 *   filtered = 1   the samples of the filter window the beauty pass resolves p from, w_s = its Gaussian weight in f64
 *                  (exp(-2 (xx xx + yy yy)), xx = 2 (xres u - (px + .5)) / filter_w, yy likewise from yres (1 - v)): the shares are
 *                  those of the beauty pixel's blend
 *   filtered = 0   the pixel's own rate_x * rate_y samples (fjgpu_render_aov's), w_s = 1
 *   k_s            -1 for a miss; key FJGPU_MATTE_KEY_INSTANCE: the hit's instance (ids[0] of the ids AOV); FJGPU_MATTE_KEY_SHADER: the
 *                  shader index by the slot rule above (ids[3]) of the sample's own shading group -- a hit whose shader is unassigned
 *                  has key -1 as well.  A key of -1 is never ranked; its weight counts in W only.
 *   W = sum of w_s over all samples.  Keys are visited in ascending order; A(key) = sum of w_s with that key (f64); (key, A) is inserted
 *   into a list of `ranks` entries before the first entry whose weight is strictly smaller, so equal weights stay in ascending key
 *   order; what leaves the list (or never enters a full one) adds its weight to R.
 *   ids[r], coverage[r] = (float) (A_r / W) rank by rank, -1 and 0 for an empty rank; rest = (float) (R / W), the share of hit keys that
 *   did not fit into `ranks`; distinct = the number of keys visited.  sum(coverage) + rest is the pixel's hit share (filtered: the alpha of
 *   an opaque scene's beauty pixel).  With filtered = 0 every sum is a count and the quotients are (float) count / (float) samples, the
 *   statement of fjgpu_render_aov's coverage.
 * Limits: those of fjgpu_render_aov (static scene and camera, fixed-grid sampler, one device); first hits only -- the matte of a glass
 * object is the glass, not what is seen through it.
 * Everything else is fjgpu_render_aov's: tiles, region, untouched pixels, batches ("aov_batch_samples"), transient buffers, stats
 * (resolve_ms is the matte reduction) and the refusals, the messages naming fjgpu_render_aov_matte.  FJGPU_EINVAL, with the reason, for
 * a NULL description or buffer struct, a NULL ids or coverage buffer, an unknown key and ranks outside 1..FJGPU_MATTE_MAX_RANKS. */
#define FJGPU_MATTE_KEY_INSTANCE 0   /* ids[0] of the ids AOV */
#define FJGPU_MATTE_KEY_SHADER   1   /* ids[3]: ObjectInstance::GetShader of the sample's shading group */
#define FJGPU_MATTE_MAX_RANKS    16
typedef struct fjgpu_matte_desc { int32_t key, ranks, filtered, pad; } fjgpu_matte_desc;
typedef struct fjgpu_matte_buffers {      /* DEVICE pointers, row-major */
  int32_t *ids;        /* [yres*xres*ranks]  key of rank r, -1 = empty rank     (required) */
  float   *coverage;   /* [yres*xres*ranks]  its share of the pixel, 0 if empty (required) */
  float   *rest;       /* [yres*xres]  share of hit keys that did not fit into `ranks` (optional) */
  int32_t *distinct;   /* [yres*xres]  number of distinct keys among the pixel's samples (optional) */
} fjgpu_matte_buffers;
int fjgpu_render_aov_matte(fjgpu_scene *scene, const fj_render_desc *render, const int32_t *tile_ids, int n_tiles,
    const fjgpu_matte_desc *matte, const fjgpu_matte_buffers *buffers, void *hip_stream, fjgpu_stats *stats);

/* Diagnostics: the camera rays of one tile exactly as fjgpu_render_aov (and the beauty pass) traces them, HOST arrays:
 * rays8 [n][8] = orig xyz, dir xyz, znear, zfar in sample order k = y * nx + x (margin samples included) -- the layout
 * fjgpu_trace takes.  Writes at most `cap` rays (cap 0: none, rays8 may be NULL); returns the tile's sample count n, or a
 * negative error (the refusals of fjgpu_render_aov). */
int fjgpu_camera_samples(fjgpu_scene *scene, const fj_render_desc *render, int tile_id, double *rays8, int cap);

/* Denoiser: an edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch, HPG 2010) over a beauty frame, guided by the
 * feature buffers of fjgpu_render_aov.  Device buffers in, device buffers out; no scene handle.  A spatial filter of ONE frame: albedo
 * demodulation is fjgpu_denoise_albedo below (without it textured surfaces lean on the colour term), variance guidance is fjgpu_denoise_variance further below, reuse of earlier frames is fjgpu_denoise_temporal below that.
 *
 * All arithmetic is f32 without fused multiply-adds, sums left to right (csrc/device/fjgpu_denoise_math.h is the one source of the
 * kernel, of the host twin the CPU tests run and of the constants).  h = (1/16, 1/4, 3/8, 1/4, 1/16).  For iteration i = 0 ..
 * iterations-1 with s = 2^i, C = color_in (i = 0) or the previous iteration's output, and every region pixel p: the taps q = p + s (dx, dy),
 * dy = -2..2 (outer), dx = -2..2 (inner).  A tap outside the region is skipped; with stop_at_ids a tap with ids[q][0] != ids[p][0] is
 * skipped (background, -1, is an id like any other: it never bleeds into geometry).  Otherwise
 *   d2c = (Cq.r-Cp.r)^2 + (Cq.g-Cp.g)^2 + (Cq.b-Cp.b)^2, d2n and d2x likewise from normal and position,
 *   e = d2c k_c + d2n k_n + d2x k_x,  w = (h[dy+2] h[dx+2]) expf(-e)     (one expf per tap, of the summed exponent)
 *   sum += w Cq over all four channels (alpha is filtered with the same weights), wsum += w;   out_p = sum / wsum
 * (the centre tap contributes 9/64, so wsum > 0).  k_c = (float) (1 / (sigma_color 2^-i)^2), k_n = (float) (1 / sigma_normal^2),
 * k_x = (float) (1 / sigma_position^2), computed in f64 and rounded once (capped at FLT_MAX); k = 0 for a term that is off.
 *
 * Only pixels of the region are read and written; pixels of color_out outside it stay untouched.  color_out may EQUAL color_in (any
 * other overlap of the two is not allowed); both must be 16-byte aligned.  The inputs must be finite, and so must the squared
 * differences of neighbouring pixels (a NaN or an infinity spreads over the filter's support).
 * Scratch is allocated per call and freed before the call returns: two RGBA frames of the region and one 32-byte guide record per region
 * pixel.  Work is enqueued on `hip_stream` and the call returns after the stream has been synchronised.  stats (may be NULL): gen_ms (the
 * guide pack), resolve_ms (the filter iterations), total_ms, batches = iterations.
 * Errors: FJGPU_EINVAL, the message naming fjgpu_denoise, for a NULL desc / color_in / color_out, an invalid region, iterations outside
 * 1..8, a NaN sigma, a misaligned colour pointer; FJGPU_ENODEV when no device is visible. */
typedef struct fjgpu_denoise_desc {
  int32_t xres, yres;          /* row-major frame the buffers describe                                   */
  int32_t region[4];           /* xmin ymin xmax ymax, the convention (and validation) of fj_render_desc */
  int32_t iterations;          /* 1..8; iteration i uses tap spacing 2^i                                 */
  float   sigma_color;         /* > 0, or <= 0 / +inf: term off; halves every iteration                  */
  float   sigma_normal;        /* likewise; ignored where `normal` is NULL                               */
  float   sigma_position;      /* likewise, world units; ignored where `position` is NULL                */
  int32_t stop_at_ids;         /* 1: a tap whose instance id (ids[0]) differs from the centre's weighs 0 */
} fjgpu_denoise_desc;

int fjgpu_denoise(int device, const fjgpu_denoise_desc *desc,
                  const float *color_in,   /* DEVICE [yres][xres][4] RGBA f32                */
                  const float *normal,     /* DEVICE [.][.][3] or NULL                       */
                  const float *position,   /* DEVICE [.][.][3] or NULL                       */
                  const int32_t *ids,      /* DEVICE [.][.][4] or NULL (then stop_at_ids = 0)*/
                  float *color_out,        /* DEVICE [.][.][4]; may equal color_in           */
                  void *hip_stream, fjgpu_stats *stats);

/* fjgpu_denoise with albedo demodulation: the filter sees the illumination, not the texture.  albedo NULL: fjgpu_denoise, bit for bit
 * (albedo_floor is ignored).  Else, for every region pixel and k = r, g, b, in f32:
 *   a'_k = albedo_k > albedo_floor ? albedo_k : albedo_floor;   D_k = C_k / a'_k  (one IEEE division);
 *   the filter above runs on (D_r, D_g, D_b, C_alpha), so its colour term compares demodulated values;
 *   out_k = F_k * a'_k  (one multiply); alpha is the filter's.
 * `albedo` is a DEVICE [yres][xres][3] f32 buffer (fjgpu_render_aov_albedo's) of which only region pixels are read; color_out may still
 * equal color_in.  One more pass over the region before the iterations and one after them; the scratch is the same.  stats: gen_ms
 * includes the demodulating copy, resolve_ms the remodulation.
 * Errors: those of fjgpu_denoise; FJGPU_EINVAL naming albedo_floor where albedo is set and albedo_floor is not finite and > 0. */
int fjgpu_denoise_albedo(int device, const fjgpu_denoise_desc *desc, const float *color_in, const float *normal, const float *position,
    const int32_t *ids, const float *albedo /* DEVICE [yres][xres][3] or NULL */, float albedo_floor, float *color_out,
    void *hip_stream, fjgpu_stats *stats);

/* Variance-guided denoising: the filter above with the edge-stopping function of SVGF (Schied et al., HPG 2017, 4.2 and 4.4) in place of
 * the colour term.  The luminance distance of a tap is measured in units of the local standard deviation, and the variance is filtered
 * along with the colour, so one sigma_luminance serves noisy and clean pixels alike.  The variance is the caller's (variance_in) or a
 * spatial estimate from the frame itself under the guides -- what SVGF falls back to for pixels without temporal history.
 * csrc/device/fjgpu_denoise_var_math.h is the one source of the arithmetic: f32 without fused multiply-adds, sums left to right, one expf
 * per tap, taps dy outer and dx inner; a tap outside the region is skipped, and so is (stop_at_ids) a tap with ids[q][0] != ids[p][0].
 * k_n and k_x are those of fjgpu_denoise.  l(C) = 0.2126f C.r + 0.7152f C.g + 0.0722f C.b.
 *
 * Estimate (fjgpu_denoise_estimate_variance; fjgpu_denoise_variance with variance_in NULL): for every region pixel p over the taps
 * q = p + (dx, dy), dx, dy = -3..3, with w = expf(-(d2n k_n + d2x k_x)) (the guides only; the centre weighs 1):
 *   pass 1: s0 += w, s1 += w l_q, m = s1 / s0;    pass 2, same taps and weights: d = l_q - m, s2 += w (d d);    V = s2 / s0, V = V > 0 ? V : 0.
 * Iteration i = 0 .. iterations-1, spacing 2^i, colour C and variance V (the estimate or variance_in at i = 0, then the previous outputs):
 *   g = the 3 x 3 average of V around p at spacing 1, weights k3[dy+1] k3[dx+1], k3 = (1/4, 1/2, 1/4), taps outside the region skipped,
 *       divided by the sum of the weights used (no id stop);
 *   k_l = 1.f / (sigma_luminance sqrtf(g) + 1e-6f), or 0.f (term off) for sigma_luminance <= 0 or +inf; it does not halve per iteration --
 *       the variance shrinks by itself;
 *   e = fabsf(l_q - l_p) k_l + d2n k_n + d2x k_x,  w = (h[dy+2] h[dx+2]) expf(-e) over the 5 x 5 taps,
 *   sum += w C_q (four channels), wsum += w, vsum += (w w) V_q;   C' = sum / wsum,  V' = vsum / (wsum wsum).
 * With sigma_luminance = 0 the colours are fjgpu_denoise's with sigma_color = 0, bit for bit.
 *
 * desc->sigma_color is ignored by both entries (a NaN is still refused), desc->iterations by the estimate.  Only region pixels of any buffer
 * are read or written.  The variance buffers are DEVICE [yres][xres] f32; variance_in must be finite and >= 0.  color_out may equal
 * color_in; variance_out must not overlap variance_in or a colour buffer (equal pointers are refused).  With albedo (fjgpu_denoise_albedo's
 * demodulation, same kernels) the order is demodulate, estimate on the demodulated frame, iterate, remodulate, and the variances are
 * those of the demodulated luminance.  Scratch per call: fjgpu_denoise's plus two f32 planes of the region.  stats: gen_ms covers the guide
 * pack, the demodulation and the estimate, resolve_ms the iterations and the remodulation, batches = iterations (0 for the estimate alone).
 * Errors: those of fjgpu_denoise_albedo and a NaN sigma_luminance, each message naming the function called; FJGPU_ENODEV when no device
 * is visible. */
int fjgpu_denoise_estimate_variance(int device, const fjgpu_denoise_desc *desc,
    const float *color, const float *normal, const float *position, const int32_t *ids,
    float *variance_out /* DEVICE [yres][xres] f32 */, void *hip_stream, fjgpu_stats *stats);

int fjgpu_denoise_variance(int device, const fjgpu_denoise_desc *desc, float sigma_luminance,
    const float *color_in, const float *normal, const float *position, const int32_t *ids,
    const float *albedo /* or NULL */, float albedo_floor,
    const float *variance_in  /* DEVICE [yres][xres] f32, or NULL: estimated as above */,
    float *color_out, float *variance_out /* or NULL */, void *hip_stream, fjgpu_stats *stats);

/* The estimate of the frame divided by its albedo: the first stage of fjgpu_denoise_variance with an albedo -- demodulate (fjgpu_denoise_albedo's
 * statements), then the estimate above -- with the estimate as the result.  It is the variance of the demodulated luminance, the quantity the
 * moments of fjgpu_denoise_temporal describe, and so that call's variance_spatial where an albedo is in use.  albedo NULL:
 * fjgpu_denoise_estimate_variance, bit for bit.  Scratch: the guide records and one RGBA frame of the region.  Errors: those of
 * fjgpu_denoise_estimate_variance, the messages naming this function; FJGPU_EINVAL for an albedo_floor that is not finite and > 0 and for a
 * variance_out that is the albedo buffer. */
int fjgpu_denoise_estimate_variance_albedo(int device, const fjgpu_denoise_desc *desc,
    const float *color, const float *normal, const float *position, const int32_t *ids,
    const float *albedo /* DEVICE [yres][xres][3] or NULL */, float albedo_floor,
    float *variance_out /* DEVICE [yres][xres] f32 */, void *hip_stream, fjgpu_stats *stats);

/* Camera of a resident scene.  A sequence over a static set -- a turntable, a fly-through -- moves nothing but the camera, and the camera is
 * host-side state of the scene that every render call copies into its launch parameters: setting it costs no device work and no BLAS build.
 * get: the camera the scene renders with -- the desc it was created with, or last set to.
 * set: recomputes what fjgpu_scene_create derives from desc->camera for a static camera, with the same statements (the transform's matrix
 * at time 0, fov, znear, zfar) and touches nothing else: not the work arena, the options, the counters, the light cones or the sort grid.
 * After set(c) every render, trace, AOV and camera-sample call gives the bits and the ray counts of a scene freshly created with camera c.
 * Errors: FJGPU_EINVAL for a NULL argument and for a sample count outside 1..FJ_MAX_XFORM_SAMPLES ("camera transform sample count out of
 * range", as at creation); FJGPU_EUNSUPPORTED, the reason in the message, for a camera with more than one sample in any channel and for a
 * scene that was created with a time-sampled camera (its buffers and random streams were sized for that). */
int fjgpu_scene_get_camera(const fjgpu_scene *scene, fj_camera_desc *out);
int fjgpu_scene_set_camera(fjgpu_scene *scene, const fj_camera_desc *camera);

/* The view of a frame: what it takes to find a world point in the frame the scene's current camera renders with `render`.  No device work.
 * With the conventions of Camera::GetRay and FixedGridSampler::generate_samples -- u = (x + .5) / xres, v = 1 - (y + .5) / yres, the ray's
 * target ((u - .5) uv_size_x, (v - .5) uv_size_y, -1) in camera space -- the projection of the world point P is, in f64,
 *   c  = world_to_camera * (P, 1);   visible only if c.z < 0
 *   fx = (c.x / -c.z / uv_size[0] + .5) * xres - .5
 *   fy = (.5 - c.y / -c.z / uv_size[1]) * yres - .5
 * so a point seen through the centre of pixel (x, y) projects to (fx, fy) = (x, y).
 * Errors: the static-camera refusals of fjgpu_render_aov (adaptive sampler, time-sampled camera, scene with motion), FJGPU_EINVAL for NULL. */
typedef struct fjgpu_view {
  double world_to_camera[12];   /* rows of the 3 x 4 inverse of the camera's transform (the Minv of MakeTransform) */
  double uv_size[2];            /* Camera::compute_uv_size with aspect = xres / yres, as the render calls set it    */
  int32_t xres, yres;
} fjgpu_view;
int fjgpu_scene_view(const fjgpu_scene *scene, const fj_render_desc *render, fjgpu_view *out);

/* Temporal accumulation (SVGF, Schied et al., HPG 2017, 4.1): the frame in front of fjgpu_denoise_variance for a SEQUENCE of a static scene.
 * The world position of every pixel is projected into the previous frame; the history found there -- accumulated colour, the first and
 * second moment of luminance, the history length -- is fetched bilinearly from the taps that still show the same surface and the new
 * frame is blended in.  The running mean over N frames is worth about N times the samples, and its moments are a per-pixel variance of the
 * pixel's own values over time: what variance_in of fjgpu_denoise_variance is for.  Device buffers in and out; no scene handle.
 * csrc/device/fjgpu_temporal_math.h is the one source of the arithmetic (kernel, host twin of the CPU tests; tests/temporal_model.py
 * restates it): f32 without fused multiply-adds, sums left to right, the projection alone in f64.
 *
 * For every region pixel p with colour C, guides P, N and I = ids[p][0]:
 *   luminance   L = l(D), l of fjgpu_denoise_variance; D = C.rgb / max(albedo, albedo_floor) per channel where there is an albedo, else C.rgb.
 *               The accumulated colour itself stays modulated: it is a beauty frame.
 *   no history  C' = C, m1 = L, m2 = L L, len = 1: where prev is NULL, I < 0 (background), P is not finite, the projection is not visible or
 *               not finite, or the valid weight below is <= 1e-4f.
 *   fetch       (fx, fy) = P through prev_view as above; x0 = floor(fx), y0 = floor(fy), a = (float) (fx - x0), b = (float) (fy - y0); the taps
 *               q = (x0 + i, y0 + j), j outer, i inner, weigh (i ? a : 1 - a) * (j ? b : 1 - b).  A tap is valid if it lies in the region,
 *               prev_ids[q][0] == I, |prev_position[q] - P|^2 <= tol_position^2, dot(prev_normal[q], N) >= cos_normal and prev->length[q] >= 1
 *               (a comparison with a NaN fails; a term that is off compares nothing).  H_colour (4), H_moments (2), H_len: the weighted
 *               sums over the valid taps, each divided by the valid weight.
 *   blend       n = min(H_len + 1, max_history), alpha = max(1 / n, alpha_min), X' = H + alpha (X - H) for X in {C, (L, L L)}; len' = n.
 *   variance    v = max(0, m2' - m1' m1'); where n < min_history_variance and variance_spatial is given, v = variance_spatial[p] (SVGF's
 *               fallback: fjgpu_denoise_estimate_variance of the current frame).
 * Only region pixels of any buffer are read or written.  `next` and variance_out must not overlap `prev`, each other or any input -- the
 * fetch reads arbitrary previous pixels -- : equal or overlapping buffers are refused.  color, prev->color and next->color are 16-byte
 * aligned.  One kernel launch, no scratch, about 170 bytes of compulsory traffic per pixel with an albedo.  Work is enqueued on `hip_stream`
 * and the call returns after the stream has been synchronised.  stats (may be NULL): resolve_ms = total_ms, batches = 1.
 * Errors: FJGPU_EINVAL, every message starting "fjgpu_denoise_temporal:", for a NULL desc, colour, guide (position, normal, ids and the
 * previous frame's three where prev is set), prev_view (where prev is set), next or member of a history; an invalid region; alpha_min
 * outside (0, 1]; max_history < 1; a NaN parameter; an albedo_floor that is not finite and > 0 where there is an albedo; overlapping
 * buffers; a misaligned colour pointer; a prev_view whose resolution is not positive.  All of them are decided before any device call.
 * FJGPU_ENODEV when no device is visible.
 *
 * Limits.  Static scenes, a static camera per frame and the fixed-grid sampler: those of the AOV pass, whose buffers this reads.  Nothing
 * that moves with the camera on a surface is reprojected -- reflections, refractions, highlights, shadows of moving lights: the colour history
 * of a glass pixel follows the glass surface, not what is seen through it.  Two frames from the same camera under the same "sampler_seed" (fjgpu_set_option)
 * are identical and accumulating them gains nothing; under different seeds they are independent draws.  A standing camera fetches its
 * history at the pixel it came from only if `position` is the hit through the pixel's centre: fjgpu_render_aov's position is the hit of the
 * pixel's nearest own sample, 0.28 pixels from the centre on average in the 64 x 48 Cornell box, and with it the history is resampled once
 * per frame (tests/test_gpu_accumulate.py has the figures; gpu.TemporalDenoiser passes a point on the centre's ray where it reseeds or the
 * camera has not moved, and then keys the fetch by the pixel, since f32's rounding of the point leaves a neighbour tap of weight 2e-6).  The exact running
 * mean of a view that stands is fjgpu_accumulate below.  There is no Si* entry: the reference's interface has no such call. */
typedef struct fjgpu_temporal_history {   /* DEVICE pointers, row-major xres*yres */
  float *color;        /* [4]  accumulated RGBA                                  */
  float *moments;      /* [2]  first and second moment of (demodulated) luminance */
  float *length;       /* [1]  history length, >= 1 on every pixel written        */
} fjgpu_temporal_history;

typedef struct fjgpu_temporal_desc {
  int32_t xres, yres;            /* row-major frame the buffers describe                                          */
  int32_t region[4];             /* xmin ymin xmax ymax: the convention (and validation) of fjgpu_denoise_desc    */
  float   alpha_min;             /* in (0, 1]: the least weight of the new frame (1: no accumulation)             */
  float   max_history;           /* >= 1: the history length saturates here                                       */
  float   tol_position;          /* world units; <= 0 or +inf: term off                                           */
  float   cos_normal;            /* <= -1: term off                                                               */
  float   min_history_variance;  /* shorter histories take variance_spatial (where given)                         */
  float   albedo_floor;          /* fjgpu_denoise_albedo's; ignored where `albedo` is NULL                        */
} fjgpu_temporal_desc;

int fjgpu_denoise_temporal(int device, const fjgpu_temporal_desc *desc,
    /* current frame  */ const float *color, const float *position, const float *normal, const int32_t *ids,
                         const float *albedo /* [3] or NULL */, const float *variance_spatial /* [yres][xres] or NULL */,
    /* previous frame */ const fjgpu_view *prev_view, const float *prev_position, const float *prev_normal, const int32_t *prev_ids,
                         const fjgpu_temporal_history *prev /* NULL: first frame */,
    /* out            */ const fjgpu_temporal_history *next, float *variance_out /* [yres][xres] or NULL */,
    void *hip_stream, fjgpu_stats *stats);

/* fjgpu_denoise_temporal with history rectification by variance clipping (Salvi, "An excursion in temporal supersampling", GDC 2016): between
 * the fetch and the blend the fetched history is clipped to a box around the CURRENT frame's values in a window about the pixel.  Radiance that
 * moves over a surface -- an emitter's rim under the pixel filter, highlights, reflections, shadows -- is invisible to ids, positions and
 * normals, so its history is accepted and is wrong; the box is what the current frame says the pixel can plausibly be.  clamp NULL: this
 * is fjgpu_denoise_temporal, bit for bit in every output.  The arithmetic is that pass's -- f32 without fused multiply-adds, sums left to
 * right, csrc/device/fjgpu_temporal_math.h its one source (fj_tp_clamp; tests/temporal_clamp_model.py restates it) -- up to and
 * including H /= valid weight.  A pixel without history is that pass's, and amount[p] = 0.  For a pixel p with history H_colour (4), (h1, h2):
 *   window   taps q = p + (dx, dy), dy = -radius..radius outer, dx = -radius..radius inner.  A tap outside the region is skipped; with
 *            stop_at_ids so is a tap with ids[q][0] != ids[p][0]; the centre always counts.  cnt = the sum of 1.f over the taps that count.
 *   box      for each of five values X -- the four channels of the current colour C_q, and L_q, the luminance above computed for pixel q
 *            (with q's albedo where there is one) --: pass 1  s1 += X_q, m = s1 / cnt;  pass 2, same taps  d = X_q - m, s2 += d * d,
 *            sd = sqrtf(s2 / cnt);  lo = m - gamma * sd, hi = m + gamma * sd.
 *   colour   H'_k = H_k < lo_k ? lo_k : (H_k > hi_k ? hi_k : H_k) for the four colour channels.
 *   moments  h1' = h1 clipped likewise against the box of L; h2' = h2 where h1' == h1, else h2' = (h2 - h1 * h1) + h1' * h1': the history keeps
 *            its spread around the moved mean.  The history length is untouched.
 *   amount   amount[p] = the largest of |H'_k - H_k| over r, g, b (where amount is not NULL).
 *   then     blend and variance of fjgpu_denoise_temporal from H', h1', h2'.
 * Inputs must be finite.  A non-finite value of X among the taps that count makes that X's m, sd, lo and hi NaN; every comparison with
 * them fails, so that value of the history passes unclipped (and amount counts nothing for it) on every pixel whose window holds the tap.
 * Only region pixels of any buffer are read or written, amount included.  amount must not overlap any input, prev, next or variance_out.
 * One kernel launch (k_tp_accumulate_clamped<radius>: the block's tile and halo of the current frame staged in LDS), no scratch, no
 * atomics.  stats as fjgpu_denoise_temporal.
 * Errors, all decided before any device call, every message starting "fjgpu_denoise_temporal_clamped:": those of fjgpu_denoise_temporal
 * first and in its order; then, for a clamp that is not NULL, a radius outside 1..3; a gamma that is NaN, infinite or <= 0; an amount
 * that overlaps another buffer.  FJGPU_ENODEV when no device is visible. */
typedef struct fjgpu_temporal_clamp {
  int32_t radius;        /* 1..3: the window is (2 radius + 1)^2 pixels of the CURRENT frame */
  float   gamma;         /* finite, > 0: half-width of the box in standard deviations        */
  int32_t stop_at_ids;   /* 1: a tap whose ids[q][0] differs from the centre's is skipped    */
  int32_t _pad;
  float  *amount;        /* DEVICE [yres][xres] f32 or NULL: how far the history was moved    */
} fjgpu_temporal_clamp;

int fjgpu_denoise_temporal_clamped(int device, const fjgpu_temporal_desc *desc, const fjgpu_temporal_clamp *clamp /* NULL: no clamp */,
    /* current frame  */ const float *color, const float *position, const float *normal, const int32_t *ids,
                         const float *albedo /* [3] or NULL */, const float *variance_spatial /* [yres][xres] or NULL */,
    /* previous frame */ const fjgpu_view *prev_view, const float *prev_position, const float *prev_normal, const int32_t *prev_ids,
                         const fjgpu_temporal_history *prev /* NULL: first frame */,
    /* out            */ const fjgpu_temporal_history *next, float *variance_out /* [yres][xres] or NULL */,
    void *hip_stream, fjgpu_stats *stats);

/* Progressive accumulation: the running mean of frames of ONE view that differ only in their "sampler_seed" (fjgpu_set_option), the
 * variance of that mean per pixel, and its reduction to one error per tile -- so that a frame can be refined by rendering it again, and
 * only the tiles that have not converged are rendered again (the tile list of fjgpu_render_tiles).  Device buffers in and out; no scene
 * handle.  csrc/device/fjgpu_accum_math.h is the one source of the arithmetic (kernels, host twin of the CPU tests;
 * tests/accumulate_model.py restates it): f32 without fused multiply-adds in the order written here, the tile's sum alone in f64.
 *
 * fjgpu_accumulate, for every pixel of a listed rectangle with new colour x (RGBA) and state (mean[4], m2, count):
 *   reset      != 0: the state read counts as zero, whatever is stored (NaN included).
 *   skip       a channel of x that is not finite: the state stays as read (as zero under reset, and zero is then what is stored) -- a
 *              firefly NaN must not poison the mean.
 *   update     n = count + 1;  mean_k' = mean_k + (x_k - mean_k) / n for the four channels;  with l = l(x.rgb) and m = l(mean.rgb) of the mean
 *              BEFORE the update (l of fjgpu_denoise_variance: it is linear, so the luminance mean is not a plane of its own):
 *              d = l - m;  m' = m + d / n;  m2' = m2 + d * (l - m');  count' = n.
 *   variance   variance_out = count' >= 2 ? m2' / (count' * (count' - 1)) : 0 -- the variance of the MEAN, the quantity
 *              fjgpu_denoise_variance takes as variance_in (of a skipped pixel: from the state it keeps).
 * fjgpu_accumulate_tile_error, one value per listed rectangle: e_p = sqrtf(variance as above) / max(l(mean.rgb), lum_floor) per pixel; the
 * f64 sum of e_p over the rectangle in a fixed order (fjgpu_accum_math.h; a serial sum differs by the rounding of f64 sums), divided by the
 * pixel count and rounded to f32.  A rectangle with a pixel of count < 2 has the error +INFINITY.  Only n_rects floats cross to the host.
 *
 * rects: HOST [n_rects][4] = xmin ymin xmax ymax (fjgpu_tile_rect's), each non-empty and inside the frame, no two overlapping (not
 * checked: a pixel in two rectangles is updated by two threads); NULL: the whole frame, n_rects is not read; n_rects 0: nothing is done.
 * Pixels outside the rectangles are neither read nor written, in any buffer.  color must not overlap the state, variance_out neither the
 * state nor color; color and state->mean are 16-byte aligned.  One launch of k_ac_accumulate (blocks of 16 x 16 pixels over (rectangle,
 * patch), about 64 bytes per pixel, no LDS) or k_ac_tile_error (one block per rectangle: wave butterflies and one LDS step); no atomics,
 * no scratch memory.  Work is enqueued on `hip_stream` and the call returns after the stream has been synchronised.  stats (may be NULL):
 * resolve_ms = total_ms, batches = 1.
 * Errors, all decided before any device call, FJGPU_EINVAL with a message that starts with the entry's name: a NULL color, state, member of
 * the state or errors_out; a resolution that is not positive; n_rects < 0; a rectangle that is empty or not inside the frame; overlapping
 * buffers (fjgpu_accumulate); a lum_floor that is not finite and > 0 (fjgpu_accumulate_tile_error); a misaligned color or mean; more than
 * 2^31 - 1 blocks.  FJGPU_ENODEV when no device is visible.
 *
 * Limits.  Frames are weighted alike: no inverse-variance weighting.  The seed is a single scene's: fjgpu_render_frame_multi and
 * fjgpu_scene_create_multi's replicas are not seeded together (each replica keeps its own option, default 0).  There is no Si* or
 * bin/scene entry.  The CPU oracle has no seed: a seeded frame has no oracle render, only the oracle's trace of its camera rays. */
typedef struct fjgpu_accum_state {   /* DEVICE, row-major xres*yres */
  float *mean;    /* [4] running mean of RGBA             */
  float *m2;      /* [1] Welford M2 of the luminance       */
  float *count;   /* [1] frames accumulated in this pixel  */
} fjgpu_accum_state;

int fjgpu_accumulate(int device, int xres, int yres, const int32_t *rects /* HOST [n][4] xmin ymin xmax ymax, NULL = whole frame */,
    int n_rects, const float *color /* [4] */, const fjgpu_accum_state *state, int reset, float *variance_out /* [1] or NULL */,
    void *hip_stream, fjgpu_stats *stats);

int fjgpu_accumulate_tile_error(int device, int xres, int yres, const int32_t *rects, int n_rects,
    const fjgpu_accum_state *state, float lum_floor, float *errors_out /* HOST [n_rects] */, void *hip_stream, fjgpu_stats *stats);

/* Tunables (all have defaults): "sampler_seed" 0..65535 (default 0; any other value: FJGPU_EINVAL naming the option and the range): the
 * random streams of the beauty pass.  0: the reference's -- every call uploads and launches exactly what it did before the option
 * existed.  s != 0: the jitter and time tables are the draws of the reference's seeded generator, XorShift(s) (src/fj_random.cc:18-24), in
 * the layout of the unseeded tables, and the sample uid behind the pathtracing shader's, the area lights' and the motion's streams is
 * that of tile id + 4096 s ("Random streams").  It applies alike to fjgpu_render_tiles, fjgpu_render_tiles_variance,
 * fjgpu_render_frame, the three AOV entries, fjgpu_camera_samples and the adaptive sampler, which agree with each other under one seed;
 * the scene's cached tables are rebuilt when the seed changes or the table grows, and not otherwise.  fjgpu_scene_query("sampler_seed")
 * returns it.  With a jitter of 0, no pathtracing shader, no area light and no motion nothing is drawn and the seed changes nothing.
 * "batch_tiles" tiles per wavefront batch, "batch_samples" samples per batch where batch_tiles is 0
 * (0, the default: as many as the memory budget holds -- fastest where frames repeat; a caller that renders one frame per scene
 * sets a few M: the work arena shrinks from ~110 GB to a few GB at the headline size and the cold frame starts sooner),
 * "count_nodes" 0/1 enable traversal event counters, "overlap_shadow" 0/1 run the shadow work of
 * a recursion level on its own stream, concurrent with the next level; "release_work" 1: hand the work arena back to the driver
 * now (the scene stays resident; the next render call allocates again); "light_cones" 1/0 (default 1): the light loop settles the box misses
 * of single-instance shadow groups with the per-light shadow cones built at scene creation (point lights, whole rays; same results, fewer
 * instructions); 0: every pair takes the box test; "light_hulls" 1/0 (default 1; only with light_cones on): that loop first settles the pairs
 * whose surface point lies outside the light's hull cone around the instance's mesh -- unoccluded, neither box-tested nor queued (static
 * single-instance mesh groups, point lights; same results, fewer shadow rays walked); 0: the box cones alone; "shade_first_touch" 1/0 (default 1;
 * other values are refused): the camera level of a fixed-grid batch stores each sample once -- its hit's radiance and alpha, zeros for a
 * miss -- and the batch's samples are not cleared first; 0: memset, then atomic adds and an alpha store (the same frame bit for bit; query
 * "accum_memsets": batches of the last render call that took the memset, which the adaptive sampler always does). Returns 0 or FJGPU_EINVAL. */
int fjgpu_set_option(fjgpu_scene *scene, const char *name, long value);

/* Process-wide options read by fjgpu_scene_create (which stands for the reference's
 * build_accelerators(), src/fj_scene_interface.cc:1161-1202): "device_build" -1/0/1/2 -- 0: the host's binned-SAH
 * build; 1: build the BLAS of meshes on the GPU by locally-ordered clustering (surface-area agglomeration over the
 * Morton order); 2: on the GPU as the radix tree of the Morton codes (fastest build, slowest tree); -1 (default): not
 * set -- the host build, or, for scenes created while "single_frame_build" is 1, the GPU's clustering build.
 * "blas_treelet_passes" 0..8 (default 0): scenes created from now on run that many passes of SAH treelet restructuring (7-leaf treelets,
 * the cheapest of all trees over them by dynamic programming; Karras & Aila 2013) over a GPU-built BLAS -- either builder -- before its collapse
 * to 4-wide nodes; a pass that rewrites nothing is the last.  0: the tree as the builder formed it.  The host build ignores it.  The environment
 * variable FJGPU_TREELET_PASSES, read at scene creation, wins over the option.  Closest hits do not depend on it; node counts and counters do.
 * "multi_exchange" 0/1: how fjgpu_render_frame_multi moves the devices' tile slabs to the first device -- 0 (default): one hipMemcpyPeer per
 * device (over xGMI where peer access exists; nothing to bring up, which is what a one-frame process wants); 1: RCCL -- once EVERY device has
 * rendered and packed its share, one ncclGroupStart / ncclGroupEnd holds each device's ncclSend and the first device's ncclRecv for it (the
 * exchange is collective over success: a device that failed returns its error and no rank is left waiting; librccl.so is loaded at first use;
 * devices must be distinct; a communicator that cannot be created falls back to the peer copies).  Same bytes over the same links.
 * "cold_start" 1/0 (default 1): a scene's FIRST fjgpu_render_tiles call renders in batches of 16 M samples whatever the memory would hold (a work
 * arena of ~14 GB instead of ~110 GB at 1080p / 64 spp: the first image after 0.15 s instead of the seconds the large allocation can take);
 * the second call sizes its batches by memory and pays for the growth once.  0: the first call already does.
 * "anyhit_filter_off" 0/1 (diagnostics, default 0): the lean any-hit walk's conservative f32 triangle filter decides nothing -- every leaf test goes
 * through the walk's exact phase (the reference's FP64 statements on the ray rebuilt from the queue entry).  Same image, several times the
 * walk's time: what tests use to put that phase under load.
 * "speculative_walk" 1/0 (default 1): the closest-hit walk of the next recursion level is enqueued behind a level's shading launch, before the
 * host has read how many rays that launch emitted (the walk reads the count from device memory): no host round trip between the levels.
 * "cold_batch_samples" n: ... in batches of n samples instead (0 = back to 16 M).
 * "single_frame_build" 0/1 (per calling THREAD): the caller renders ONE frame per scene it creates (SiRenderScene switches it on around its
 * scene creation; scenes created on other threads meanwhile are unaffected): the 0.4 s of host build the tree's 3-6 % faster frames would need many frames to earn back are not spent.
 * "device_tlas" 1/0 (default 1): the instance level of every group (the reference's BVHAccelerator over
 * ObjectInstances, src/fj_bvh_accelerator.cc:253-334) is built on the GPU; 0: by the host's builder (the
 * same list).  "tlas_verify" 0/1: scene creation also builds it on the host and fails on any byte that differs.
 * "ray_sort" -1..9: grid bits per axis of the ray-queue sort in front of the closest-hit walk (rays of
 * recursion level >= 1 in direction-octant / origin-cell order); 0 = off, -1 (default) = 7 bits in scenes
 * whose shaders scatter (glass, pathtracing), off elsewhere.  "ray_sort_min": launches of fewer rays keep
 * queue order (default 65536).  "split_shadow" 1/0 (default 1): in scenes served by the lean any-hit walk, a shadow
 * ray into a group of several instances is queued once per instance whose box it passes (joined by a counter)
 * instead of walking the group's instance level in the traversal kernel (C2: 134 -> 121 ms per frame).
 * "compact_squeue" 1/0 (default 1): shadow-queue records of 56 instead of 80 bytes (no direction / distance: the walk rebuilds them from the origin and
 * the light sample, same statements, same bits) where the lean or the curve any-hit walk consumes the queue and the lights are point / dome lights.
 * "flat_groups" 0/1/2 (default 1): scenes created from now on whose closest-hit rays are incoherent (glass, pathtracing shaders) and whose groups hold only
 * small static meshes built on the host (at most 2 M triangles and 32 instances per group, 80 instances in the scene: the walk keeps every instance's
 * M^-1 in LDS) get ONE world-space culling tree per group over the triangles of all its instances; the exact tests stay in object space
 * (k_trace_closest_flat).  0: the instance loop of k_trace_closest_phased.  2: scenes with coherent rays as well (an experiment switch: their walks lose
 * with it -- C2's closest-hit side 21 -> 29 ms, C3's 24 -> 104 with FJGPU_FLAT_MAX_TRIS_LOG2=25 -- profiles/r05_flat_for_coherent_scenes.txt).
 * "curve_anyhit" 1/0 (default 1): scenes created from now on that hold curve sets, no time-sampled motion and only opaque occluders walk their
 * shadow rays with k_shadow_anyhit_curves (phase-scheduled, ribbon tests as a phase of their own); 0: with the general k_shadow_trace.
 * "inst_lds" 1/0 (default 1): scenes created from now on whose instance level is small (79 threaded nodes / 33 instances /
 * 24 groups for the closest-hit and general shadow walks of mesh scenes, 39 / 16 / 12 for the phase-scheduled walk (the flat-group
 * walk keeps only M^-1 of up to 80 instances), 15 / 6 / 12 for the walks of curve scenes, 292 nodes for the light loop; one instance is a 304-byte DInstEntry) have it
 * copied to LDS by every block of those walks; 0, or a scene beyond its kernel's budget: it is read from global memory (same
 * results; option 0, or a scene of more than 80 instances, also builds no flat groups).
 * "batch_tiles" n: scenes created from now on start with the per-scene option of that name set to n (0 = sized by
 * memory; how a host that never sees the scene handle -- SiRenderScene -- cuts a frame into batches).  0 or FJGPU_EINVAL. */
int fjgpu_global_option(const char *name, long value);

/* Inspection, no device needed: the instance level of `group` as the HOST builder lays it out (the device builds
 * the same list, option "tlas_verify") -- a depth-first node list, node k: out_inst[k] = instance index or -1 for an
 * inner node, out_skip[k] = index (within this list) of the node after an inner node's subtree, out_box[6 k..] = the
 * instance's reference box / the inner node's widened union box.  The leaves are in the depth-first order of the
 * reference's BVHAccelerator over the group's instances (src/fj_bvh_accelerator.cc:253-334).  Writes at most `cap`
 * nodes (any out pointer may be NULL); returns the node count, or a negative error. */
int fjgpu_host_instance_level(const fj_scene_desc *desc, int group, int32_t *out_inst, int32_t *out_skip, double *out_box, int cap);

/* Inspection, no device needed: the per-light hull cones of single-instance `group` as scene creation builds them (fjgpu_light_hull.h): one
 * 160-byte record per light sample (six plane normals double[6][3], double reach, int32 plane count, int32 pad; count 0 = no record: the
 * group has no row, or the light none) and the light samples' positions.  Writes at most `cap` of each (either pointer may be NULL);
 * out_M (or NULL): rows 0..2 of the object-to-world matrix of the group's one instance, 12 doubles.  Returns the number of light samples, or
 * a negative error. */
int fjgpu_host_light_hulls(const fj_scene_desc *desc, int group, void *out_records, double *out_Pl, int cap, double *out_M);

/* Inspection, no device needed: the BLAS over curve set `curve_set` as scene creation builds it on the host (it reads
 * FJGPU_CURVE_SEGDEPTH like scene creation does), a read-only view.  Per BLAS slot s (one piece of one curve): out_curve[s] = the
 * curve's index in the set, out_capsule[7 s ..] = chord A xyz, chord B xyz, reach (f32, as uploaded; reach = inf with vertex
 * velocities), out_depth[s] = the cached split depth of the curve, out_box[6 s ..] = min xyz, max xyz of the leaf box the tree holds
 * for the slot (f32; a set of ONE slot has no node: the set's padded bounds).  out_grid_n[3], out_grid_cell[3], out_bounds[6]: the
 * reference grid over the set that the cell-listing rule uses and the set's padded bounds.  Writes at most `cap` slots (any out
 * pointer may be NULL); returns the slot count, or a negative error. */
int fjgpu_host_curve_blas(const fj_scene_desc *desc, int curve_set, int32_t *out_curve, float *out_capsule, int32_t *out_depth,
                          float *out_box, int cap, int32_t *out_grid_n, double *out_grid_cell, double *out_bounds);

/* Facts about the built device scene (for measurement: record sizes of the actual layout).
 * "node_record_bytes" (128; "anyhit_node_record_bytes" 64: the lean any-hit walk reads the quantised
 * twin of a node), "tri_record_bytes" (36 when every mesh is stored as exact f32
 * triangles, else 72), "blas_nodes", "stack_need", "blas_treelet_passes" / "blas_treelets_changed" (treelet passes actually run / treelets
 * rewritten in them), "blas_sah_cost_initial" / "blas_sah_cost" (SAH cost of the binary tree over its root's half area -- the leaf rule's model:
 * C(triangle) = A, C(inner) = min(trav A + C(l) + C(r), A count for count <= 4) -- as the builder formed it / after the passes; equal with 0
 * passes; all four are sums over the scene's GPU-built meshes and 0 when there is none), "lean_anyhit" (1: shadow rays are walked by
 * k_shadow_anyhit, 0: not), "curve_anyhit" (1: by k_shadow_anyhit_curves -- curve scene, every occluder opaque, no motion; both 0: by the
 * general k_shadow_trace), "closest_kernel" (0 k_trace_closest, 1 k_trace_closest_phased,
 * 2 its curve instantiation, 3 its motion instantiation, 4 k_trace_closest_flat: one world-space tree per group), "closest_node_record_bytes" (64: the closest-hit walk reads the
 * quantised nodes too; 128 in scenes with curve sets or motion), "has_curves", "has_motion", "scene_bytes" (device memory of the
 * resident scene: BLAS, instance level, lights, textures), "work_bytes" (the wavefront work arena -- queues, accumulators -- as the
 * largest call so far sized it; scene_bytes + work_bytes = the HBM this scene holds), "stack_peak" (with option count_nodes on: the most
 * entries any lane's traversal stack held in the launches of the last render_* / trace call -- "stack_peak_closest" / "stack_peak_shadow": of the
 * closest-hit / the shadow walks alone; 0 without the option), "stack_lds" / "stack_lds_anyhit" / "stack_lds_curves" / "stack_lds_min" (entries
 * the walks keep in LDS: a peak above a walk's figure went through the global overflow area), "light_cone_rows" / "light_cone_records" (single-instance
 * groups with a row in the shadow-cone table; records of those rows that hold a cone), "light_cone_verdicts" / "light_cone_contradictions" (a
 * -DFJ_LIGHT_CONE_VALIDATE build: cone verdicts of the light loop since the library was loaded, and how many the exact box test contradicted;
 * -1 in any other build), "light_hull_rows" / "light_hull_records" (the same for the hull-cone table), "light_hull_verdicts" (pairs the hull
 * cones settled in the last render call with count_nodes on, else 0; a -DFJ_LIGHT_HULL_VALIDATE build: the settled pairs queued and walked
 * all the same since the library was loaded), "light_hull_contradictions" (that build: how many of those walks found a hit; -1 in any other
 * build), "stack_lds_canyhit" (the LDS entries of k_shadow_anyhit_curves, beside the other four), "tri_filter_miss" / "tri_filter_hit" /
 * "tri_filter_maybe" / "tri_filter_exact_hits" / "tri_filter_contradictions" (a -DFJ_TRI_FILTER_VALIDATE build: the verdicts of the lean
 * any-hit walk's f32 triangle filter since the library was loaded, the hits of the exact test run behind every one of them, and the MISS / HIT
 * verdicts the exact test contradicted; reading does not reset them; -1 in any other build).  Returns 0 or FJGPU_EINVAL. */
int fjgpu_scene_query(const fjgpu_scene *scene, const char *name, double *value);

/* What this library was compiled with; needs no device and no scene.  Names: "stack_lds", "stack_lds_curves", "stack_lds_anyhit",
 * "stack_lds_canyhit", "stack_lds_min" (traversal stack entries per lane the walks keep in LDS: FJ_STACK_LDS*), "tri_filter_validate",
 * "light_cone_validate", "light_hull_validate" (1: built with -DFJ_TRI_FILTER_VALIDATE / -DFJ_LIGHT_CONE_VALIDATE / -DFJ_LIGHT_HULL_VALIDATE,
 * 0: not).  Returns 0, or FJGPU_EINVAL for an unknown name or a NULL argument. */
int fjgpu_build_config(const char *name, double *value);

/* Diagnostics: the host-side math that feeds geometry to the device (matrices,
 * RNG tables, sampler margins), exported so it can be pinned against the
 * reference's golden vectors on a machine without a GPU. */
void fjgpu_host_make_transform(int transform_order, int rotate_order, const double *trs9, double *M16, double *Minv16);
void fjgpu_host_xorshift_f01(int n, double *out);
/* the same under option "sampler_seed" = seed: seed 0 is fjgpu_host_xorshift_f01, else the first n draws of XorShift(seed) */
void fjgpu_host_xorshift_f01_seeded(unsigned seed, int n, double *out);
/* what the host writes into a tile's id under that seed (tile_id + 4096 seed; DESIGN.md 4, "Random streams") */
int32_t fjgpu_host_seeded_tile_id(unsigned seed, int32_t tile_id);
void fjgpu_host_sampler_margin(const fj_render_desc *render, int32_t *margin2);
double fjgpu_host_camera_uv_size_y(double fov);

/* Diagnostics: RCCL bring-up on one device.  fjgpu_render_frame_multi can move the devices' tile slabs with RCCL's grouped point-to-point
 * calls (global option "multi_exchange" 1); this runs the same calls -- ncclCommInitAll, ncclGroupStart, ncclSend + ncclRecv, ncclGroupEnd --
 * on a communicator of ONE rank (`device` sends n_floats to itself) and checks the data: librccl.so is loadable, its symbols bind, a
 * collective-library kernel runs.  0, or FJGPU_ENODEV with the reason. */
int fjgpu_dev_rccl_selftest(int device, int n_floats);

/* Diagnostics: the ray-queue sort on its own (fjgpu_raysort.hip: the hand-written wave64 LSD radix sort that orders the rays
 * of recursion level >= 1 in front of the closest-hit walk).  Sorts the pairs (keys[i], i) of HOST arrays on `device`,
 * stable, over the low key_bits bits (1 .. 32): keys_out ascending, perm[k] = index of the k-th pair (either may be NULL; without
 * keys_out the last pass writes the permutation only, as the product's sort does).
 * sort_ms (may be NULL): the fastest of `repeats` device-side runs, HIP events around the sort's launches alone. */
int fjgpu_dev_sort_pairs(int device, const uint32_t *keys, int n, int key_bits, uint32_t *keys_out, uint32_t *perm, int repeats, double *sort_ms);

/* Diagnostics: the BLAS walks' conservative slab tests on their own (csrc/device/fjgpu_slab32.h).  n (ray, box) pairs of HOST arrays run
 * through the statements the walks compile -- filter_rcp of the direction, slab32q_setup, slab32_shift, both slab32q_test overloads on the
 * quantised box, slab32_setup / slab32_test on the same box decoded to f32 planes -- one pair per lane.
 *   rays [n][8]: origin xyz, direction xyz, tmin, tmax;  grid [n][6]: grid origin xyz, cell xyz;  words [n][3]: (min, max) words of x, y, z
 *   out [n] records of 128 bytes (Slab32Probe): double inv[3]; float q[9] (i, l, h of x, y, z, quantised form); float f[9] (f32 form);
 *   float tnear_q, tnear_f; uint32 verdict (bit 0 slab32q_test, bit 1 its packed overload, bit 2 slab32_test); uint32 sh[3]; uint32 pad[2] */
int fjgpu_dev_slab32_batch(int device, int n, const double *rays, const double *grid, const uint32_t *words, void *out);

/* Diagnostics: k_quantize_nodes on its own: n BLAS nodes (128-byte DNode records, HOST array) onto the grid origin + q * cell;
 * out [n] 64-byte DNodeQ records. */
int fjgpu_dev_quantize_nodes(int device, int n, const void *nodes, const double *origin, const double *cell, void *out);

/* Human-readable message for the last error on this thread. */
const char *fjgpu_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FJGPU_H */
