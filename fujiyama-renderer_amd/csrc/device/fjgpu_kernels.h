// fjgpu_kernels.h -- launch parameters and host launchers of fjgpu_kernels.hip
#ifndef FJGPU_KERNELS_H
#define FJGPU_KERNELS_H

#include <hip/hip_runtime.h>
#include "fjgpu_types.h"

struct TileDesc {              // one tile of the current batch
  int32_t xmin, ymin, xmax, ymax;
  int32_t nx, ny;              // samples incl. filter margin: rate * size + 2 * margin
  uint32_t sample_offset;      // first sample slot of this tile in the batch arrays
  int32_t id;
  uint32_t cell_offset;        // adaptive sampler: first level-0 lattice cell of this tile in the batch
  int32_t pad;
};

struct GenParams {
  int32_t rate_x, rate_y, margin_x, margin_y;
  double udelta, vdelta, jitter;
  int32_t jittered, pad;
};

struct AovParams {             // fjgpu_render_aov: the reduce kernel's view of the call (fjgpu_dev_aov.h)
  int32_t xres, rate_x, rate_y, margin_x, margin_y, pad;
  float *depth, *position, *normal, *uv;     // DEVICE buffers of the frame, row-major; null = not wanted (fjgpu_aov_buffers)
  int32_t *ids;
  float *coverage;
};

struct AlbedoParams {          // fjgpu_render_aov_albedo: the albedo kernel's view of the call (fjgpu_dev_albedo.h)
  int32_t xres, rate_x, rate_y, margin_x, margin_y;
  int32_t lanes, lanes_log2, pad;   // lanes per pixel: the smallest power of two >= min(rate_x * rate_y, 64)
  float *albedo;               // DEVICE [yres][xres][3]
};

struct AdaptiveParams {       // AdaptiveGridSampler, src/fj_adaptive_grid_sampler.cc
  int32_t D, div;              // adaptive_max_subdivision, 2^D lattice cells per pixel
  int32_t margin_x, margin_y;  // filter margin in PIXELS: ceil(filterwidth - 1)
  double udelta, vdelta, jitter, threshold;
  int32_t jittered, level;
  uint32_t cells0;             // level-0 lattice cells of the whole batch
  uint32_t ray_capacity;
};

struct ShadeParams {
  int32_t max_diffuse_depth, max_reflect_depth, max_refract_depth;
  int32_t count_all_shadow;    // 1: zero-weight light records go to the light loop too, so that their shadow rays are COUNTED (reference ray counts);
                               // they are never queued or traced (k_shadow_cull: a pair whose colour is exactly zero)
  uint32_t ray_capacity, light_capacity;
  // ray-queue sort (fjgpu_raysort.hip): the key of a child ray is computed where the ray is emitted -- origin and direction
  // are in registers there -- instead of by a pass of its own over the queue (C4: 1.6 G rays x 48 B less read per frame)
  uint32_t *next_keys;         // key of the child in slot k of the next queue, or null (no sort in this scene / for this level)
  // filter colour of refraction children (DPath.flags bit 0), 3 floats per queue slot: of the rays being shaded / of the children emitted; null in
  // scenes without a glass or pathtracing shader (no ray ever sets the bit there)
  const float *fc_in;
  float *fc_out;
  double sort_lo[3], sort_scale[3];
  int32_t sort_bits;
  // 1: a camera level whose entry i is sample DScene.cam_slot0 + i, and nothing has added to the batch's samples yet: every entry STORES its sample
  // (radiance and alpha of its hit, zeros for a miss) instead of adding to a cleared one, and the batch's memset is not issued
  int32_t first_touch;
};

struct ShadowParams {
  double cos_half_pi, cos_pi;  // cos(PI/2.), cos(PI) evaluated by the host libm
  uint32_t pre_resolve;        // 1: queue entries of single-instance groups carry ~instance (lean any-hit walk)
  uint32_t queue_capacity;     // entries of the shadow-ray queue
  uint32_t join_capacity;      // slots of DScene.shadow_join (0: shadow rays into groups of several instances stay whole)
  int32_t cast_shadow;
  int32_t compact;             // 1: the queue holds DShadowRayC records (DScene.compact_squeue)
  int32_t light_cones;         // 1: whole-ray launches of scenes with a cone table (DScene.light_cones) settle box misses with the per-light cones
                               // (scene option "light_cones", default 1); 0: the instantiation without them
  int32_t light_hulls;         // 1: ... and, before the box is consulted, the pairs outside the light's hull cone (DScene.light_hulls; scene option
                               // "light_hulls", default 1; only with light_cones: the hulls live in the cone instantiation)
  int32_t pad_;
};

struct ResolveParams {
  int32_t xres, yres, rate_x, rate_y, npx_x, npx_y;
  double fw, fh;
};

int launch_gen_camera(hipStream_t st, const DScene &S, const GenParams &gp, const TileDesc *d_tiles, int n_tiles,
    uint32_t max_tile_samples, const double *jit, const double *tim, double *s_uv, DRay *rays, DPath *paths, uint32_t *s_tk = nullptr);
int launch_trace_closest(hipStream_t st, const DScene &S, const DRay *rays, const DPath *paths, DHit *hits,
    uint32_t n, DCounters *cnt, int count_events);
int launch_shade(hipStream_t st, const DScene &S, const ShadeParams &sp, const DRay *rays, const DPath *paths,
    const DHit *hits, uint32_t n, float *s_accum, DRay *next_rays, DPath *next_paths, DLightRec *lrecs, DCounters *cnt);
uint32_t shadow_queue_padding();
void shadow_queue_reset(hipStream_t st, DCounters *cnt);
int launch_shadow_cull(hipStream_t st, const DScene &S, const ShadowParams &sp, const DLightRec *lrecs, uint32_t b, uint32_t e,
    float *s_accum, DShadowRay *squeue, DCounters *cnt, int count_events, int blocks_per_cu = 0);      // (0: what fits)
int launch_shadow_trace(hipStream_t st, const DScene &S, const DShadowRay *squeue, float *s_accum, DCounters *cnt, int count_events);
// the quantised node array of the lean any-hit walk from the f32 one (same indices)
int launch_quantize_nodes(hipStream_t st, const DNode *nodes, uint32_t n, const double *origin, const double *cell, DNodeQ *out);
// diagnostics: n (ray, box) pairs through the walks' slab-test statements, one 128-byte Slab32Probe record each (fjgpu_slab32.h)
int launch_slab32_batch(hipStream_t st, uint32_t n, const double *rays, const double *grid, const uint32_t *words, void *out);
// multi-GPU frame: pack a device's tiles (d_rects [n][4] = xmin ymin xmax ymax) into a slab of
// tile_px pixels per tile, or scatter such a slab into the framebuffer (unpack)
int launch_move_tiles(hipStream_t st, bool unpack, float *fb, int xres, const int32_t *d_rects, int n_tiles, int tile_px, float *slab);
void set_anyhit_filter_off(long v);     // diagnostics: fjgpu_global_option("anyhit_filter_off")
// -DFJ_LIGHT_CONE_VALIDATE builds: the cone verdicts of the light loop so far (current device) and how many of them the exact test contradicted;
// other builds: -1, -1
void light_cone_validate_counts(double *verdicts, double *contradictions);
// -DFJ_LIGHT_HULL_VALIDATE builds: the hull-settled pairs the any-hit walks have walked so far and how many of those walks found a hit; other builds: -1, -1
void light_hull_validate_counts(double *verdicts, double *contradictions);
// -DFJ_TRI_FILTER_VALIDATE builds: the filter's verdicts in the lean any-hit walk so far (current device) -- miss, hit, maybe --, the exact test's hits and
// the verdicts it contradicted, in that order; other builds: -1 five times.  Reads only (debug_phase_stats prints and resets them).
void tri_filter_validate_counts(double out[5]);
// the constants THIS file's kernels were compiled with (fjgpu_build_config's names); false: no such name.  No device call.
bool kernels_build_config(const char *name, double *value);
void debug_phase_stats();     // FJ_PHASE_STATS builds: print and reset the any-hit walk's phase tallies (stderr)
// threads of the largest persistent grid (sizes per-thread scratch such as the stack overflow area)
size_t persistent_threads();

// sample values: f32 RGBA as accumulated (fixed grid) or f64 RGBA (adaptive grid: interpolated samples)
int launch_resolve(hipStream_t st, const ResolveParams &rp, const TileDesc *d_tiles, int n_tiles, int max_tile_pixels,
    const double *s_uv, const float *s_accum, const double *s_data64, float *fb);

// first-hit AOV pass (fjgpu_dev_aov.h): the own samples of every pixel of the batch's tiles reduced to the nearest hit, its attributes written out
int launch_aov_reduce(hipStream_t st, const DScene &S, const AovParams &ap, const TileDesc *d_tiles, int n_tiles, int max_tile_pixels,
    const DRay *rays, const DHit *hits);

// albedo AOV (fjgpu_dev_albedo.h): the mean surface colour of every pixel's own samples, from the hit records of the batch k_aov_reduce read
int launch_aov_albedo(hipStream_t st, const DScene &S, const AlbedoParams &ap, const TileDesc *d_tiles, int n_tiles, int max_tile_pixels,
    const DHit *hits);

// adaptive grid sampler (fjgpu_dev_adaptive.h)
int launch_adaptive_uv(hipStream_t st, const AdaptiveParams &ap, const TileDesc *d_tiles, int n_tiles, uint32_t max_tile_samples,
    const double *jit, double *s_uv);
int launch_adaptive_points(hipStream_t st, const DScene &S, const AdaptiveParams &ap, const TileDesc *d_tiles, int n_tiles,
    uint32_t max_tile_points, const uint8_t *cells, const double *s_uv, const float *s_accum, uint8_t *pstate, double *seen,
    DRay *rays, DPath *paths, DCounters *cnt);
int launch_adaptive_decide(hipStream_t st, const AdaptiveParams &ap, const TileDesc *d_tiles, int n_tiles, uint32_t max_tile_cells,
    uint8_t *cells, const float *s_accum, const uint8_t *pstate, const double *seen);
int launch_adaptive_fill(hipStream_t st, const AdaptiveParams &ap, const TileDesc *d_tiles, int n_tiles, uint32_t max_tile_samples,
    const uint8_t *cells, const float *s_accum, const uint8_t *pstate, const double *seen, double *final_data);

#endif
