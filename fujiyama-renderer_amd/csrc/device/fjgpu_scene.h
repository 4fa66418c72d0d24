// fjgpu_scene.h -- private to the two translation units that know what a fjgpu_scene is: fjgpu_api.hip (residency, options and queries, the
// multi-device frame, fjgpu_trace, the AOV pass, the camera) and fjgpu_frame.hip (the work arena and the wavefront frame loop).  The scene
// record, what both check a render description with, and the few pieces of a render call's set-up that the frame loop and the AOV pass share.
#ifndef FJGPU_SCENE_H
#define FJGPU_SCENE_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

#include "fjgpu.h"
#include "fjgpu_api_common.h"
#include "fjgpu_build.h"
#include "fjgpu_kernels.h"

#define FJ_LREC_BUFS 4

struct fjgpu_scene {
  int device;
  DScene S;                        // device pointers inside
  fjgpu::DeviceBuffers mem;        // scene-lifetime allocations
  double cam_fov;
  fj_camera_desc camera;           // the desc the scene was created with or last set to (fjgpu_scene_get_camera / fjgpu_scene_set_camera)
  int n_light_samples;
  // options
  long batch_tiles;
  long batch_samples = 0;          // option "batch_samples": samples per batch where batch_tiles is 0 (0: as many as the memory budget holds)
  long aov_batch_samples = 0;      // option "aov_batch_samples": samples per batch of fjgpu_render_aov (0: FJ_AOV_BATCH_SAMPLES)
  long render_calls = 0;           // fjgpu_render_tiles calls that rendered something (the first one sizes its batches for a cold start)
  long count_events;
  long light_cones = 1;            // option "light_cones" (default 1): the light loop of whole-ray launches settles box misses with the per-light shadow cones built at
                                   // scene creation (fjgpu_light_cone.h); 0: the instantiation without them, the same pairs through the box test
  int cone_rows = 0, cone_records = 0;   // queries "light_cone_rows" / "light_cone_records": groups with a row in the table, records of them with a plane
  long light_hulls = 1;            // option "light_hulls" (default 1): the cone instantiation of the light loop settles the pairs outside the light's hull cone (fjgpu_light_hull.h)
                                   // before the box is consulted: unoccluded, neither box-tested nor queued; 0: the box cones alone
  int hull_rows = 0, hull_records = 0;   // queries "light_hull_rows" / "light_hull_records"
  unsigned long long hull_verdicts = 0;  // query "light_hull_verdicts": pairs the hull cones settled in the last render call (counting frames, option count_nodes; else 0)
  long count_all_shadow;           // option "count_all_shadow" (default 1): light records of weight zero reach the light loop, which counts their shadow rays as the
                                   // reference does; it never queues them (their colour is exactly zero), so nothing walks them.  0: k_shade drops such records (other counts)
  long shade_first_touch = 1;      // option "shade_first_touch" (default 1): the camera level of a fixed-grid batch STORES its samples (ShadeParams.first_touch) and the
                                   // batch's memset of d_accum is not issued; 0: memset, then atomic adds and the alpha store, as every other level
  unsigned long long accum_memsets = 0;  // query "accum_memsets": batches of the last render call that cleared d_accum with a memset
  // queries "stack_peak" / "stack_peak_closest" / "stack_peak_shadow": the most entries any lane's traversal stack held in the launches of the
  // last render_* / trace call (counting instantiations only, option count_nodes; 0 without it)
  unsigned long long stack_peak_closest = 0, stack_peak_shadow = 0;
  // work buffers (lazily sized)
  std::unique_ptr<fjgpu::DeviceBuffers> work;
  size_t work_samples, work_rays;
  double *d_suv;
  uint32_t *d_stk = nullptr;       // (tile id, index in the tile) per sample slot: DScene.cam_tk (scenes with uid-keyed random streams), or null
  float *d_accum;
  // adaptive grid sampler (allocated on first use, in the `work` arena)
  double *d_aseen = nullptr, *d_afinal = nullptr;
  uint8_t *d_apstate = nullptr, *d_acells = nullptr;
  const void *a_owner = nullptr;
  size_t a_samples = 0, a_cell_bytes = 0;
  struct Level { DRay *rays; DPath *paths; size_t cap; uint32_t *keys; float *fc; };     // keys: sort keys of the level's rays (written by the shading kernel that emits them) or null;
                                   // fc: filter colours of refraction children, 3 floats per slot (scenes with a glass / pathtracing shader) or null
  bool has_filter_rays = false;    // some shader emits refraction children that carry a filter colour (DPath.flags bit 0)
  std::vector<Level> levels;       // ray queue per recursion level (allocated on first use)
  bool uses_sample_uid;            // some random stream or sample time of the scene is keyed by the sample's uid / index in its tile
  int max_children;                // most child rays one shading event can emit in this scene
  bool bounce_diffuse, bounce_reflect, bounce_refract;   // bounce types some shader of the scene emits
  DHit *d_hits;
  DLightRec *d_lrecs[FJ_LREC_BUFS];   // several buffers: the shadow stream consumes one while shading fills another (two are used without the overlap)
  DLightHair *d_lhair[FJ_LREC_BUFS];  // only when the scene has a HairShader
  int lrec_bufs = 2;                  // buffers allocated: 2, or FJ_LREC_BUFS once the overlap option is on
  long overlap;                    // option "overlap_shadow": 0 off, 1 on, 2 by the batch size
  bool overlap_now = false;        // ... what this render call does
  size_t free_cached = 0;          // free HBM + this scene's own work arena, as of the last query
  hipEvent_t ev_frame[2] = {nullptr, nullptr};   // frame start / end
  long early_shadow = 0;           // FJGPU_EARLY_SHADOW = k > 0 (only where the light loops run on their own stream: small batches, a rank's share of a frame): the shadow
                                   // queue is flushed after level k - 1's light loops, so that the one big any-hit walk runs BESIDE the deeper levels' closest-hit walks
                                   // instead of after them.  Round 6, a rank's share: C3 0 / 1 / 2 / 3 -> 18.7 / 18.1-18.6 / 18.3 / 18.5 ms, C6 +0.3, arealights +0.3, C2
                                   // 14.0 -> 15.1 with 1; switched on for single-instance shadow groups only, the SLOWEST of C3's eight shares went 17.95 -> 19.2 ms: off.
  hipStream_t shadow_stream;       // light loop + shadow traversal run here, overlapping the next level's closest-hit work
  hipStream_t read_stream = nullptr;   // the counters of a shading launch come back on this one while the main stream already runs the next level's walk
  hipEvent_t ev_shaded = nullptr;
  hipEvent_t ev_shadow_done[FJ_LREC_BUFS];    // shadow work reading d_lrecs[k] has finished
  std::vector<hipEvent_t> ev_pool; // per-launch timing events (resolved at the end of the frame: no host sync per launch)
  DShadowRay *d_squeue;
  size_t squeue_rec_bytes = 0;       // bytes per entry the queue was allocated for (DShadowRayC or DShadowRay)
  size_t squeue_cap;
  uint32_t *d_join = nullptr; size_t join_cap = 0;   // DScene.shadow_join (work arena)
  bool split_overflowed = false;   // the last render call overflowed a queue while rays were split
  uint32_t split_kfac = 1;         // queue entries the host allows per (light record, light) pair when rays are split
  bool split_shadow = false;       // the lean any-hit walk serves shadow groups of several instances: rays are queued per candidate instance
  DCounters *d_cnt;
  TileDesc *d_tiles;
  double *d_jit, *d_tim;
  size_t tab_len;
  long sampler_seed = 0;           // option "sampler_seed" (0..65535, default 0: the streams of the reference): the jitter / time tables are those of
                                   // XorShiftTableSeeded and TileDesc.id is SeededTileId of it, in every entry that draws ("Random streams")
  long tab_seed = 0;               // the seed d_jit / d_tim were built with
  int tiles_cap;
  int stack_need;
  double tri_record_bytes;         // 36 when every mesh is stored as f32 triangles, else 72
  size_t blas_nodes;
  // SAH treelet restructuring (fjgpu_lbvh.hip), summed over the device-built meshes of the scene
  long blas_treelet_passes = 0;
  unsigned long long blas_treelets_changed = 0;
  double blas_sah_cost_initial = 0., blas_sah_cost = 0.;
  size_t squeue_max;               // shadow-queue entries allowed by the memory budget
  size_t batch_fit_samples = 0;    // 0, or the samples per batch the work buffers were cut down to when an allocation failed (not tried beyond again)
  // ray-queue sort (fjgpu_raysort.hip): levels >= 1 of scenes with incoherent secondary rays
  int ray_sort_bits = 0;           // grid bits per axis; 0 = rays are walked in queue order
  double scene_box[6];             // union of the instances' world boxes (the sort's grid)
  uint32_t *d_sort[4] = {nullptr, nullptr, nullptr, nullptr};   // -, keys_alt, -, perm (in the `work` arena)
  void *d_sort_tmp = nullptr; size_t sort_tmp_bytes = 0; size_t sort_cap = 0;
  // frame-level buffers of fjgpu_render_frame_multi (lazily sized, freed with the scene)
  float *d_frame = nullptr; size_t d_frame_n = 0;      // this device's framebuffer
  float *d_slab = nullptr; size_t d_slab_n = 0;        // packed tiles: own ones (sender) / incoming (first device)
  int32_t *d_rects = nullptr; size_t d_rects_n = 0;    // tile rectangles of a slab
  fjgpu_batch_fn batch_fn = nullptr; void *batch_user = nullptr;   // fjgpu_set_batch_callback
};

// Option "overlap_shadow" (0 off, 1 on, 2 = by the size of the batch, the default): the light loops on a stream of their own, concurrent
// with the NEXT recursion levels' closest-hit walks, and with only FJ_OVERLAP_CULL_BLOCKS resident blocks per CU so that they leave the
// walks room.  It pays where the launches are small -- a rank's share of an 8-GPU frame, a small frame: the closest-hit walks of the deeper
// levels are then a few long rays each (a launch per level: 0.7 ms of dependent fetches and nothing else, profiles/r04_wave_timeline_*.txt),
// and the light loops' VALU work fits underneath: a rank's share of C3 20.9 -> 19.7 ms (profiles/r04_overlap_small_launches.txt).  A whole
// 1080p frame on one GPU loses with it (123 -> 136 ms: its walks fill the chip for most of their time), so "by size" turns it on below
// FJ_OVERLAP_MAX_SAMPLES samples per batch, for scenes whose shaders bounce.  (Round 1-3 kept it off: with the light loop at full
// occupancy the two streams only took turns.  Walking level 0's shadow rays early, under the deeper levels, was measured too
// (FJGPU_EARLY_SHADOW): the persistent walk fills every slot and the shading kernels of the deeper levels wait behind it: 20.3 ms.)
#ifndef FJ_OVERLAP_MAX_SAMPLES
#define FJ_OVERLAP_MAX_SAMPLES ((size_t) 24 << 20)    // (a quarter of a 1080p, 64 spp frame still loses with it: 35.5 -> 36.1 ms; an eighth gains)
#endif
#ifndef FJ_OVERLAP_CULL_BLOCKS
#define FJ_OVERLAP_CULL_BLOCKS 1
#endif
inline int enable_overlap(fjgpu_scene *sc)
{
  if (sc->shadow_stream) return 0;
  // (FJGPU_OVERLAP_PRIO: the stream gets the LOWEST priority, so that its blocks only take the slots the main stream's kernels leave)
  int prio_lo = 0, prio_hi = 0;
  if (getenv("FJGPU_OVERLAP_PRIO") && hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) == hipSuccess && prio_lo != prio_hi) {
    if (hipStreamCreateWithPriority(&sc->shadow_stream, hipStreamNonBlocking, prio_lo) != hipSuccess) { sc->shadow_stream = nullptr; return -1; }
  }
  else if (hipStreamCreateWithFlags(&sc->shadow_stream, hipStreamNonBlocking) != hipSuccess) { sc->shadow_stream = nullptr; return -1; }
  for (int k = 0; k < FJ_LREC_BUFS; k++)
    if (hipEventCreateWithFlags(&sc->ev_shadow_done[k], hipEventDisableTiming) != hipSuccess) return -1;
  return 0;
}

// A render description the tiler can work on: positive sizes and a region inside the frame.
// The reference only asserts region min < max (src/fj_tiler.cc:75-76) and would write outside
// its framebuffer for a region past the frame; this is a public C ABI, so it is refused.
inline const char *bad_tiling(const fj_render_desc *r)
{
  if (r->xres <= 0 || r->yres <= 0 || r->tile_w <= 0 || r->tile_h <= 0)
    return "bad render settings: resolution and tilesize must be positive";
  if (r->region[0] < 0 || r->region[1] < 0 || r->region[2] > r->xres || r->region[3] > r->yres ||
      r->region[0] >= r->region[2] || r->region[1] >= r->region[3])
    return "bad render settings: render_region must be a non-empty rectangle inside the frame";
  return nullptr;
}
inline const char *bad_render(const fj_render_desc *r)
{
  if (const char *why = bad_tiling(r)) return why;
  if (r->rate_x <= 0 || r->rate_y <= 0) return "bad render settings: pixelsamples must be positive";
  return nullptr;
}

// the process-wide options (fjgpu_global_option) the frame loop reads; defined in fjgpu_api.hip beside that function, where each is described
namespace fjgpu {
extern long g_spec_walk, g_ray_sort_min, g_cold_start, g_cold_batch_samples, g_compact_squeue;

// the work arena of a scene is gone or about to go: nothing of the scene points into it any more (fjgpu_frame.hip)
void ForgetWorkArena(fjgpu_scene *sc);
}  // namespace fjgpu

// ---- what the frame loop, the multi-device frame and the AOV pass set up alike

// the tiles of a call: the caller's list, or every tile of the render region; an id outside the tiling is refused
inline int listed_tiles(const int32_t *tile_ids, int n_tiles, size_t n_all, std::vector<int32_t> *ids)
{
  if (tile_ids) ids->assign(tile_ids, tile_ids + std::max(0, n_tiles));
  else for (size_t i = 0; i < n_all; i++) ids->push_back((int32_t) i);
  for (int32_t id : *ids) if (id < 0 || id >= (int32_t) n_all) return fjgpu::fail(FJGPU_EINVAL, "tile id out of range");
  return 0;
}

// the fixed-grid sampler's parameters of a render description
inline GenParams gen_params(const fj_render_desc *r, const int *margin)
{
  GenParams gp;
  gp.rate_x = r->rate_x; gp.rate_y = r->rate_y; gp.margin_x = margin[0]; gp.margin_y = margin[1];
  gp.udelta = 1. / (r->rate_x * r->xres);
  gp.vdelta = 1. / (r->rate_y * r->yres);
  gp.jitter = r->jitter;
  gp.jittered = r->jitter > 0 ? 1 : 0;
  gp.pad = 0;
  return gp;
}

// camera (Renderer::preprocess_camera + Camera::compute_uv_size)
inline void camera_uv_size(double fov, const fj_render_desc *r, double uv_size[2])
{
  const double aspect = r->xres / (double) r->yres;
  uv_size[1] = fjgpu::CameraUvSizeY(fov);
  uv_size[0] = uv_size[1] * aspect;
}

// a tile of the fixed-grid sampler: rate x rate samples per pixel plus the filter margin
inline TileDesc fixed_grid_tile(const fjgpu_scene *sc, const fj_render_desc *r, const fjgpu::TileRect &t, const int *margin, uint32_t sample_offset)
{
  TileDesc d;
  d.xmin = t.xmin; d.ymin = t.ymin; d.xmax = t.xmax; d.ymax = t.ymax; d.id = fjgpu::SeededTileId(t.id, (unsigned) sc->sampler_seed);
  d.nx = r->rate_x * (t.xmax - t.xmin) + 2 * margin[0];
  d.ny = r->rate_y * (t.ymax - t.ymin) + 2 * margin[1];
  d.sample_offset = sample_offset; d.cell_offset = 0; d.pad = 0;
  return d;
}

#endif
