// fjgpu_frame.hip -- C ABI of libfjgpu.so (include/fjgpu.h), the beauty pass: fjgpu_render_tiles and fjgpu_render_tiles_variance, the work
// arena of a scene and the wavefront frame loop behind them.  render_tiles_once reads top to bottom: plan, reserve, launch parameters,
// batches (BatchRun), totals.  (the scene record and what is shared with the other entry points on a scene: fjgpu_scene.h)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fjgpu.h"
#include "fjgpu_api_common.h"
#include "fjgpu_build.h"
#include "fjgpu_kernels.h"
#include "fjgpu_raysort.h"
#include "fjgpu_sample_variance.h"
#include "fjgpu_scene.h"

using fjgpu::fail;
using fjgpu::DeviceBuffers;

// ---- the work arena

void fjgpu::ForgetWorkArena(fjgpu_scene *sc)
{
  sc->work.reset();
  sc->work_samples = sc->work_rays = 0; sc->tiles_cap = 0; sc->lrec_bufs = std::min(sc->lrec_bufs, 2); sc->squeue_rec_bytes = 0;
  // the adaptive sampler's buffers lived in the old arena (a new arena may be allocated at the
  // old one's address, so the owner pointer alone does not tell)
  sc->sort_cap = 0; sc->a_owner = nullptr; sc->a_samples = 0; sc->a_cell_bytes = 0;
  sc->d_aseen = sc->d_afinal = nullptr; sc->d_apstate = sc->d_acells = nullptr;
  for (auto &L : sc->levels) { L.rays = nullptr; L.paths = nullptr; L.cap = 0; L.keys = nullptr; }
}

namespace {

// compact queue records (DShadowRayC, 56 bytes) where the consumers rebuild direction and distance: the lean and the curve any-hit walk,
// point / dome lights, no motion
bool scene_compact_squeue(const DScene &S)
{
  const bool lean = S.all_opaque && !S.has_curves && !S.has_motion && S.blas_base;
  const bool curve_walk = S.has_curves && !S.has_motion && S.all_opaque && S.curve_anyhit && S.inst_lds && S.n_group_nodes <= FJ_INST_LDS_NODES_CURVES &&
      S.n_instances <= FJ_INST_LDS_INSTS_CURVES && S.n_groups <= FJ_INST_LDS_GROUPS_CURVES && FJ_CURVE_QNODES && FJ_CLOSEST_QNODES;
  return (lean || curve_walk) && !S.has_area && fjgpu::g_compact_squeue && !getenv("FJGPU_NO_COMPACT_SQUEUE");
}

// IMPLICIT CAMERA RAYS (fjgpu_dev_shade.h): level 0 is rebuilt from the (u, v) table where it is needed, and nothing reads the level's 112
// bytes per sample -- 15 GB of a cold C3 frame's allocations -- so the level is not allocated.  Scenes whose random streams are keyed by the
// sample's uid -- pathtracing shader, area lights -- get a (tile, index) table of 8 bytes per sample beside the (u, v) table, d_stk;
// time-sampled motion keeps explicit rays: the walks read the sample's time from the path record.
// ONE rule for the allocation and for the batches.  It used to be written twice, as "!uses_sample_uid || !has_motion" where the levels are
// allocated and as "!uses_sample_uid || (uses_sample_uid && !has_motion && d_stk)" in the batch.  They agree: both also ask for no camera
// transform, ensure_work allocates d_stk exactly when uses_sample_uid && !has_motion && !cam_xform (all three fixed at scene creation, and
// a failed allocation ends the call), so without a camera transform "d_stk exists" says "uses_sample_uid && !has_motion" and the second
// spelling reduces to the first.
bool implicit_camera_rays(const fjgpu_scene *sc, bool adaptive)
{
  return !adaptive && sc->S.cam_xform == nullptr && (!sc->uses_sample_uid || !sc->S.has_motion) && !getenv("FJGPU_EXPLICIT_CAMERA_RAYS");
}

int ensure_work(fjgpu_scene *sc, size_t samples, size_t rays, int tiles, size_t tab_len)
{
  const int want_bufs = sc->overlap_now ? FJ_LREC_BUFS : 2;
  // the shadow queue is allocated at the record size the scene's walks read (56 or 80 bytes: 12 GB apart at the headline size); a scene
  // that goes back to the long record (option compact_squeue switched off between calls) gets a new arena
  const size_t rec_bytes = scene_compact_squeue(sc->S) ? sizeof(DShadowRayC) : sizeof(DShadowRay);
  if (samples > sc->work_samples || rays > sc->work_rays || tiles > sc->tiles_cap || want_bufs > sc->lrec_bufs || rec_bytes > sc->squeue_rec_bytes) {
    // the arena only GROWS: a reallocation for one reason (a small batch that wants the overlap's extra light-record buffers after a
    // whole frame, a longer tile list) keeps every other dimension at the largest size seen, or callers that alternate whole frames
    // with region / rank-share renders would free and reallocate tens of GB on every call
    samples = std::max(samples, sc->work_samples); rays = std::max(rays, sc->work_rays); tiles = std::max(tiles, sc->tiles_cap);
    const int old_bufs = sc->lrec_bufs;
    // (the extra light-record buffers of the overlap mode belong to SMALL batches: an arena that grows to a larger batch -- the second call after
    // a cold start -- takes what that batch wants, 2 x 80 B per ray, not the 4 the small one had: 21 GB at the headline size)
    const int new_bufs = samples > sc->work_samples ? want_bufs : std::max(sc->lrec_bufs, want_bufs);
    fjgpu::ForgetWorkArena(sc);
    sc->lrec_bufs = new_bufs;
    sc->work.reset(new DeviceBuffers());
    DeviceBuffers &W = *sc->work;
    int e = 0;
    e |= W.alloc(samples * 2, &sc->d_suv);
    sc->d_stk = nullptr;
    if (sc->uses_sample_uid && !sc->S.has_motion && !sc->S.cam_xform) e |= W.alloc(samples * 2, &sc->d_stk);      // (tile, index) per sample: implicit camera rays
    e |= W.alloc(samples * 4, &sc->d_accum);
    e |= W.alloc(rays, &sc->d_hits);
    for (int k = 0; k < sc->lrec_bufs; k++) {
      e |= W.alloc(rays, &sc->d_lrecs[k]);
      sc->d_lhair[k] = nullptr;
      if (sc->S.has_hair) e |= W.alloc(rays, &sc->d_lhair[k]);
    }
    // (rays queued once per candidate instance: room for twice the entries, or the light loop runs in many short launches)
    // (sized for the light loop's WORST case -- every (record, light) pair survives the cull -- where the memory is there: the bound decides
    // into how many launches the light loop of a level is cut, and each cut is a host round trip: a rank's share of C3 took three)
    const size_t per_ray = std::max<size_t>(sc->split_shadow ? 16 : 8, std::min<size_t>(64, (size_t) std::max(1, sc->n_light_samples) * (sc->split_shadow ? 2 : 1)));
    // (from the batch's own samples, not from the 8 M-entry floor small frames get for their RAY queues: a 64 x 64 render under a dome
    // light of 64 samples allocated 40 GB here -- ADVICE round 4.  The bound only decides into how many launches the shadow walk is cut.)
    const size_t lrec_bound = std::min<size_t>(rays, std::max<size_t>(samples * 4, (size_t) 1 << 16));
    sc->squeue_cap = std::min<size_t>(lrec_bound * per_ray, sc->squeue_max) + 4096 * 1024;   // + one chunk per resident wave
    { char *q = nullptr; e |= W.alloc(sc->squeue_cap * rec_bytes, &q); sc->d_squeue = (DShadowRay *) q; sc->squeue_rec_bytes = e ? 0 : rec_bytes; }
    // join slots of shadow rays queued once per candidate instance (DScene.shadow_join): a ray that has one
    // owns at least two queue entries
    sc->d_join = nullptr; sc->join_cap = 0;
    // (a slot per ray with >= 2 entries -- at most squeue_cap / 2 of them -- but the light loop's waves reserve slots JQ_CHUNK = 64 at a
    // time and a chunk roll-over discards up to 63 of them, i.e. up to about half of what is reserved over a launch: sized for that
    // worst case plus one chunk per resident wave and launch; 4 bytes per slot.  Beyond it the join area overflows like the queue
    // does and the frame is rendered again without the split)
    if (sc->split_shadow) { sc->join_cap = sc->squeue_cap + 1 + 32 * (persistent_threads() / 64) * 64; e |= W.alloc(sc->join_cap, &sc->d_join); }
    e |= W.alloc(1, &sc->d_cnt);
    e |= W.alloc((size_t) tiles, &sc->d_tiles);
    if (e) { sc->lrec_bufs = old_bufs; fjgpu::ForgetWorkArena(sc); return -1; }
    sc->work_samples = samples; sc->work_rays = rays; sc->tiles_cap = tiles;
  }
  if (tab_len > sc->tab_len) {
    // the tables live with the scene (small): 3 draws per sample of the largest tile
    std::vector<double> draws;
    fjgpu::XorShiftTableSeeded((unsigned) sc->sampler_seed, 2 * tab_len, &draws);
    if (sc->mem.upload(draws.data(), 2 * tab_len, const_cast<const double **>(&sc->d_jit))) return -1;
    if (sc->mem.upload(draws.data(), tab_len, const_cast<const double **>(&sc->d_tim))) return -1;
    sc->tab_len = tab_len;
    sc->tab_seed = sc->sampler_seed;
  } else if (sc->tab_seed != sc->sampler_seed) {
    // another seed, the same length: the draws go into the tables that are there (no call is in flight: every render call ends synchronised)
    std::vector<double> draws;
    fjgpu::XorShiftTableSeeded((unsigned) sc->sampler_seed, 2 * sc->tab_len, &draws);
    if (hipMemcpy(sc->d_jit, draws.data(), sizeof(double) * 2 * sc->tab_len, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (hipMemcpy(sc->d_tim, draws.data(), sizeof(double) * sc->tab_len, hipMemcpyHostToDevice) != hipSuccess) return -1;
    sc->tab_seed = sc->sampler_seed;
  }
  return 0;
}

// AdaptiveGridSampler buffers: per sample the value its users see when it holds an earlier
// leaf's interpolation, the final (filtered) value, a state byte; per lattice cell a verdict
int ensure_adaptive(fjgpu_scene *sc, size_t samples, size_t cell_bytes)
{
  // (the work buffers were just sized by ensure_work: these live in the same arena, which is
  // replaced as a whole when it grows)
  if (sc->a_owner == sc->work.get() && samples <= sc->a_samples && cell_bytes <= sc->a_cell_bytes) return 0;
  DeviceBuffers &W = *sc->work;
  if (W.alloc(samples * 4, &sc->d_aseen) || W.alloc(samples * 4, &sc->d_afinal) || W.alloc(samples, &sc->d_apstate) ||
      W.alloc(cell_bytes, &sc->d_acells)) { sc->a_owner = nullptr; return -1; }
  sc->a_owner = sc->work.get(); sc->a_samples = samples; sc->a_cell_bytes = cell_bytes;
  return 0;
}

int ensure_level(fjgpu_scene *sc, int level, size_t cap)
{
  fjgpu_scene::Level &L = sc->levels[level];
  if (L.cap >= cap) return 0;
  DeviceBuffers &W = *sc->work;
  if (W.alloc(cap, &L.rays) || W.alloc(cap, &L.paths)) return -1;   // older, smaller buffers stay owned by `work`
  L.keys = nullptr;
  L.fc = nullptr;
  if (sc->has_filter_rays && level >= 1 && W.alloc(cap * 3, &L.fc)) return -1;
  if (sc->ray_sort_bits > 0 && level >= 1 && W.alloc(cap, &L.keys)) return -1;
  L.cap = cap;
  return 0;
}

// scratch of the ray-queue sort for up to `cap` rays (lives in the work arena like the queues)
int ensure_sort(fjgpu_scene *sc, size_t cap)
{
  if (sc->sort_cap >= cap) return 0;
  DeviceBuffers &W = *sc->work;
  sc->d_sort[0] = sc->d_sort[2] = nullptr;       // (keys come from the shading kernel; the values are the indices, implicit in the first pass)
  if (W.alloc(cap, &sc->d_sort[1]) || W.alloc(cap, &sc->d_sort[3])) return -1;
  sc->sort_tmp_bytes = ray_sort_temp_bytes((uint32_t) cap, sc->ray_sort_bits);
  char *tmp = nullptr;
  if (W.alloc(sc->sort_tmp_bytes, &tmp)) return -1;
  sc->d_sort_tmp = tmp;
  sc->sort_cap = cap;
  return 0;
}

// ---- stage 1, the plan: what the call renders and in batches of how many tiles.  Host arithmetic only.

// fjgpu_render_tiles_variance's part of a call: where the variance of the listed tiles' pixels goes and, optionally, the albedo it is taken under
struct SampleVarianceOut { float *variance; const float *albedo; float albedo_floor; };

struct FramePlan {
  bool adaptive;                         // Renderer::SetSamplerType, src/fj_renderer.cc:487-499
  std::vector<fjgpu::TileRect> all;      // the tiling of the render region
  std::vector<int32_t> ids;              // the tiles of this call, in the caller's order
  int margin[2];
  int a_div;                             // lattice cells per pixel and axis (adaptive sampler), else 1
  size_t full_tile_samples;
  int deepest;                           // the deepest recursion level this scene can reach under the depth limits
  bool implicit_cam, tk_cam;             // implicit_camera_rays(); ... with the (tile, index) table d_stk beside the (u, v) table
  long bt;                               // tiles per batch
};

int check_request(const fj_render_desc *r)
{
  const bool adaptive = r->sampler_type == 1;
  if (r->sampler_type != 0 && !adaptive) return fail(FJGPU_EINVAL, "unknown sampler_type");
  if (adaptive && (r->adaptive_max_subdivision < 0 || r->adaptive_max_subdivision > 8 || !(r->adaptive_subdivision_threshold >= 0)))
    return fail(FJGPU_EINVAL, "adaptive_max_subdivision must be in [0, 8] and adaptive_subdivision_threshold >= 0");
  if (const char *why = bad_render(r)) return fail(FJGPU_EINVAL, why);
  return 0;
}

int plan_tiles(const fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles, FramePlan *P)
{
  P->adaptive = r->sampler_type == 1;
  fjgpu::GenerateTiles(*r, &P->all);
  if (const int e = listed_tiles(tile_ids, n_tiles, P->all.size(), &P->ids)) return e;

  // samples of a tile: rate x rate per pixel plus the filter margin (fixed grid), or the
  // corners of a lattice of 2^max_subdivision cells per pixel, margin in whole pixels (adaptive
  // grid: count_samples_in_region / count_samples_in_margin, src/fj_adaptive_grid_sampler.cc:195-216)
  int *margin = P->margin;
  fjgpu::SamplerMargin(*r, margin);
  P->a_div = P->adaptive ? 1 << r->adaptive_max_subdivision : 1;
  if (P->adaptive) {
    margin[0] = (int) std::ceil((double) r->filter_w - 1);
    margin[1] = (int) std::ceil((double) r->filter_h - 1);
  }
  P->full_tile_samples = P->adaptive
      ? (size_t) (P->a_div * (r->tile_w + 2 * margin[0]) + 1) * (size_t) (P->a_div * (r->tile_h + 2 * margin[1]) + 1)
      : (size_t) (r->rate_x * r->tile_w + 2 * margin[0]) * (r->rate_y * r->tile_h + 2 * margin[1]);
  // recursion levels this scene can reach: one queue per level, level = bounces so far, and a
  // bounce type only occurs if some shader of the scene emits it
  P->deepest = (sc->bounce_diffuse ? std::max(0, r->max_diffuse_depth) : 0) +
      (sc->bounce_reflect ? std::max(0, r->max_reflect_depth) : 0) + (sc->bounce_refract ? std::max(0, r->max_refract_depth) : 0);
  P->implicit_cam = implicit_camera_rays(sc, P->adaptive);
  P->tk_cam = P->implicit_cam && sc->uses_sample_uid;
  return 0;
}

// Batch size.  The persistent traversal kernels pay a tail per launch (ray costs are
// heavy tailed: the last waves finish long after the average one), so launches should be
// few and large: up to 160 M samples per batch -- a whole 1080p / 64 spp frame, ~80 GB of
// queues plus the shadow queue -- bounded by 40 % of the free HBM, unless told otherwise.
// Measured on C3: 4 M samples per batch 473 ms/frame, 80 M 392 ms, whole frame 390 ms; later,
// with a 196 ms frame: two batches 195.8 ms, one 192.9 ms.
// In this order: the options, the cold start, the memory share (of `free_now` bytes), the clamps.
long plan_batch_tiles(const fjgpu_scene *sc, const FramePlan &P, size_t free_now)
{
  const size_t full_tile_samples = P.full_tile_samples;
  long bt = sc->batch_tiles;
  // (a caller that renders ONE frame per scene -- SiRenderScene -- asks for batches of a few M samples: the work arena is then a few GB
  // instead of ~110 GB at the headline size, and a cold frame does not wait for the driver to hand out, and clear, that much memory)
  if (bt <= 0 && sc->batch_samples > 0) bt = std::max<long>(1, (long) ((size_t) sc->batch_samples / full_tile_samples));
  // COLD START: a scene's FIRST call renders in batches of FJ_COLD_BATCH_SAMPLES samples whatever the memory would hold -- a work arena of ~14 GB
  // instead of ~110 GB at the headline size: the first image is there after 0.15 s instead of the 2-5 s hipMalloc takes to hand out (and, after a process
  // that has just ended, clear) the large arena (profiles/r05_e2e_scene.txt).  The second call sizes its batches by memory as before and pays for the
  // growth once; a caller that renders one frame per scene never does.  ("cold_start" 0 / FJGPU_COLD_START=0: the first call already sizes by memory.)
  if (bt <= 0 && sc->render_calls == 0 && fjgpu::g_cold_start && !P.adaptive) {
    static const int on = [] { const char *e = getenv("FJGPU_COLD_START"); return e ? atoi(e) : 1; }();
    if (on) bt = std::max<long>(1, (long) ((size_t) fjgpu::g_cold_batch_samples / full_tile_samples));
  }
  if (bt <= 0) {
    const size_t per_sample = 32 + (size_t) (P.deepest + 1) * (sizeof(DRay) + sizeof(DPath) + (sc->has_filter_rays ? 12 : 0)) + sizeof(DHit) + 2 * sizeof(DLightRec) + (P.adaptive ? 72 : 0) +
        ((sc->ray_sort_bits > 0 && P.deepest >= 1) ? 24 : 0);       // (the ray sort's keys, slots, permutation and scratch)
    // (a scene without lights queues no shadow rays: the fifth of the HBM that queue may take goes to the ray queues --
    // C4, nine recursion levels: 1010 -> 994 ms per frame.  Walking a whole level in one launch with per-level hit
    // buffers and chunking only the shading was measured too: 130 -> ~50 closest-hit launches per frame, 1005 ms: dropped)
    const double share = sc->n_light_samples == 0 ? .6 : .4;
    const size_t target = std::min<size_t>((size_t) 160 << 20, (size_t) (share * (double) free_now) / per_sample);
    bt = std::max<long>(1, (long) (target / full_tile_samples));
  }
  bt = std::min<long>(bt, (long) P.ids.size());
  bt = std::min<long>(bt, (long) (((size_t) 1 << 31) / full_tile_samples));   // sample slots are 32-bit
  // (a batch that did not fit last time -- a batch_tiles option beyond the memory -- is not tried again frame after frame: each failed attempt
  // allocates and releases tens of GB, 15-20 s per frame measured with batch_tiles = 1020 on C4)
  if (sc->batch_fit_samples && full_tile_samples * (size_t) bt > sc->batch_fit_samples) bt = std::max<long>(1, (long) (sc->batch_fit_samples / full_tile_samples));
  if (bt < 1) bt = 1;
  return bt;
}

// ---- stage 2, reserve: streams and the work arena for batches of P.bt tiles -- or fewer, where the memory is not there

// (asked once per arena: the query is a driver round trip, and a rank's share of a frame is 20 ms; an allocation that fails because
// somebody else took the memory meanwhile halves the batch below)
void query_free(fjgpu_scene *sc)
{
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t) 16 << 30;
  sc->free_cached = free_b + (sc->work ? sc->work->bytes : 0);   // our own work buffers are re-usable
}

// the shadow-queue entries the memory budget allows: a fifth of the free HBM, between 4 M and 512 M entries
void set_squeue_max(fjgpu_scene *sc, size_t free_now)
{
  sc->squeue_max = std::max<size_t>((size_t) 4 << 20, std::min<size_t>((size_t) 512 << 20, (size_t) (.2 * (double) free_now) / sizeof(DShadowRay)));
  if (sc->n_light_samples == 0) sc->squeue_max = (size_t) 4 << 20;
  if (const char *e = getenv("FJGPU_SQUEUE_M")) sc->squeue_max = (size_t) std::max(1, atoi(e)) << 20;
}

void choose_streams(fjgpu_scene *sc, const FramePlan &P)
{
  // light loops beside the next levels' closest-hit walks (option overlap_shadow): on, or by the size of the batch
  sc->overlap_now = !P.adaptive && sc->n_light_samples > 0 && (sc->overlap == 1 || (sc->overlap == 2 && P.deepest >= 1 && P.full_tile_samples * (size_t) P.bt <= FJ_OVERLAP_MAX_SAMPLES));
  if (sc->overlap_now && enable_overlap(sc)) sc->overlap_now = false;
  if (!sc->read_stream) {      // (the speculative walk's counter read-back; without them the loop reads on the main stream as before)
    if (hipStreamCreateWithFlags(&sc->read_stream, hipStreamNonBlocking) != hipSuccess) sc->read_stream = nullptr;
    else if (hipEventCreateWithFlags(&sc->ev_shaded, hipEventDisableTiming) != hipSuccess) { (void) hipStreamDestroy(sc->read_stream); sc->read_stream = nullptr; sc->ev_shaded = nullptr; }
  }
}

int reserve_arena(fjgpu_scene *sc, FramePlan *P, size_t *cap_samples_out, size_t *cap_rays_out)
{
  const size_t full_tile_samples = P->full_tile_samples;
  long &bt = P->bt;
  set_squeue_max(sc, sc->free_cached);
  size_t cap_samples = 0, cap_rays = 0;
  bool requeried = false;
  for (;;) {
    cap_samples = full_tile_samples * (size_t) bt;
    // one level holds at most the rays its parent chunk can emit (the scheduler chunks by
    // max_children), so a queue never needs more than one entry per sample
    // (small frames get queues of at least 8 M entries: with room for the worst-case fan-out the
    // scheduler does not have to cut their levels into chunks of a few thousand rays)
    cap_rays = std::max<size_t>(cap_samples, std::min<size_t>((size_t) 8 << 20, cap_samples * 16)) + 1024;
    // the arena is about to be replaced: the shadow queue's bound follows what is free NOW, not what was free when the scene's first
    // frame asked (other scenes or processes may have allocated since)
    if (!requeried && sc->work && (cap_samples > sc->work_samples || cap_rays > sc->work_rays || (int) bt > sc->tiles_cap ||
                                   (sc->overlap_now ? FJ_LREC_BUFS : 2) > sc->lrec_bufs)) {
      requeried = true;
      query_free(sc);
      set_squeue_max(sc, sc->free_cached);
    }
    bool ok = ensure_work(sc, cap_samples, cap_rays, (int) bt, full_tile_samples) == 0;
    // every reachable level now, so that a failure shrinks the batch instead of ending the frame
    // (level 0 only where camera rays are explicit records: implicit_camera_rays)
    for (int l = P->implicit_cam ? 1 : 0; ok && l <= P->deepest; l++) ok = ensure_level(sc, l, cap_rays) == 0;
    // ... and the ray sort's scratch (a failure here also halves the batch)
    if (ok && sc->ray_sort_bits > 0 && P->deepest >= 1) ok = ensure_sort(sc, cap_rays) == 0;
    if (ok) break;
    (void) hipGetLastError();
    if (bt == 1) return fail(FJGPU_ENOMEM, "device allocation failed for the wavefront work buffers");
    // another process holds part of the HBM: half the batch (the old arena is released first)
    fjgpu::ForgetWorkArena(sc);
    sc->free_cached = 0;
    bt = std::max<long>(1, bt / 2);
    sc->batch_fit_samples = full_tile_samples * (size_t) bt;      // (at most this from now on; a smaller one that fails lowers it again)
  }
  *cap_samples_out = cap_samples; *cap_rays_out = cap_rays;
  return 0;
}

// ---- stage 3, the launch parameters of the frame

struct LaunchParams {
  DScene S;
  GenParams gp;
  ShadeParams shp;
  ShadowParams swp;
  ResolveParams rp;
  AdaptiveParams ap;
  // FIRST TOUCH: the fixed-grid sampler queues every sample of the batch exactly once at level 0, entry i of a launch at chunk offset
  // `off` being sample off + i (implicit camera rays by construction, explicit ones because camera_path writes sample = slot), and nothing adds to
  // d_accum between the previous batch's resolve and this batch's level-0 shading launches: a batch ends with finish_shadow() -- the main stream waits
  // for the shadow stream -- and its resolve, and the host synchronises with both before the next batch or call.  So level 0 stores its samples and
  // the batch's memset of d_accum is not needed.  (The adaptive sampler queues SOME samples per pass and reads the others: it keeps the memset.)
  bool first_touch;
};

void fill_launch_params(const fjgpu_scene *sc, const fj_render_desc *r, const FramePlan &P, size_t cap_rays, LaunchParams *L)
{
  const int *margin = P.margin;
  DScene &S = L->S;
  S = sc->S;
  camera_uv_size(sc->cam_fov, r, S.cam_uv_size);
  S.time_tab = sc->d_tim; S.time_start = r->time_start; S.time_end = r->time_end;
  S.lrec_hair = nullptr;      // set per launch (double buffered)

  L->gp = gen_params(r, margin);
  ShadeParams &shp = L->shp;
  shp.max_diffuse_depth = r->max_diffuse_depth; shp.max_reflect_depth = r->max_reflect_depth; shp.max_refract_depth = r->max_refract_depth;
  shp.count_all_shadow = (int) sc->count_all_shadow;
  shp.ray_capacity = (uint32_t) cap_rays; shp.light_capacity = (uint32_t) cap_rays;
  shp.fc_in = nullptr; shp.fc_out = nullptr;
  shp.next_keys = nullptr; shp.sort_bits = std::max(1, std::min(9, sc->ray_sort_bits)); shp.first_touch = 0;
  L->first_touch = !P.adaptive && sc->shade_first_touch != 0;
  ray_sort_grid(sc->scene_box, shp.sort_bits, shp.sort_lo, shp.sort_scale);
  ShadowParams &swp = L->swp;
  swp.cos_half_pi = std::cos(3.14159265358979323846 / 2.);
  swp.cos_pi = std::cos(3.14159265358979323846);
  swp.pre_resolve = (S.all_opaque && !S.has_curves && !S.has_motion && S.blas_base) ? 1 : 0;   // the lean any-hit walk consumes the queue
  swp.cast_shadow = r->cast_shadow;
  // compact queue records (DShadowRayC) where the consumers rebuild direction and distance: the lean and the curve any-hit walk, point / dome lights, no motion
  S.compact_squeue = scene_compact_squeue(S) ? 1 : 0;
  S.pad_cs_ = 0;
  swp.compact = S.compact_squeue;
  swp.light_cones = (sc->light_cones && S.light_cones && S.cone_rows) ? 1 : 0;
  swp.pad_ = 0;
  swp.light_hulls = (swp.light_cones && sc->light_hulls && S.light_hulls && S.hull_rows) ? 1 : 0;
  swp.queue_capacity = (uint32_t) sc->squeue_cap;
  swp.join_capacity = (swp.pre_resolve && sc->split_shadow && sc->d_join) ? (uint32_t) sc->join_cap : 0u;
  S.shadow_join = swp.join_capacity ? sc->d_join : nullptr;
  S.shadow_queue_cap = (uint32_t) sc->squeue_cap;
  ResolveParams &rp = L->rp;
  rp.xres = r->xres; rp.yres = r->yres; rp.rate_x = r->rate_x; rp.rate_y = r->rate_y;
  rp.npx_x = r->rate_x + 2 * margin[0]; rp.npx_y = r->rate_y + 2 * margin[1];
  AdaptiveParams &ap = L->ap;
  std::memset(&ap, 0, sizeof(ap));
  if (P.adaptive) {
    ap.D = r->adaptive_max_subdivision; ap.div = P.a_div;
    ap.margin_x = margin[0]; ap.margin_y = margin[1];
    ap.udelta = 1. / (P.a_div * r->xres);
    ap.vdelta = 1. / (P.a_div * r->yres);
    ap.jitter = r->jitter;
    ap.jittered = r->jitter > 0 ? 1 : 0;
    ap.threshold = (double) r->adaptive_subdivision_threshold;
    ap.ray_capacity = (uint32_t) cap_rays;
    // get_sampleset_in_pixel (src/fj_adaptive_grid_sampler.cc:172-193): a pixel's window starts
    // div samples after its neighbour's and is div * (1 + 2 margin) + 1 samples wide
    rp.rate_x = rp.rate_y = P.a_div;
    rp.npx_x = P.a_div * (1 + 2 * margin[0]) + 1; rp.npx_y = P.a_div * (1 + 2 * margin[1]) + 1;
  }
  rp.fw = (double) r->filter_w; rp.fh = (double) r->filter_h;
}

// ---- the launch timer.  Per-launch timing without a host round trip per launch: event pairs are recorded around
// every launch on its stream and turned into durations once, after the frame's last sync.
struct LaunchTimer {
  struct Span { size_t a, b; double *bucket; };
  fjgpu_scene *sc;
  std::vector<Span> spans;
  size_t ev_used = 0;

  explicit LaunchTimer(fjgpu_scene *scene) : sc(scene) {}
  size_t take_event()
  {
    if (ev_used == sc->ev_pool.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return (size_t) -1; sc->ev_pool.push_back(e); }
    return ev_used++;
  }
  template <class Launch> int timed(hipStream_t stream, double *bucket, Launch &&launch)
  {
    const size_t a = take_event(), b = take_event();
    if (a == (size_t) -1 || b == (size_t) -1) return -1;
    (void) hipEventRecord(sc->ev_pool[a], stream);
    const int le = launch();
    (void) hipEventRecord(sc->ev_pool[b], stream);
    if (le) return le;
    spans.push_back(Span{a, b, bucket});
    return 0;
  }
  // the launch timed last turned out to have had nothing to do (a speculative walk of no rays): its span is not counted
  void drop_last() { spans.pop_back(); }
  // after the frame's last synchronisation: every span into its bucket
  void resolve()
  {
    float ms = 0;
    for (const Span &sp : spans)
      if (hipEventElapsedTime(&ms, sc->ev_pool[sp.a], sc->ev_pool[sp.b]) == hipSuccess) *sp.bucket += ms;
  }
};

// ---- the tiles of one batch as the kernels see them
struct BatchLayout {
  std::vector<TileDesc> td;
  uint32_t n_samples = 0, max_ts = 0, cells0 = 0;     // cells0: lattice cells of the coarsest level (adaptive sampler)
  int max_px = 0, max_w0 = 0, max_h0 = 0;
};

void layout_batch(const fjgpu_scene *sc, const fj_render_desc *r, const FramePlan &P, size_t b0, int nb, BatchLayout *B)
{
  B->td.resize(nb);
  uint32_t off = 0;
  for (int k = 0; k < nb; k++) {
    const fjgpu::TileRect &t = P.all[P.ids[b0 + k]];
    TileDesc &d = B->td[k];
    d = fixed_grid_tile(sc, r, t, P.margin, off);
    d.cell_offset = B->cells0;
    if (P.adaptive) {
      const int w0 = t.xmax - t.xmin + 2 * P.margin[0], h0 = t.ymax - t.ymin + 2 * P.margin[1];
      d.nx = P.a_div * w0 + 1; d.ny = P.a_div * h0 + 1;
      B->cells0 += (uint32_t) w0 * (uint32_t) h0;
      B->max_w0 = std::max(B->max_w0, w0); B->max_h0 = std::max(B->max_h0, h0);
    }
    off += (uint32_t) d.nx * (uint32_t) d.ny;
    B->max_ts = std::max(B->max_ts, (uint32_t) d.nx * (uint32_t) d.ny);
    B->max_px = std::max(B->max_px, (t.xmax - t.xmin) * (t.ymax - t.ymin));
  }
  B->n_samples = off;
}

// ---- stage 4, the batches.
// Depth-first wavefront schedule: the rays of one recursion level live in that
// level's queue; a level is consumed in chunks small enough that the children a
// chunk can emit (max_children per ray) fit the next level's queue, and that
// queue is drained completely before the next chunk is taken.  Memory is bounded
// by levels x capacity whatever the branching of the shaders (glass: 2 children,
// pathtracing: up to 3), while plastic-only scenes run whole levels at once.
struct BatchRun {
  fjgpu_scene *sc;
  const FramePlan &P;
  const LaunchParams &L;
  LaunchTimer &T;
  fjgpu_stats &acc;
  const size_t cap_rays;
  const hipStream_t st;
  // The light loop and the shadow traversal of level L are independent of the closest-hit
  // work of level L+1 (both consume what shading L produced), so they run on their own
  // stream and fill each other's tails; light records are double buffered between them.
  const hipStream_t sst;
  const unsigned lrec_ring;
  unsigned shade_seq = 0;
  bool shadow_pending[FJ_LREC_BUFS] = {false, false, false, false};
  // shadow-ray queue of a batch: the light loops of every level append, one traversal
  // launch consumes it (flush) at the end of the batch or when it could overflow
  const uint64_t sq_cap, sq_pad, nl_q;
  uint64_t sq_bound = 0;             // upper bound of the entries reserved so far
  bool sq_dirty = false;
  // SPECULATIVE WALK (round 5): after the shading launch of a level the host needs two counters back -- how many children, how many light
  // records -- before it can go on, and the device used to wait 40-145 us for that round trip at every level.  The children's closest-hit walk does
  // not need the host to know: it is enqueued right behind the shading launch and reads its ray count from the counter itself (DScene.trace_n_dev,
  // bounded by the chunk the host would have cut), while the counters come back on a stream of their own.  `walk_launched`: process() was called
  // for rays whose first chunk is already being walked.
  bool walk_launched = false;
  bool speculate;

  BatchRun(fjgpu_scene *scene, const FramePlan &plan, const LaunchParams &params, LaunchTimer &timer, fjgpu_stats &stats, size_t ray_capacity, hipStream_t stream)
    : sc(scene), P(plan), L(params), T(timer), acc(stats), cap_rays(ray_capacity), st(stream),
      sst((scene->overlap_now && scene->shadow_stream) ? scene->shadow_stream : stream),
      lrec_ring((sst != st && scene->lrec_bufs >= FJ_LREC_BUFS) ? FJ_LREC_BUFS : 2),
      sq_cap(scene->squeue_cap), sq_pad(shadow_queue_padding()),
      nl_q((uint64_t) std::max(1, scene->n_light_samples) * (params.S.shadow_join ? scene->split_kfac : 1u))
  {
    static const bool spec_env = [] { const char *e = getenv("FJGPU_SPEC_WALK"); return e ? atoi(e) != 0 : true; }();
    speculate = fjgpu::g_spec_walk && spec_env && sc->ray_sort_bits <= 0 && sc->read_stream && sc->ev_shaded;
  }

  // a chunk of one level's queue: entries [off, off + n)
  struct Chunk { int level; uint32_t off, n; bool can_emit, implicit; const DRay *rays; const DPath *paths; };

  void begin_shadow_queue()
  {
    sq_bound = 0; sq_dirty = false; walk_launched = false;
    shadow_queue_reset(sst, sc->d_cnt);
  }

  int flush_shadow(const DScene &Sx)
  {
    if (sq_dirty) {
      const int fe = T.timed(sst, &acc.shadow_walk_ms, [&]() {
        return launch_shadow_trace(sst, Sx, sc->d_squeue, sc->d_accum, sc->d_cnt, (int) sc->count_events);
      });
      if (fe) return fe;
      acc.trace_launches++; acc.shadow_walk_launches++;
      shadow_queue_reset(sst, sc->d_cnt);
    }
    sq_bound = 0; sq_dirty = false;
    return 0;
  }

  // the filter (and the adaptive sampler's decisions) need every shadow contribution so far
  int finish_shadow()
  {
    DScene Sf = L.S; Sf.lrec_hair = nullptr;
    const int fe = flush_shadow(Sf);
    if (fe) return fe;
    if (sst != st) { (void) hipEventRecord(sc->ev_shadow_done[0], sst); shadow_pending[0] = true; }
    for (int k = 0; k < FJ_LREC_BUFS; k++) if (shadow_pending[k] && sst != st) { (void) hipStreamWaitEvent(st, sc->ev_shadow_done[k], 0); shadow_pending[k] = false; }
    return 0;
  }

  // the camera fields of a launch over implicit level-0 entries
  void implicit_chunk(DScene *Sx, const Chunk &c) const
  {
    Sx->cam_uv = sc->d_suv + 2 * (size_t) c.off; Sx->cam_slot0 = c.off; Sx->cam_tk = P.tk_cam ? sc->d_stk + 2 * (size_t) c.off : nullptr;
  }

  // the closest-hit walk of a chunk, behind the sort of its rays where they are sorted; `skip_walk`: a speculative launch already walks them
  int sort_and_walk(const Chunk &c, bool skip_walk)
  {
    (void) hipMemsetAsync(&sc->d_cnt->next_count, 0, sizeof(uint32_t) * 2, st);   // next_count + light_count
    // secondary rays leave the shading kernel in emission order: walk them in (octant, cell) order
    DScene St = L.S;
    if (c.implicit) implicit_chunk(&St, c);
    if (sc->ray_sort_bits > 0 && c.level >= 1 && (long) c.n >= fjgpu::g_ray_sort_min) {
      if (ensure_sort(sc, cap_rays)) return fail(FJGPU_ENOMEM, "device allocation failed for the ray sort");   // (sized with the queues: cannot fail here)
      // (the keys were written by the shading kernel that emitted these rays: ShadeParams.next_keys)
      const int e = T.timed(st, &acc.sort_ms, [&]() {
        return launch_ray_sort_keyed(st, sc->levels[c.level].keys + c.off, c.n, sc->ray_sort_bits, sc->d_sort[1], sc->d_sort[3],
            sc->d_sort_tmp, sc->sort_tmp_bytes);
      });
      if (e) return e;
      St.ray_perm = sc->d_sort[3];
      acc.rays_sorted += c.n;
    }
    if (!skip_walk) {
      const int e = T.timed(st, &acc.closest_ms, [&]() {
        return launch_trace_closest(st, St, c.rays, c.paths, sc->d_hits, c.n, sc->d_cnt, (int) sc->count_events);
      });
      if (e) return e;
      acc.trace_launches++; acc.closest_launches++;
    }
    return 0;
  }

  // the shading launch of a chunk: children into the next level's queue, light records into buffer *lb of the ring.  *Sl: the scene
  // record of the launch, which the chunk's light loops take too
  int shade(const Chunk &c, unsigned *lb_out, DScene *Sl)
  {
    const unsigned lb = shade_seq++ % lrec_ring;   // light-record buffer of this shading call
    if (shadow_pending[lb] && sst != st) (void) hipStreamWaitEvent(st, sc->ev_shadow_done[lb], 0);
    shadow_pending[lb] = false;
    *Sl = L.S;
    if (c.implicit) implicit_chunk(Sl, c);
    if (L.first_touch && c.level == 0) Sl->cam_slot0 = c.off;      // (explicit camera rays too: the sample of entry i)
    Sl->lrec_hair = sc->d_lhair[lb];
    ShadeParams shl = L.shp;
    shl.first_touch = (L.first_touch && c.level == 0) ? 1 : 0;
    shl.next_keys = (c.can_emit && sc->ray_sort_bits > 0) ? sc->levels[c.level + 1].keys : nullptr;
    shl.fc_in = (!c.implicit && sc->levels[c.level].fc) ? sc->levels[c.level].fc + 3 * (size_t) c.off : nullptr;
    shl.fc_out = c.can_emit ? sc->levels[c.level + 1].fc : nullptr;
    *lb_out = lb;
    return T.timed(st, &acc.shade_ms, [&]() {
      return launch_shade(st, *Sl, shl, c.rays, c.paths, sc->d_hits, c.n, sc->d_accum,
          c.can_emit ? sc->levels[c.level + 1].rays : nullptr, c.can_emit ? sc->levels[c.level + 1].paths : nullptr, sc->d_lrecs[lb], sc->d_cnt);
    });
  }

  // the counters of the chunk's shading launch into *hc -- which the caller owns, and which is complete when this returns: every branch
  // synchronises with the stream its copy went to -- with the children's walk enqueued first where the loop speculates (*launched_next)
  int read_counters(const Chunk &c, uint32_t kids, DCounters *hc, bool *launched_next)
  {
    // (with the light loops on their own stream the ORDER of the launches decides who is resident first: level 0's light loop -- the big one -- must
    // reach the device before level 1's walk fills it, or the two take turns instead of overlapping: C2 93.8 -> 97.3 ms with the walk first; from
    // level 1 on the light loops are small and the round trip is what costs)
    if (speculate && c.can_emit && (sst == st || c.level >= 1)) {
      // the children's walk behind the shading launch, the counters back on the side stream (which waits for the shading launch only)
      if (hipEventRecord(sc->ev_shaded, st) != hipSuccess) return -1;
      DScene Sn = L.S;
      Sn.trace_n_dev = &sc->d_cnt->next_count;
      // (sized by what THIS launch can emit -- n rays, at most `kids` children each -- not by the queue's capacity: a deep level of a few
      //  hundred rays no longer starts a full persistent grid whose waves read the count and leave)
      const uint32_t chunk_cap = kids <= 1 ? (uint32_t) std::min<size_t>(cap_rays, 0xffffffffu) : std::max<uint32_t>(1u, (uint32_t) (cap_rays / kids));
      const uint32_t next_chunk = (uint32_t) std::min<uint64_t>(chunk_cap, (uint64_t) c.n * kids);
      const int e = T.timed(st, &acc.closest_ms, [&]() {
        return launch_trace_closest(st, Sn, sc->levels[c.level + 1].rays, sc->levels[c.level + 1].paths, sc->d_hits, next_chunk, sc->d_cnt, (int) sc->count_events);
      });
      if (e) return e;
      *launched_next = true;
      if (hipStreamWaitEvent(sc->read_stream, sc->ev_shaded, 0) != hipSuccess ||
          hipMemcpyAsync(hc, sc->d_cnt, sizeof(*hc), hipMemcpyDeviceToHost, sc->read_stream) != hipSuccess || hipStreamSynchronize(sc->read_stream) != hipSuccess) return -1;
    }
    else if (hipMemcpyAsync(hc, sc->d_cnt, sizeof(*hc), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
    return 0;
  }

  // the light loops over the hc.light_count records the chunk's shading launch wrote to buffer lb, cut so that the shadow queue holds
  // what they can append
  int queue_light_records(const Chunk &c, const DCounters &hc, unsigned lb, const DScene &Sl)
  {
    // shading has completed (the host just synchronised with it): no event needed.
    // The queue holds hc.shadow_count entries so far (exact when the shadow work runs on
    // this stream, a lower bound otherwise: then the host-side bound is kept).
    if (sst == st) sq_bound = hc.shadow_count;
    uint32_t b = 0;
    bool bound_is_exact = sst == st;
    while (b < hc.light_count) {
      const uint64_t room = sq_cap > (uint64_t) sq_bound + sq_pad ? sq_cap - sq_bound - sq_pad : 0;
      uint32_t can = (uint32_t) std::min<uint64_t>(room / nl_q, hc.light_count - b);
      if (can < hc.light_count - b && !bound_is_exact && sst == st) {
        // the bound assumed that every (record, light) pair survived the cull: ask the
        // device how full the queue really is before paying for a traversal launch
        uint32_t used = 0;
        if (hipMemcpyAsync(&used, &sc->d_cnt->shadow_count, sizeof(used), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
        sq_bound = used;
        bound_is_exact = true;
        continue;
      }
      if (can == 0 || (can < hc.light_count - b && can < (1u << 16))) {
        // not worth a light-loop launch of its own: empty the queue first (an empty queue
        // that still cannot take one record's rays takes them one record at a time)
        if (sq_bound > 0) { const int e = flush_shadow(Sl); if (e) return e; continue; }
        if (can == 0) can = 1;
      }
      acc.light_loop_launches++;
      const int e = T.timed(sst, &acc.light_loop_ms, [&]() {
        return launch_shadow_cull(sst, Sl, L.swp, sc->d_lrecs[lb], b, b + can, sc->d_accum, sc->d_squeue, sc->d_cnt, (int) sc->count_events,
            sst != st ? FJ_OVERLAP_CULL_BLOCKS : 0);
      });
      if (e) return e;
      sq_bound += (uint64_t) can * nl_q + sq_pad;      // worst case: every pair survives, every wave leaves a padded chunk
      bound_is_exact = false;
      sq_dirty = true;
      b += can;
    }
    if (sst != st) { (void) hipEventRecord(sc->ev_shadow_done[lb], sst); shadow_pending[lb] = true; }
    // overlap: the shadow rays of level 0 -- most of a frame's -- are walked NOW, on the shadow stream, while the main stream runs the
    // deeper levels' closest-hit walks, which are a few long rays each (a launch of its own per level, latency bound): the big walk hides them
    // (early_shadow = k: the queue is flushed after level k - 1's light loops -- 2: levels 0 and 1, nearly all of a frame's shadow rays, are walked
    //  beside the closest-hit walks of levels >= 2, which are a few long rays each)
    if (sst != st && sc->early_shadow > 0 && c.level == (int) sc->early_shadow - 1 && c.can_emit && hc.next_count) return flush_shadow(Sl);
    return 0;
  }

  // `count` rays of recursion level `level`, and everything they spawn
  int process(int level, uint32_t count)
  {
    // rays of the deepest reachable level cannot emit children (has_reached_bounce_limit):
    // there is no next queue
    const bool can_emit = level < P.deepest;
    bool skip_walk = walk_launched;      // (the first chunk's walk)
    walk_launched = false;
    if (can_emit && ensure_level(sc, level + 1, cap_rays)) return fail(FJGPU_ENOMEM, "device allocation failed for a ray queue level");
    const uint32_t kids = (uint32_t) std::max(1, sc->max_children);
    const uint32_t chunk_max = kids <= 1 ? count : std::max<uint32_t>(1u, (uint32_t) (cap_rays / kids));
    for (uint32_t off = 0; off < count; off += chunk_max) {
      Chunk c;
      c.level = level; c.off = off; c.n = std::min(chunk_max, count - off);
      c.can_emit = can_emit; c.implicit = P.implicit_cam && level == 0;
      c.rays = c.implicit ? nullptr : sc->levels[level].rays + off;
      c.paths = c.implicit ? nullptr : sc->levels[level].paths + off;
      int e = sort_and_walk(c, skip_walk);
      if (e) return e;
      skip_walk = false;
      unsigned lb = 0;
      DScene Sl;
      e = shade(c, &lb, &Sl);
      if (e) return e;
      DCounters hc;
      bool launched_next = false;
      e = read_counters(c, kids, &hc, &launched_next);
      if (e) return e;
      if (hc.overflow) { sc->split_overflowed = L.S.shadow_join != nullptr; return fail(FJGPU_ENOMEM, "ray queue overflow: lower the batch_tiles option"); }
      if (launched_next && hc.next_count) { acc.trace_launches++; acc.closest_launches++; }       // (a walk of no rays is not counted ...
      else if (launched_next) T.drop_last();                                                      //  ... and not timed: its span was the last one recorded)
      if (hc.light_count) { e = queue_light_records(c, hc, lb, Sl); if (e) return e; }
      if (hc.next_count) {
        if (!can_emit) return fail(FJGPU_EINVAL, "ray recursion deeper than the depth limits allow");
        walk_launched = launched_next;
        e = process(level + 1, hc.next_count);
        if (e) return e;
      }
    }
    return 0;
  }

  // a batch of the fixed-grid sampler: every sample once
  int run_fixed(const BatchLayout &B, int nb)
  {
    const int rc = T.timed(st, &acc.gen_ms, [&]() {
      return launch_gen_camera(st, L.S, L.gp, sc->d_tiles, nb, B.max_ts, sc->d_jit, sc->d_tim, sc->d_suv,
          P.implicit_cam ? nullptr : sc->levels[0].rays, P.implicit_cam ? nullptr : sc->levels[0].paths, P.tk_cam ? sc->d_stk : nullptr);
    });
    if (rc) return rc;
    acc.rays.camera += B.n_samples;
    begin_shadow_queue();
    if (const int e = process(0, B.n_samples)) return e;
    return finish_shadow();
  }

  // a batch of the AdaptiveGridSampler, level by level (fjgpu_dev_adaptive.h): points -> wavefront -> decisions
  int run_adaptive(const BatchLayout &B, int nb)
  {
    begin_shadow_queue();
    AdaptiveParams ap = L.ap;
    ap.cells0 = B.cells0;
    (void) hipMemsetAsync(sc->d_apstate, 0, (size_t) B.n_samples, st);
    (void) hipMemsetAsync(sc->d_acells, 0, (size_t) B.cells0 * (((((size_t) 1) << (2 * (ap.D + 1))) - 1) / 3), st);
    int rc = T.timed(st, &acc.gen_ms, [&]() { return launch_adaptive_uv(st, ap, sc->d_tiles, nb, B.max_ts, sc->d_jit, sc->d_suv); });
    for (int level = 0; level <= ap.D && rc == 0; level++) {
      ap.level = level;
      (void) hipMemsetAsync(&sc->d_cnt->cam_count, 0, sizeof(uint32_t), st);
      const uint32_t max_pts = (uint32_t) ((B.max_w0 << level) + 1) * (uint32_t) ((B.max_h0 << level) + 1);
      rc = T.timed(st, &acc.gen_ms, [&]() {
        return launch_adaptive_points(st, L.S, ap, sc->d_tiles, nb, max_pts, sc->d_acells, sc->d_suv, sc->d_accum, sc->d_apstate,
            sc->d_aseen, sc->levels[0].rays, sc->levels[0].paths, sc->d_cnt);
      });
      if (rc) return rc;
      DCounters hc;
      if (hipMemcpyAsync(&hc, sc->d_cnt, sizeof(hc), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
      if (hc.overflow) return fail(FJGPU_ENOMEM, "camera ray queue overflow in the adaptive sampler");
      acc.rays.camera += hc.cam_count;
      if (hc.cam_count) {
        rc = process(0, hc.cam_count);
        if (rc) return rc;
        rc = finish_shadow();
        if (rc) return rc;
      }
      rc = T.timed(st, &acc.resolve_ms, [&]() {
        return launch_adaptive_decide(st, ap, sc->d_tiles, nb, (uint32_t) (B.max_w0 << level) * (uint32_t) (B.max_h0 << level),
            sc->d_acells, sc->d_accum, sc->d_apstate, sc->d_aseen);
      });
    }
    if (rc) return rc;
    return T.timed(st, &acc.resolve_ms, [&]() {
      return launch_adaptive_fill(st, ap, sc->d_tiles, nb, B.max_ts, sc->d_acells, sc->d_accum, sc->d_apstate, sc->d_aseen, sc->d_afinal);
    });
  }
};

// ---- stage 5, the counters of a finished batch into the call's statistics and the scene's peaks
void fold_counters(const DCounters &hc, fjgpu_stats *acc, fjgpu_scene *sc)
{
  acc->rays.shadow += hc.rays[CXT_SHADOW_RAY];
  acc->rays.diffuse += hc.rays[CXT_DIFFUSE_RAY];
  acc->rays.reflect += hc.rays[CXT_REFLECT_RAY];
  acc->rays.refract += hc.rays[CXT_REFRACT_RAY];
  acc->nodes_visited += hc.nodes;
  acc->prims_tested += hc.prims;
  acc->insts_tested += hc.insts;
  acc->rays_traced += hc.traced;
  acc->shadow_traversed += hc.squeued;
  acc->shadow_nodes += hc.sh_nodes; acc->shadow_prims += hc.sh_prims; acc->shadow_insts += hc.sh_insts;
  sc->stack_peak_closest = std::max(sc->stack_peak_closest, hc.stack_peak);
  sc->stack_peak_shadow = std::max(sc->stack_peak_shadow, hc.sh_stack_peak);
  sc->hull_verdicts += hc.hull_settled;
  acc->batches++;
}

int render_tiles_once(fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    float *d_fb, void *hip_stream, fjgpu_stats *stats, const SampleVarianceOut *sv)
{
  if (const int e = check_request(r)) return e;
  HIP_TRY(hipSetDevice(sc->device));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  sc->stack_peak_closest = sc->stack_peak_shadow = 0;
  sc->hull_verdicts = 0;
  sc->accum_memsets = 0;

  // plan
  FramePlan P;
  if (const int e = plan_tiles(sc, r, tile_ids, n_tiles, &P)) return e;
  if (!sc->work || sc->free_cached == 0) query_free(sc);
  if (sc->levels.size() < (size_t) P.deepest + 1) sc->levels.resize((size_t) P.deepest + 1, fjgpu_scene::Level{nullptr, nullptr, 0, nullptr});
  P.bt = plan_batch_tiles(sc, P, sc->free_cached);

  // reserve
  choose_streams(sc, P);
  size_t cap_samples = 0, cap_rays = 0;
  if (const int e = reserve_arena(sc, &P, &cap_samples, &cap_rays)) return e;
  // adaptive grid: split / leaf byte per lattice cell of every level (4/3 of the finest level)
  const size_t a_cells0_cap = P.adaptive ? (size_t) P.bt * (size_t) (r->tile_w + 2 * P.margin[0]) * (size_t) (r->tile_h + 2 * P.margin[1]) : 0;
  const size_t a_cell_bytes = a_cells0_cap * (((((size_t) 1) << (2 * (r->adaptive_max_subdivision + 1))) - 1) / 3);
  if (P.adaptive && a_cells0_cap >= ((size_t) 1 << 32)) return fail(FJGPU_EINVAL, "too many lattice cells per batch: lower the batch_tiles option");
  if (P.adaptive && ensure_adaptive(sc, cap_samples, a_cell_bytes))
    return fail(FJGPU_ENOMEM, "device allocation failed for the adaptive sampler's buffers");

  // parameters
  LaunchParams L;
  fill_launch_params(sc, r, P, cap_rays, &L);

  // batches
  fjgpu_stats acc;
  std::memset(&acc, 0, sizeof(acc));
  LaunchTimer T(sc);
  BatchRun run(sc, P, L, T, acc, cap_rays, st);
  int rc = 0;
  hipEvent_t *ev_all = sc->ev_frame;      // (created once per scene: two driver calls less per frame)
  if (!ev_all[0]) { HIP_TRY(hipEventCreate(&ev_all[0])); HIP_TRY(hipEventCreate(&ev_all[1])); }
  (void) hipEventRecord(ev_all[0], st);
  for (size_t b0 = 0; b0 < P.ids.size() && rc == 0; b0 += (size_t) P.bt) {
    const int nb = (int) std::min<size_t>((size_t) P.bt, P.ids.size() - b0);
    BatchLayout B;
    layout_batch(sc, r, P, b0, nb, &B);
    if ((hipMemcpyAsync(sc->d_tiles, B.td.data(), sizeof(TileDesc) * nb, hipMemcpyHostToDevice, st)) != hipSuccess) { rc = -1; break; }
    if (!L.first_touch) { (void) hipMemsetAsync(sc->d_accum, 0, sizeof(float) * 4 * (size_t) B.n_samples, st); sc->accum_memsets++; }
    (void) hipMemsetAsync(sc->d_cnt, 0, sizeof(DCounters), st);
    rc = P.adaptive ? run.run_adaptive(B, nb) : run.run_fixed(B, nb);
    if (rc) break;
    rc = T.timed(st, &acc.resolve_ms, [&]() {
      return launch_resolve(st, L.rp, sc->d_tiles, nb, B.max_px, sc->d_suv, sc->d_accum, P.adaptive ? sc->d_afinal : nullptr, d_fb);
    });
    if (rc) break;
    // fjgpu_render_tiles_variance: the same samples once more, while the batch still holds them
    if (sv) {
      rc = T.timed(st, &acc.resolve_ms, [&]() {
        return launch_sample_variance(st, L.rp, sc->d_tiles, nb, B.max_px, sc->d_suv, sc->d_accum, sv->albedo, sv->albedo_floor, sv->variance);
      });
      if (rc) break;
    }
    DCounters hc;
    if (hipMemcpyAsync(&hc, sc->d_cnt, sizeof(hc), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { rc = -1; break; }
    if (hc.overflow) { sc->split_overflowed = L.S.shadow_join != nullptr; rc = fail(FJGPU_ENOMEM, "wavefront queue overflow: lower the batch_tiles option"); break; }
    fold_counters(hc, &acc, sc);
    if (sc->batch_fn) {
      // (the stream was synchronised above: the batch's pixels are final in d_fb)
      const std::vector<int32_t> bids(P.ids.begin() + (long) b0, P.ids.begin() + (long) b0 + nb);
      if (sc->batch_fn(sc->batch_user, sc->device, bids.data(), nb)) { acc.interrupted = 1; break; }
    }
  }

  // totals
  (void) hipEventRecord(ev_all[1], st);
  hipError_t se = hipStreamSynchronize(st);
  if (run.sst != st) { const hipError_t s2 = hipStreamSynchronize(run.sst); if (se == hipSuccess) se = s2; }
  if (rc == 0 && se == hipSuccess) {
    float ms = 0;
    (void) hipEventElapsedTime(&ms, ev_all[0], ev_all[1]);
    acc.total_ms = ms;
    T.resolve();
    acc.closest_ms += acc.sort_ms;       // the sort is part of what the closest-hit side costs
    acc.trace_ms = acc.closest_ms + acc.light_loop_ms + acc.shadow_walk_ms;
  }
  if (rc > 0 || rc == -1) return fail(FJGPU_ENODEV, std::string("HIP failure in the wavefront loop: ") + hipGetErrorString(hipGetLastError()));
  if (rc) return rc;
  if (se != hipSuccess) return fail(FJGPU_ENODEV, std::string("stream synchronize: ") + hipGetErrorString(se));
  if (stats) *stats = acc;
  return 0;
}

int render_tiles_retrying(fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    float *d_fb, void *hip_stream, fjgpu_stats *stats, const SampleVarianceOut *sv)
{
  sc->split_overflowed = false;
  int e = render_tiles_once(sc, r, tile_ids, n_tiles, d_fb, hip_stream, stats, sv);
  if (e == FJGPU_ENOMEM && sc->split_overflowed) {
    // rays queued once per candidate instance outgrew the host's bound on the shadow queue (a scene whose
    // instance boxes overlap many times over): this scene goes back to whole rays and the tiles are rendered again
    // (said once per scene, verbose or not: from here on the scene's frames take the slower path)
    fprintf(stderr, "fjgpu: shadow queue overflow with rays split per candidate instance: rendering the tiles again without the split, "
        "which stays off for this scene (option split_shadow)\n");
    sc->split_shadow = false;
    e = render_tiles_once(sc, r, tile_ids, n_tiles, d_fb, hip_stream, stats, sv);
  }
  if (!e) sc->render_calls++;
  return e;
}

}  // namespace

extern "C" {

int fjgpu_render_tiles(fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    float *d_fb, void *hip_stream, fjgpu_stats *stats)
{
  if (!sc || !r || !d_fb) return fail(FJGPU_EINVAL, "null argument");
  return render_tiles_retrying(sc, r, tile_ids, n_tiles, d_fb, hip_stream, stats, nullptr);
}

int fjgpu_render_tiles_variance(fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    float *d_fb, const float *d_albedo, float albedo_floor, float *d_variance, void *hip_stream, fjgpu_stats *stats)
{
  const std::string f = "fjgpu_render_tiles_variance";
  if (!sc || !r || !d_fb || !d_variance) return fail(FJGPU_EINVAL, f + ": null argument (scene, render, framebuffer and variance are required)");
  if (d_albedo && !(std::isfinite(albedo_floor) && albedo_floor > 0)) return fail(FJGPU_EINVAL, f + ": albedo_floor must be finite and > 0");
  if (const char *why = bad_render(r)) return fail(FJGPU_EINVAL, f + ": " + why);
  const size_t px = (size_t) r->xres * (size_t) r->yres;
  auto overlaps = [](const float *a, size_t na, const float *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t) a, b0 = (uintptr_t) b;
    return a0 < b0 + nb * sizeof(float) && b0 < a0 + na * sizeof(float);
  };
  if (overlaps(d_variance, px, d_fb, 4 * px) || (d_albedo && overlaps(d_variance, px, d_albedo, 3 * px)))
    return fail(FJGPU_EINVAL, f + ": the variance buffer must not overlap the framebuffer or the albedo buffer");
  // (the adaptive sampler resolves INTERPOLATED samples: they are not independent draws, and their spread is not the estimate's variance)
  if (r->sampler_type == 1) return fail(FJGPU_EUNSUPPORTED, f + ": the adaptive sampler is not supported (its resolved samples are interpolated, not independent)");
  const SampleVarianceOut sv = {d_variance, d_albedo, albedo_floor};
  return render_tiles_retrying(sc, r, tile_ids, n_tiles, d_fb, hip_stream, stats, &sv);
}

}  // extern "C"
