// fjgpu_api.hip -- C ABI of libfjgpu.so (include/fjgpu.h), the entry points that take a fjgpu_scene: device scene
// residency, options and queries, the multi-device frame, the ray-batch trace entry point, the AOV pass and the camera of a resident scene.
// (the beauty pass -- fjgpu_render_tiles, the work arena and the wavefront frame loop -- is in fjgpu_frame.hip, the scene record in
// fjgpu_scene.h; the image-space passes, which take only buffers, are in fjgpu_image_api.hip)
#include <hip/hip_runtime.h>
#include <mutex>
#include <map>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "fjgpu.h"
#include "fjgpu_api_common.h"
#include "fjgpu_build.h"
#include "fjgpu_kernels.h"
#include "fjgpu_lbvh.h"
#include "fjgpu_light_cone.h"
#include "fjgpu_light_hull.h"
#include "fjgpu_matte.h"
#include "fjgpu_raysort.h"
#include "fjgpu_scene.h"
#include "fjgpu_tlas.h"

// the ONE error text of the library: every translation unit sets it through fjgpu::fail (fjgpu_api_common.h)
static thread_local std::string t_last_error;

int fjgpu::fail(int code, const std::string &msg)
{
  t_last_error = msg;
  return code;
}

namespace {

using fjgpu::fail;
using fjgpu::DeviceBuffers;

// ---- RCCL, loaded at first use (no link-time dependency: the single-device paths never need it).  The slab exchange of
// fjgpu_render_frame_multi in RCCL's spelling -- ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd, SURVEY 8(e) -- beside the peer copy.
struct Rccl {
  typedef void *comm_t;
  int (*CommInitAll)(comm_t *, int, const int *) = nullptr;
  int (*CommDestroy)(comm_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*Send)(const void *, size_t, int, int, comm_t, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, comm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  void *handle = nullptr;
  bool ok = false;
  static constexpr int kFloat = 7;          // ncclFloat32 (rccl.h)
};

Rccl &rccl()
{
  static Rccl R;
  static std::once_flag once;
  std::call_once(once, []() {
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { R.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (R.handle) break; }
    if (!R.handle) return;
    auto sym = [&](const char *n) { return dlsym(R.handle, n); };
    R.CommInitAll = (decltype(R.CommInitAll)) sym("ncclCommInitAll");
    R.CommDestroy = (decltype(R.CommDestroy)) sym("ncclCommDestroy");
    R.GroupStart = (decltype(R.GroupStart)) sym("ncclGroupStart");
    R.GroupEnd = (decltype(R.GroupEnd)) sym("ncclGroupEnd");
    R.Send = (decltype(R.Send)) sym("ncclSend");
    R.Recv = (decltype(R.Recv)) sym("ncclRecv");
    R.GetErrorString = (decltype(R.GetErrorString)) sym("ncclGetErrorString");
    R.ok = R.CommInitAll && R.CommDestroy && R.GroupStart && R.GroupEnd && R.Send && R.Recv;
  });
  return R;
}

// one communicator set per list of devices, created at first use and kept until the process exits (bring-up takes of the order of a second);
// destroyed by an atexit hook -- live communicators at exit are a known source of RCCL shutdown hangs.  A failed bring-up is remembered WITH its
// reason (the next frame falls back to peer copies at once and says why) and is retried after FJ_RCCL_RETRY_CALLS calls.
#define FJ_RCCL_RETRY_CALLS 64
struct RcclSet { std::vector<Rccl::comm_t> comms; std::string why; int calls_since_failure = 0; };
std::mutex g_rccl_mu;
std::map<std::vector<int>, RcclSet> g_rccl_comms;

void rccl_destroy_all()
{
  Rccl &R = rccl();
  std::lock_guard<std::mutex> lock(g_rccl_mu);
  for (auto &kv : g_rccl_comms)
    for (Rccl::comm_t c : kv.second.comms) if (c && R.CommDestroy) (void) R.CommDestroy(c);
  g_rccl_comms.clear();
}

const std::vector<Rccl::comm_t> *rccl_comms(const std::vector<int> &devices, std::string *why)
{
  Rccl &R = rccl();
  if (!R.ok) { *why = "librccl.so not loadable"; return nullptr; }
  std::lock_guard<std::mutex> lock(g_rccl_mu);
  static bool hooked = false;
  if (!hooked) { hooked = true; atexit(rccl_destroy_all); }
  auto it = g_rccl_comms.find(devices);
  if (it != g_rccl_comms.end()) {
    if (!it->second.comms.empty()) return &it->second.comms;
    if (++it->second.calls_since_failure < FJ_RCCL_RETRY_CALLS) { *why = it->second.why + " (remembered)"; return nullptr; }
    g_rccl_comms.erase(it);
  }
  RcclSet set;
  set.comms.assign(devices.size(), nullptr);
  const int e = R.CommInitAll(set.comms.data(), (int) devices.size(), devices.data());
  if (e) { set.why = std::string("ncclCommInitAll: ") + (R.GetErrorString ? R.GetErrorString(e) : "error"); set.comms.clear(); *why = set.why; }
  auto &slot = g_rccl_comms[devices] = set;
  return slot.comms.empty() ? nullptr : &slot.comms;
}

}  // namespace

static int grow(void **p, size_t *have, size_t want, size_t elem)
{
  if (*have >= want && *p) return 0;
  if (*p) (void) hipFree(*p);
  *p = nullptr; *have = 0;
  if (hipMalloc(p, std::max<size_t>(want, 1) * elem) != hipSuccess) return -1;
  *have = want;
  return 0;
}

// FLAT groups (DFlat, fjgpu_dev_flat.h): when EVERY group of a scene with incoherent closest-hit rays holds only small static meshes built on
// the host, each group gets one world-space culling tree over the triangles of all its instances.  Returns the flats (empty: not applicable)
// and the deepest stack any of the trees needs.
#ifndef FJ_FLAT_MAX_TRIS
#define FJ_FLAT_MAX_TRIS (1 << 21)
#endif

struct HostFlat { fjgpu::HostPrimSet tree; std::vector<DFlatRef> refs; std::vector<double> refbox; double grid[6]; };
// one group: false if it cannot be flattened (an instance that is not a static, host-built, f32-exact mesh; more than 32 instances or max_tris triangles)
static bool build_flat_group(const fjgpu::HostScene &hs, size_t g, size_t max_tris, HostFlat *Fp)
{
  const DGroup &G = hs.groups[g];
  // the instances in the order the walks (and the reference's BVH) visit them: the leaves of the threaded instance level
  std::vector<int> order;
  for (int k = G.first; k < G.first + G.count; k++) if (hs.group_nodes[k].inst >= 0) order.push_back(hs.group_nodes[k].inst);
  if (order.empty() || order.size() > 32 || (int) order.size() != G.n_instances) return false;
  size_t total = 0;
  std::vector<size_t> first_ref(order.size() + 1, 0);
  for (size_t pos = 0; pos < order.size(); pos++) {
    const int inst = order[pos];
    const DInstance &I = hs.instances[inst];
    const fjgpu::HostPrimSet &ps = hs.primsets[I.primset];
    if (ps.type != FJ_PRIMSET_MESH || ps.device_build || I.xform >= 0 || !ps.tri_vel.empty() || inst >= (1 << 24)) return false;
    if (ps.n_prims > 0 && ps.tri_verts32.empty()) return false;          // (the leaf records hold f32 triangles: exact only for such sets)
    first_ref[pos] = total;
    total += (size_t) ps.n_prims;
  }
  first_ref[order.size()] = total;
  if (total > max_tris || total >= ((size_t) 1 << 28)) return false;
  HostFlat &F = *Fp;
  std::vector<fjgpu::PrimRef> prs(total);
  std::vector<DFlatRef> src(total);
  double gmn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, gmx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  bool finite = true;
  for (size_t pos = 0; pos < order.size(); pos++) {
    const int inst = order[pos];
    const DInstance &I = hs.instances[inst];
    const fjgpu::HostPrimSet &ps = hs.primsets[I.primset];
    const double *rb = order.size() == 1 ? G.sbounds : I.wbounds;
    for (int k = 0; k < 6; k++) F.refbox.push_back(rb[k]);
    const size_t base = first_ref[pos];
    const int n = ps.n_prims;
    // (threads over the triangles of the instance: C2's group is 17.4 M of them)
    const unsigned hc = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    std::vector<char> bad(hc, 0);
    for (unsigned t = 0; t < hc; t++) th.emplace_back([&, t]() {
      for (int k = (int) ((size_t) n * t / hc); k < (int) ((size_t) n * (t + 1) / hc); k++) {
        double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        for (int v = 0; v < 3; v++) {
          double p[3];
          for (int a = 0; a < 3; a++) p[a] = (double) ps.tri_verts32[(size_t) k * 9 + 3 * v + a];
          for (int a = 0; a < 3; a++) {
            const double w = I.M[4 * a] * p[0] + I.M[4 * a + 1] * p[1] + I.M[4 * a + 2] * p[2] + I.M[4 * a + 3];
            mn[a] = std::min(mn[a], w); mx[a] = std::max(mx[a], w);
          }
        }
        fjgpu::PrimRef r;
        for (int a = 0; a < 3; a++) {
          // the exact test runs in object space: its hit point, carried to the world by o + t d, lies on the image of the triangle up to the
          // roundings of M v and M^-1 (o, d) -- a relative 1e-9 (and 1e-12 absolute) covers them many times over
          if (!std::isfinite(mn[a]) || !std::isfinite(mx[a])) { bad[t] = 1; mn[a] = mx[a] = 0; }
          const double pad = 1e-9 * (std::fabs(mn[a]) + std::fabs(mx[a])) + 1e-12;
          r.bmin[a] = fjgpu::RoundDown2(mn[a] - pad);
          r.bmax[a] = fjgpu::RoundUp2(mx[a] + pad);
          r.c[a] = (float) (.5 * (mn[a] + mx[a]));
        }
        r.id = (uint32_t) (base + (size_t) k);
        prs[base + (size_t) k] = r;
        DFlatRef fr;
        for (int q = 0; q < 9; q++) fr.v[q] = ps.tri_verts32[(size_t) k * 9 + q];
        fr.inst_ord = ((uint32_t) inst << 8) | (uint32_t) pos;
        fr.pid = ps.prim_ids[k];
        fr.pad = 0;
        src[base + (size_t) k] = fr;
      }
    });
    for (auto &t : th) t.join();
    for (char b : bad) if (b) finite = false;
  }
  if (!finite) return false;
  for (const fjgpu::PrimRef &r : prs)
    for (int a = 0; a < 3; a++) { gmn[a] = std::min(gmn[a], (double) r.bmin[a]); gmx[a] = std::max(gmx[a], (double) r.bmax[a]); }
  F.tree.type = FJ_PRIMSET_MESH; F.tree.device_build = false; F.tree.f32_exact = false; F.tree.mesh = nullptr; F.tree.curve = nullptr;
  {
    // (experiment knobs like the mesh builder's: leaf size / SAH cost of a node step in candidate tests)
    int max_leaf = FJ_MAX_LEAF_PRIMS;
    float trav_cost = .7f;           // (a candidate costs three node steps here -- record, M^-1, transform, test: C4 frame 611 / 606 / 605 / 690 ms at 1.2 / .4 / .7 / 2.5)
    if (const char *e = getenv("FJGPU_FLAT_MAX_LEAF")) max_leaf = atoi(e);
    if (const char *e = getenv("FJGPU_FLAT_TRAV_COST")) trav_cost = (float) atof(e);
    fjgpu::BuildBlas(&F.tree, prs, max_leaf, trav_cost);
  }
  F.refs.resize(src.size());
  for (size_t sl = 0; sl < src.size(); sl++) F.refs[sl] = src[F.tree.prim_ids[sl]];
  for (int a = 0; a < 3; a++) {
    if (total == 0) { gmn[a] = 0; gmx[a] = 1; }
    const double pad = 1e-4 * std::max(1., gmx[a] - gmn[a]);
    F.grid[a] = gmn[a] - pad;
    F.grid[3 + a] = std::max(1e-300, (gmx[a] - gmn[a] + 2 * pad) / 65535. * (1 + 1e-9));
    F.tree.bounds[a] = gmn[a] - pad; F.tree.bounds[3 + a] = gmx[a] + pad;
  }
  return true;
}
// every group of the scene, or none
static bool build_flat_groups(const fjgpu::HostScene &hs, std::vector<HostFlat> *out)
{
  out->clear();
  if (hs.groups.empty() || !hs.xforms.empty()) return false;
  std::vector<HostFlat> flats(hs.groups.size());
  size_t max_tris = (size_t) FJ_FLAT_MAX_TRIS;
  if (const char *e = getenv("FJGPU_FLAT_MAX_TRIS_LOG2")) max_tris = (size_t) 1 << std::max(1, std::min(27, atoi(e)));
  for (size_t g = 0; g < hs.groups.size(); g++) if (!build_flat_group(hs, g, max_tris, &flats[g])) return false;
  out->swap(flats);
  return true;
}

static long g_ray_sort = -1;       // "ray_sort": grid bits per axis of the ray-queue sort (fjgpu_raysort.hip); 0 = off, -1 = by scene
long fjgpu::g_ray_sort_min = FJ_RAY_SORT_MIN;   // "ray_sort_min": smaller launches keep queue order
static long g_device_tlas = 1;     // "device_tlas": the instance level of every group is built on the device (fjgpu_tlas.hip)
static long g_tlas_verify = 0;     // "tlas_verify": ... and compared node for node with the host's build (scene creation fails on a difference)
static long g_split_shadow = 1;    // "split_shadow": shadow rays into groups of several instances are queued once per candidate instance
                                   // (C2: any-hit walk 91 -> 54 ms, the light loop that now lists every candidate 18 -> 41 ms, frame 134 -> 121)
long fjgpu::g_compact_squeue = 1;  // "compact_squeue": 56-byte shadow-queue records (DShadowRayC) where the walks can rebuild direction and distance
static long g_flat_groups = 1;     // "flat_groups": scenes with incoherent closest-hit rays whose groups hold only small static meshes walk ONE world-space tree per group
static long g_curve_anyhit = 1;    // "curve_anyhit": curve scenes whose occluders are all opaque walk their shadow rays with k_shadow_anyhit_curves
static long g_inst_lds = 1;        // "inst_lds": the walks keep the instance level of scenes that fit their budget in LDS (DInstEntry)
static long g_batch_tiles = 0;     // "batch_tiles": default of the per-scene option of that name for scenes created from now on (0 = by memory)
static long g_device_build = -1;   // "device_build": BLAS of meshes built on the GPU (fjgpu_lbvh.hip): 1 = clustering, 2 = radix tree; 0 = on the host; -1 = not set
static long g_treelet_passes = 0;  // "blas_treelet_passes": 0 .. 8 passes of SAH treelet restructuring over a device-built BLAS (0 = off: today's trees)
static long g_multi_exchange = 0;  // "multi_exchange": how fjgpu_render_frame_multi moves the devices' tile slabs: 0 one hipMemcpyPeer each, 1 RCCL grouped send / recv
long fjgpu::g_spec_walk = 1;       // "speculative_walk": the next recursion level's closest-hit walk is enqueued before the host has read how many rays it has (the walk reads the count itself)
long fjgpu::g_cold_start = 1;      // "cold_start": a scene's first render call uses batches of FJ_COLD_BATCH_SAMPLES samples (a small arena: a fast first frame)
#ifndef FJ_COLD_BATCH_SAMPLES
#define FJ_COLD_BATCH_SAMPLES ((size_t) 16 << 20)
#endif
long fjgpu::g_cold_batch_samples = (long) FJ_COLD_BATCH_SAMPLES;      // "cold_batch_samples": ... of this many samples (0 = the default, 16 M)
// "single_frame_build": scenes created while it is on render ONE frame (SiRenderScene): where device_build is not set they build on the GPU.
// PER THREAD (the caller switches it on around ITS fjgpu_scene_create call, which reads it on the same thread): a scene created at the same time on
// another thread is not touched by the toggle.
static thread_local long g_single_frame = 0;
// (the fjgpu:: ones above are those the frame loop reads: declared in fjgpu_scene.h)
using fjgpu::g_ray_sort_min; using fjgpu::g_compact_squeue; using fjgpu::g_spec_walk; using fjgpu::g_cold_start; using fjgpu::g_cold_batch_samples;

extern "C" {

int fjgpu_global_option(const char *name, long value)
{
  if (!name) return fail(FJGPU_EINVAL, "bad option call");
  if (std::string(name) == "ray_sort") { g_ray_sort = value < -1 ? -1 : (value > 9 ? 9 : value); return 0; }
  if (std::string(name) == "ray_sort_min") { g_ray_sort_min = value < 1 ? 1 : value; return 0; }
  if (std::string(name) == "device_tlas") { g_device_tlas = value != 0; return 0; }
  if (std::string(name) == "tlas_verify") { g_tlas_verify = value != 0; return 0; }
  if (std::string(name) == "split_shadow") { g_split_shadow = value != 0; return 0; }
  if (std::string(name) == "inst_lds") { g_inst_lds = value != 0; return 0; }
  if (std::string(name) == "curve_anyhit") { g_curve_anyhit = value != 0; return 0; }
  if (std::string(name) == "flat_groups") { g_flat_groups = value < 0 ? 0 : (value > 2 ? 2 : value); return 0; }
  if (std::string(name) == "compact_squeue") { g_compact_squeue = value != 0; return 0; }
  if (std::string(name) == "batch_tiles") { g_batch_tiles = value < 0 ? 0 : value; return 0; }
  if (std::string(name) == "device_build") { g_device_build = value < 0 ? -1 : (value > 2 ? 2 : value); return 0; }
  if (std::string(name) == "blas_treelet_passes") { g_treelet_passes = value < 0 ? 0 : (value > 8 ? 8 : value); return 0; }
  if (std::string(name) == "single_frame_build") { g_single_frame = value != 0; return 0; }
  if (std::string(name) == "speculative_walk") { g_spec_walk = value != 0; return 0; }
  if (std::string(name) == "anyhit_filter_off") { set_anyhit_filter_off(value); return 0; }
  if (std::string(name) == "cold_start") { g_cold_start = value != 0; return 0; }
  if (std::string(name) == "cold_batch_samples") { g_cold_batch_samples = value > 0 ? value : (long) FJ_COLD_BATCH_SAMPLES; return 0; }
  if (std::string(name) == "multi_exchange") { if (value < 0 || value > 1) return fail(FJGPU_EINVAL, "multi_exchange: 0 peer copies, 1 RCCL send / recv"); g_multi_exchange = value; return 0; }
  return fail(FJGPU_EINVAL, std::string("unknown global option ") + name);
}

const char *fjgpu_last_error(void) { return t_last_error.c_str(); }

int fjgpu_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int fjgpu_tile_count(const fj_render_desc *render)
{
  if (!render) return 0;
  if (const char *why = bad_tiling(render)) { (void) fail(FJGPU_EINVAL, why); return 0; }
  std::vector<fjgpu::TileRect> t;
  fjgpu::GenerateTiles(*render, &t);
  return (int) t.size();
}

int fjgpu_tile_rect(const fj_render_desc *render, int tile_id, int32_t rect[4])
{
  if (!render || !rect) return fail(FJGPU_EINVAL, "null argument");
  if (const char *why = bad_tiling(render)) return fail(FJGPU_EINVAL, why);
  std::vector<fjgpu::TileRect> t;
  fjgpu::GenerateTiles(*render, &t);
  if (tile_id < 0 || tile_id >= (int) t.size()) return FJGPU_EINVAL;
  rect[0] = t[tile_id].xmin; rect[1] = t[tile_id].ymin; rect[2] = t[tile_id].xmax; rect[3] = t[tile_id].ymax;
  return 0;
}

}  // extern "C"

// per-light hull cones (fjgpu_light_hull.h): one record per (single-instance group whose instance is a static mesh, point light sample), from
// the world images of ALL vertices of the mesh -- two passes over them per light, on worker threads.  Time-sampled transforms, vertex
// velocities, curve sets, groups of several instances, area lights and dome samples get none (the box cones exclude the same cases).
// hulls: rows of one record per light sample; rows[g]: the row of group g or -1.  cone_reach[g]: the reach of the group's box cones or -1.
static void build_light_hull_rows(const fjgpu::HostScene &hs, const std::vector<double> &cone_reach, std::vector<DLightCone> &hulls,
    std::vector<int32_t> &rows, int *n_rows, int *n_records)
{
  const size_t nl = hs.light_samples.size();
  rows.assign(hs.groups.size(), -1);
  hulls.clear();
  if (!hs.area_lights.empty()) return;      // (a scene with a rectangle or sphere light runs the light loop's general instantiation: nothing would read the table)
  for (size_t g = 0; g < hs.groups.size() && nl; g++) {
    if (hs.groups[g].n_instances != 1) continue;
    const DInstance &I = hs.instances[hs.group_members[hs.group_member_first[g]]];
    const fjgpu::HostPrimSet &ps = hs.primsets[I.primset];
    if (I.xform >= 0 || ps.type != FJ_PRIMSET_MESH || !ps.mesh || ps.mesh->velocity || ps.mesh->n_points <= 0) continue;
    std::vector<size_t> lights;                 // the samples with a fixed position near enough to have a cone at all
    for (size_t l = 0; l < nl; l++) if (hs.light_samples[l].type == FJ_POINT_LIGHT) lights.push_back(l);
    if (lights.empty()) continue;
    const size_t nv = (size_t) ps.mesh->n_points, nk = lights.size();
    // vertex ranges of a fixed size (the sums and maxima do not depend on the number of threads), claimed by the workers
    const size_t chunk = 16384, nchunks = (nv + chunk - 1) / chunk;
    // (at most 16 workers, fewer where OMP_NUM_THREADS says so: a process is often given a part of the machine hardware_concurrency() reports)
    size_t workers = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char *omp = getenv("OMP_NUM_THREADS")) { const long v = atol(omp); if (v >= 1) workers = std::min<size_t>(workers, (size_t) v); }
    const unsigned hc = (unsigned) std::max<size_t>(1, std::min(workers, nchunks));
    auto over_chunks = [&](const std::function<void(size_t)> &fn) {
      std::atomic<size_t> next(0);
      std::vector<std::thread> th;
      for (unsigned t = 0; t < hc; t++) th.emplace_back([&]() { for (size_t c; (c = next.fetch_add(1)) < nchunks;) fn(c); });
      for (auto &t : th) t.join();
    };
    std::vector<double> W(3 * nv), csum(3 * nchunks, 0.);
    over_chunks([&](size_t c) {
      double s[3] = {0., 0., 0.};
      for (size_t i = c * chunk; i < std::min(nv, (c + 1) * chunk); i++) {
        light_hull_world(I.M, ps.mesh->P + 3 * i, &W[3 * i]);
        for (int k = 0; k < 3; k++) s[k] += W[3 * i + k];
      }
      for (int k = 0; k < 3; k++) csum[3 * c + k] = s[k];
    });
    double ctr[3] = {0., 0., 0.};
    for (size_t c = 0; c < nchunks; c++) for (int k = 0; k < 3; k++) ctr[k] += csum[3 * c + k];
    for (int k = 0; k < 3; k++) ctr[k] /= (double) nv;
    std::vector<LightHullAcc> acc(nk), part(nk * nchunks);
    for (size_t k = 0; k < nk; k++) light_hull_frame(hs.light_samples[lights[k]].P, ctr, &acc[k]);
    over_chunks([&](size_t c) {
      for (size_t k = 0; k < nk; k++) {
        LightHullAcc A = acc[k];
        for (size_t i = c * chunk; i < std::min(nv, (c + 1) * chunk) && A.ok; i++) light_hull_add(&A, &W[3 * i]);
        part[k * nchunks + c] = A;
      }
    });
    for (size_t k = 0; k < nk; k++) for (size_t c = 0; c < nchunks; c++) light_hull_merge(&acc[k], &part[k * nchunks + c]);
    const size_t at = hulls.size();
    hulls.resize(at + nl);
    std::memset(&hulls[at], 0, nl * sizeof(DLightCone));
    std::vector<char> open(nk, 1);
    std::vector<uint32_t> bad(nk * nchunks);
    for (int round = 0; round <= FJ_LH_WIDENINGS; round++) {
      bool any = false;
      for (size_t k = 0; k < nk; k++) if (open[k]) { if (light_hull_finish(&acc[k], hs.groups[g].sbounds, &hulls[at + lights[k]])) any = true; else open[k] = 0; }
      if (!any) break;
      // the verify pass: the finished normals against every vertex
      over_chunks([&](size_t c) {
        for (size_t k = 0; k < nk; k++) {
          uint32_t b = 0;
          if (open[k]) for (size_t i = c * chunk; i < std::min(nv, (c + 1) * chunk); i++) b |= light_hull_verify(&hulls[at + lights[k]], acc[k].Pl, &W[3 * i]);
          bad[k * nchunks + c] = b;
        }
      });
      for (size_t k = 0; k < nk; k++) {
        if (!open[k]) continue;
        uint32_t b = 0;
        for (size_t c = 0; c < nchunks; c++) b |= bad[k * nchunks + c];
        if (!b) open[k] = 0;                                 // verified: the record stands
        else light_hull_widen(&acc[k], b);
      }
    }
    for (size_t k = 0; k < nk; k++) if (open[k]) std::memset(&hulls[at + lights[k]], 0, sizeof(DLightCone));      // still failing after the last widening
    int built = 0;
    double reach = 1e300;
    for (size_t l = 0; l < nl; l++) if (hulls[at + l].count > 0) { built++; reach = std::min(reach, hulls[at + l].reach); }
    if (!built) { hulls.resize(at); continue; }
    // (read once per wave iteration: the row's smallest -- and no larger than the reach of the group's box cones: the light loop keeps one
    // set of lanes within reach for both tables)
    if (g < cone_reach.size() && cone_reach[g] >= 0) reach = std::min(reach, cone_reach[g]);
    for (size_t l = 0; l < nl; l++) hulls[at + l].reach = reach;
    rows[g] = (int32_t) (at / nl);
    (*n_rows)++; *n_records += built;
  }
}

// the reach of group g's row of box cones as upload_scene builds it (the smallest of its records' reaches), or -1: no row
static double box_cone_row_reach(const fjgpu::HostScene &hs, size_t g)
{
  if (hs.groups[g].n_instances != 1) return -1.;
  double reach = 1e300;
  int built = 0;
  for (const DLightSample &LS : hs.light_samples) {
    DLightCone C;
    if ((LS.type == FJ_POINT_LIGHT || LS.type == FJ_DOME_LIGHT) && light_cone_build(LS.P, hs.groups[g].sbounds, &C) > 0) { built++; reach = std::min(reach, C.reach); }
  }
  return built ? reach : -1.;
}

// Upload a built host scene to one device (fjgpu_scene_create = build + upload; the multi-device
// entry builds once and uploads to every device).
static int upload_scene(const fj_scene_desc *desc, fjgpu::HostScene &hs, int device, fjgpu_scene **out)
{
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(FJGPU_ENODEV, "no HIP device visible: the fjgpu core has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(FJGPU_EINVAL, "device index out of range");
  HIP_TRY(hipSetDevice(device));

  const auto t_up0 = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (getenv("FJGPU_VERBOSE")) { (void) hipDeviceSynchronize(); fprintf(stderr, "fjgpu: upload: %-28s at %.3f s\n", what,
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t_up0).count()); }
  };
  std::unique_ptr<fjgpu_scene> sc(new fjgpu_scene());
  sc->device = device;
  sc->batch_tiles = g_batch_tiles;
  sc->count_events = 0;     // traversal event counters are opt-in ("count_nodes"): they cost registers
  sc->count_all_shadow = 1;
  sc->work_samples = sc->work_rays = 0;
  sc->tab_len = 0;
  sc->overlap = 2;
  sc->shadow_stream = nullptr;
  for (int k = 0; k < FJ_LREC_BUFS; k++) { sc->ev_shadow_done[k] = nullptr; sc->d_lrecs[k] = nullptr; sc->d_lhair[k] = nullptr; }
  if (getenv("FJGPU_EARLY_SHADOW")) sc->early_shadow = atoi(getenv("FJGPU_EARLY_SHADOW"));
  if (const char *e = getenv("FJGPU_OVERLAP")) sc->overlap = std::max(0, std::min(2, atoi(e)));
  DeviceBuffers &M = sc->mem;
  int e = 0;

  std::vector<DPrimSet> dps(hs.primsets.size());
  for (size_t i = 0; i < hs.primsets.size(); i++) {
    const fjgpu::HostPrimSet &h = hs.primsets[i];
    DPrimSet &d = dps[i];
    std::memset(&d, 0, sizeof(d));
    d.type = h.type;
    d.root = h.root;
    d.n_prims = h.n_prims;
    std::memcpy(d.bounds, h.bounds, sizeof(d.bounds));
    for (int k = 0; k < 3; k++) { d.grid_cell[k] = h.grid_cell[k]; d.grid_n[k] = h.grid_n[k]; }
    if (!h.device_build) {
      e |= M.upload(h.nodes.data(), h.nodes.size(), &d.nodes);
      e |= M.upload(h.prim_ids.data(), h.prim_ids.size(), &d.prim_ids);
    }
    if (h.type == FJ_PRIMSET_MESH) {
      const fj_mesh_desc &m = *h.mesh;
      e |= M.upload(m.velocity, m.velocity ? (size_t) m.n_points * 3 : 0, &d.velocity);
      e |= M.upload(m.P, (size_t) m.n_points * 3, &d.P);
      e |= M.upload(m.N, m.N ? (size_t) m.n_points * 3 : 0, &d.N);
      e |= M.upload(m.vertex_N, m.vertex_N ? (size_t) m.n_faces * 9 : 0, &d.vN);
      e |= M.upload(m.uv, m.uv ? (size_t) m.n_points * 2 : 0, &d.uv);
      e |= M.upload(m.indices, (size_t) m.n_faces * 3, &d.indices);
      e |= M.upload(m.face_group, m.face_group ? (size_t) m.n_faces : 0, &d.face_group);
      if (h.device_build) {
        // BLAS on the device: Morton sort, clustering (or radix tree + fit), collapse, triangle gather
        if (e) return fail(FJGPU_ENOMEM, "device allocation / upload failed while creating the scene");
        const auto tb0 = std::chrono::steady_clock::now();
        LbvhOut lo;
        std::string lerr;
        if (LbvhBuildMesh(d.P, d.velocity, d.indices, m.n_faces, m.n_points, h.bounds, h.f32_exact, hs.device_build_quality, hs.device_build_treelet_passes, &lo, &lerr))
          return fail(FJGPU_ENODEV, lerr);
        for (void *p : {(void *) lo.nodes, (void *) lo.prim_ids, (void *) lo.tri_verts, (void *) lo.tri_verts32, (void *) lo.tri_vel})
          if (p) M.ptrs.push_back(p);
        d.nodes = lo.nodes; d.prim_ids = lo.prim_ids; d.root = lo.root;
        d.tri_verts = lo.tri_verts; d.tri_verts32 = lo.tri_verts32; d.tri_vel = lo.tri_vel;
        hs.primsets[i].stack_need = lo.stack_need;
        sc->blas_treelet_passes += lo.treelet_passes; sc->blas_treelets_changed += lo.treelets_changed;
        sc->blas_sah_cost_initial += lo.sah_cost_initial; sc->blas_sah_cost += lo.sah_cost;
        hs.primsets[i].nodes.n = lo.n_nodes;
        if (lo.tri_verts32) hs.primsets[i].tri_verts32.resize(1);      // (layout flags read below)
        if (lo.tri_vel) hs.primsets[i].tri_vel.resize(1);
        if (getenv("FJGPU_VERBOSE") && m.n_faces > 100000)
          fprintf(stderr, "fjgpu: device BLAS build of %d triangles: %.3f s, %zu wide nodes\n", m.n_faces,
              std::chrono::duration<double>(std::chrono::steady_clock::now() - tb0).count(), lo.n_nodes);
      } else {
        e |= M.upload(h.tri_verts.data(), h.tri_verts.size(), &d.tri_verts);
        e |= M.upload(h.tri_verts32.data(), h.tri_verts32.size(), &d.tri_verts32);
        e |= M.upload(h.tri_vel.data(), h.tri_vel.size(), &d.tri_vel);
      }
    } else {
      e |= M.upload(h.curve_cp.data(), h.curve_cp.size(), &d.curve_cp);
      e |= M.upload(h.curve_width.data(), h.curve_width.size(), &d.curve_width);
      e |= M.upload(h.curve_Cd.data(), h.curve_Cd.size(), &d.curve_Cd);
      e |= M.upload(h.curve_depth.data(), h.curve_depth.size(), &d.curve_depth);
      e |= M.upload(h.curve_capsule.data(), h.curve_capsule.size(), &d.curve_capsule);
      e |= M.upload(h.curve_vel.data(), h.curve_vel.size(), &d.curve_vel);
    }
  }
  lap("primitive sets");
  std::vector<DTexture> dtex(desc->n_textures);
  for (int i = 0; i < desc->n_textures; i++) {
    const fj_texture_desc &t = desc->textures[i];
    dtex[i].width = t.width; dtex[i].height = t.height; dtex[i].nchannels = t.nchannels; dtex[i].tilesize = t.tilesize;
    const size_t n = (t.width && t.tiles) ? (size_t) (t.width / t.tilesize) * (t.height / t.tilesize) * t.tilesize * t.tilesize * t.nchannels : 0;
    e |= M.upload(t.tiles, n, &dtex[i].tiles);
    if (!dtex[i].tiles) dtex[i].width = dtex[i].height = 0;
  }
  DScene &S = sc->S;
  std::memset(&S, 0, sizeof(S));
  {
    // quantised node arrays of the lean any-hit walk (DNodeQ): one per mesh, same node indices;
    // grid = 65536^3 cells over the primitive set's padded bounds
    std::vector<std::array<double, 6>> qgrid(dps.size());
    for (size_t i = 0; i < dps.size(); i++) {
      DPrimSet &P = dps[i];
      P.qnodes = nullptr;
      if (P.type != FJ_PRIMSET_MESH || P.n_prims == 0 || e) continue;
      const size_t n_nodes = std::max<size_t>(1, hs.primsets[i].nodes.size());
      for (int a = 0; a < 3; a++) {
        qgrid[i][a] = P.bounds[a];
        qgrid[i][3 + a] = std::max(1e-300, (P.bounds[3 + a] - P.bounds[a]) / 65535. * (1 + 1e-9));
      }
      DNodeQ *q = nullptr;
      if (M.alloc(n_nodes, &q)) { e = 1; continue; }
      if (launch_quantize_nodes(nullptr, P.nodes, (uint32_t) n_nodes, &qgrid[i][0], &qgrid[i][3], q)) e = 1;
      P.qnodes = q;
    }
    // curve sets: the same quantised twin for the closest-hit / general shadow walks of scenes with curve sets (kept out of
    // DPrimSet.qnodes, which the lean any-hit walk's tables read as "a mesh with pre-gathered triangles").  The grid spans the
    // set's bounds widened by 1e-4 of their size (at least 1e-4), so no node box is clamped at the rim.
    std::vector<const DNodeQ *> cq(dps.size(), nullptr);
    for (size_t i = 0; FJ_CURVE_QNODES && FJ_CLOSEST_QNODES && i < dps.size(); i++) {
      const DPrimSet &P = dps[i];
      if (P.type != FJ_PRIMSET_CURVE || P.n_prims == 0 || e) continue;
      const size_t n_nodes = std::max<size_t>(1, hs.primsets[i].nodes.size());
      for (int a = 0; a < 3; a++) {
        const double pad = 1e-4 * std::max(1., P.bounds[3 + a] - P.bounds[a]);
        qgrid[i][a] = P.bounds[a] - pad;
        qgrid[i][3 + a] = std::max(1e-300, (P.bounds[3 + a] - P.bounds[a] + 2 * pad) / 65535. * (1 + 1e-9));
      }
      DNodeQ *q = nullptr;
      if (M.alloc(n_nodes, &q)) { e = 1; continue; }
      if (launch_quantize_nodes(nullptr, P.nodes, (uint32_t) n_nodes, &qgrid[i][0], &qgrid[i][3], q)) e = 1;
      cq[i] = q;
    }
    lap("quantised nodes");
    e |= M.upload(dps.data(), dps.size(), &S.primsets);      // (after the loops above: DPrimSet.qnodes is set)
    {
      // the instance table, each record with a copy of its primitive set's entry data
      std::vector<DInstance> di = hs.instances;
      for (DInstance &I : di) {
        const DPrimSet &P = dps[I.primset];
        std::memcpy(I.pbounds, P.bounds, sizeof(I.pbounds));
        I.pnodes = P.nodes; I.proot = P.root; I.pn_prims = P.n_prims;
        I.pqnodes = P.qnodes ? P.qnodes : cq[I.primset];
        I.sh_indices = P.indices; I.sh_N = P.N; I.sh_vN = P.vN; I.sh_uv = P.uv; I.sh_face_group = P.face_group; I.sh_type = P.type; I.sh_pad = 0;
        for (int k = 0; k < 3; k++) { I.qorigin[k] = qgrid[I.primset][k]; I.qcell[k] = qgrid[I.primset][3 + k]; }
      }
      e |= M.upload(di.data(), di.size(), &S.instances);
      std::vector<DInstEntry> ie(di.size());
      bool any_curves = false, any_motion = !hs.xforms.empty();       // (DScene.has_curves / has_motion, set below)
      for (const auto &ps : hs.primsets) {
        if (ps.type == FJ_PRIMSET_CURVE && ps.n_prims > 0) any_curves = true;
        if (!ps.tri_vel.empty() || !ps.curve_vel.empty()) any_motion = true;
      }
      for (size_t k = 0; k < di.size(); k++) {
        const DInstance &I = di[k];
        DInstEntry &E = ie[k];
        std::memcpy(E.Minv, I.Minv, sizeof(E.Minv));
        std::memcpy(E.pbounds, I.pbounds, sizeof(E.pbounds));
        // tight world box: the eight corners of the primitive set's padded box through M, widened by 1e-7 of its size (+ 1e-9): it must contain
        // every point o + t d of a hit that the object-space test finds
        for (int a = 0; a < 3; a++) { E.tbounds[a] = -INFINITY; E.tbounds[3 + a] = INFINITY; }
        if (I.xform < 0 && I.pn_prims > 0) {
          double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
          for (int c = 0; c < 8; c++) {
            const double p[3] = {I.pbounds[(c & 1) ? 3 : 0], I.pbounds[(c & 2) ? 4 : 1], I.pbounds[(c & 4) ? 5 : 2]};
            for (int a = 0; a < 3; a++) {
              const double w = I.M[4 * a] * p[0] + I.M[4 * a + 1] * p[1] + I.M[4 * a + 2] * p[2] + I.M[4 * a + 3];
              mn[a] = std::min(mn[a], w); mx[a] = std::max(mx[a], w);
            }
          }
          bool finite = true;
          for (int a = 0; a < 3; a++) finite = finite && std::isfinite(mn[a]) && std::isfinite(mx[a]);
          if (finite)
            for (int a = 0; a < 3; a++) {
              const double pad = 1e-7 * (mx[a] - mn[a]) + 1e-7 * std::max(std::fabs(mn[a]), std::fabs(mx[a])) + 1e-9;
              E.tbounds[a] = mn[a] - pad; E.tbounds[3 + a] = mx[a] + pad;
            }
        }
        for (int a = 0; a < 3; a++) { E.qorigin[a] = I.qorigin[a]; E.qcell[a] = I.qcell[a]; }
        const DPrimSet &P = dps[I.primset];
        const bool quantised = FJ_CLOSEST_QNODES && (!any_curves || FJ_CURVE_QNODES) && !any_motion;     // (the instantiations launch_trace_closest picks)
        E.nodes = quantised ? (const void *) I.pqnodes : (const void *) I.pnodes;
        E.ptype = P.type; E.pad = 0;
        E.proot = I.proot; E.pn_prims = I.pn_prims; E.primset = I.primset; E.xform = I.xform;
        E.tri_verts = P.tri_verts; E.tri_verts32 = P.type == FJ_PRIMSET_CURVE ? P.curve_capsule : P.tri_verts32; E.tri_vel = P.tri_vel; E.prim_ids = P.prim_ids;
      }
      e |= M.upload(ie.data(), ie.size(), &S.inst_entries);
    }
    // flat per-instance records of that walk (static mesh instances): node and triangle arrays
    // as 32-bit offsets from the lowest of their addresses
    uintptr_t lo = UINTPTR_MAX, hi = 0;
    auto tris_of = [](const DPrimSet &P) { return (uintptr_t) (P.tri_verts32 ? (const void *) P.tri_verts32 : (const void *) P.tri_verts); };
    for (size_t i = 0; i < dps.size(); i++) {
      const DPrimSet &P = dps[i];
      if (!P.qnodes) continue;
      const uintptr_t pn = (uintptr_t) P.qnodes, pt = tris_of(P);
      lo = std::min(lo, std::min(pn, pt)); hi = std::max(hi, std::max(pn, pt));
    }
    // (hipMalloc returns 256-byte aligned blocks: offsets in units of 128 B span 512 GB)
    bool fits = lo != UINTPTR_MAX && lo % 128 == 0 && (hi - lo) / 128 < 0xffffffffull;
    for (size_t i = 0; i < dps.size(); i++) {
      const DPrimSet &P = dps[i];
      if (P.qnodes && (((uintptr_t) P.qnodes - lo) % 128 != 0 || (tris_of(P) - lo) % 128 != 0)) fits = false;
    }
    // the lean walk reads f32 triangle records only (every PLY mesh): a mesh that needs f64
    // vertices sends the scene's shadow rays through the general walk
    for (const DPrimSet &P : dps) if (P.qnodes && !P.tri_verts32) fits = false;
    S.blas_base = fits ? (const char *) lo : nullptr;
    if (!fits && lo != UINTPTR_MAX && getenv("FJGPU_VERBOSE"))
      fprintf(stderr, "fjgpu: BLAS arrays span %zu bytes from %p: no 32-bit offsets, the general shadow walk is used\n", (size_t) (hi - lo), (void *) lo);
    std::vector<DAnyInst> ai(hs.instances.size());
    for (size_t i = 0; i < hs.instances.size(); i++) {
      const DInstance &I = hs.instances[i];
      const DPrimSet &P = dps[I.primset];
      DAnyInst &a = ai[i];
      std::memset(&a, 0, sizeof(a));
      std::memcpy(a.Minv, I.Minv, sizeof(a.Minv));
      std::memcpy(a.bounds, P.bounds, sizeof(a.bounds));
      a.root = P.root;
      a.n_prims = (P.qnodes && S.blas_base) ? P.n_prims : 0;
      if (a.n_prims) {
        for (int k = 0; k < 3; k++) { a.qorigin[k] = qgrid[I.primset][k]; a.qcell[k] = qgrid[I.primset][3 + k]; }
        a.node_base = (uint32_t) (((uintptr_t) P.qnodes - lo) / 128);
        a.tri_base = (uint32_t) ((tris_of(P) - lo) / 128);
        a.tris_f32 = P.tri_verts32 ? 1 : 0;
        double bm = 0;
        for (int k = 0; k < 6; k++) bm = std::max(bm, std::fabs(P.bounds[k]));
        a.fbound = std::nextafter((float) bm, INFINITY);
      }
    }
    e |= M.upload(ai.data(), ai.size(), &S.any_insts);
  }
  if (g_device_tlas && e == 0 && !hs.groups.empty()) {
    // instance level on the device, from the instance table just uploaded
    std::vector<int> mcount(hs.groups.size()), nfirst, ncount;
    for (size_t g = 0; g < hs.groups.size(); g++) mcount[g] = hs.groups[g].n_instances;
    DTNode *d_nodes = nullptr;
    std::string terr;
    if (TlasBuildDevice(S.instances, hs.group_members, hs.group_member_first, mcount, &nfirst, &ncount, &d_nodes, &terr))
      return fail(FJGPU_ENODEV, terr);
    M.ptrs.push_back(d_nodes);
    size_t total = 0;
    for (int c : ncount) total += (size_t) c;
    if (g_tlas_verify) {
      std::vector<DTNode> got(total);
      HIP_TRY(hipMemcpy(got.data(), d_nodes, total * sizeof(DTNode), hipMemcpyDeviceToHost));
      bool same = total == hs.group_nodes.size();
      for (size_t g = 0; same && g < hs.groups.size(); g++) same = nfirst[g] == hs.groups[g].first && ncount[g] == hs.groups[g].count;
      if (same && total) same = std::memcmp(got.data(), hs.group_nodes.data(), total * sizeof(DTNode)) == 0;
      if (!same) return fail(FJGPU_ENODEV, "device TLAS build differs from the host's build");
    }
    std::vector<DGroup> groups = hs.groups;
    for (size_t g = 0; g < groups.size(); g++) { groups[g].first = nfirst[g]; groups[g].count = ncount[g]; }
    e |= M.upload(groups.data(), groups.size(), &S.groups);
    S.group_nodes = d_nodes;
    S.n_group_nodes = (int32_t) total;
  } else {
    e |= M.upload(hs.groups.data(), hs.groups.size(), &S.groups);
    e |= M.upload(hs.group_nodes.data(), hs.group_nodes.size(), &S.group_nodes);
    S.n_group_nodes = (int32_t) hs.group_nodes.size();
  }
  static_assert(sizeof(DInstEntry) == 8 * FJ_INST_LDS_ENTRY_WORDS && sizeof(DTNode) == 56 && sizeof(DGroup) == 64, "LDS copy of the instance level");
  S.curve_anyhit = (g_curve_anyhit && !getenv("FJGPU_NO_CURVE_ANYHIT")) ? 1 : 0;
  S.inst_lds = (g_inst_lds && !getenv("FJGPU_NO_INST_LDS")) ? 1 : 0;         // (each launcher checks the scene against its kernel's budget)
  e |= M.upload(hs.shaders.data(), hs.shaders.size(), &S.shaders);
  e |= M.upload(hs.xforms.data(), hs.xforms.size(), &S.xforms);
  S.cam_xform = nullptr;
  if (!hs.cam_static) e |= M.upload(&hs.cam_xform, 1, &S.cam_xform);
  S.has_motion = hs.xforms.empty() ? 0 : 1;
  for (const auto &ps : hs.primsets) if (!ps.tri_vel.empty() || !ps.curve_vel.empty()) S.has_motion = 1;   // vertex velocities need the ray's time too
  // shadow rays start at objects whose shader gathers light (SlIlluminance: plastic, hair) and go to
  // that object's shadow target group
  S.multi_shadow_groups = 0;
  for (const DInstance &I : hs.instances) {
    bool gathers = false;
    for (int k = 0; k < I.n_shaders; k++)
      if (I.shaders[k] >= 0 && (hs.shaders[I.shaders[k]].type == FJ_SHADER_PLASTIC || hs.shaders[I.shaders[k]].type == FJ_SHADER_HAIR)) gathers = true;
    if (gathers && I.shadow_target >= 0 && I.shadow_target < (int) hs.groups.size() && hs.groups[I.shadow_target].n_instances > 1)
      S.multi_shadow_groups = 1;
  }
  S.time_tab = nullptr; S.time_start = 0; S.time_end = 0;     // set per render call
  S.lrec_hair = nullptr;
  e |= M.upload(dtex.data(), dtex.size(), &S.textures);
  e |= M.upload(hs.light_samples.data(), hs.light_samples.size(), &S.light_samples);
  e |= M.upload(hs.area_lights.data(), hs.area_lights.size(), &S.area_lights);
  // per-light shadow cones (fjgpu_light_cone.h): one record per (single-instance group, light sample) whose position the light loop uses as it
  // stands -- point and dome samples; grid and sphere lights draw theirs per shading event.  Lights and instance boxes are fixed for the scene's life.
  S.light_cones = nullptr; S.cone_rows = nullptr;
  std::vector<double> cone_reach;        // per group: the reach of its row of box cones, -1: no row
  {
    const size_t nl = hs.light_samples.size();
    std::vector<int32_t> rows(hs.groups.size(), -1);
    std::vector<DLightCone> cones;
    cone_reach.assign(hs.groups.size(), -1.);
    for (size_t g = 0; g < hs.groups.size() && nl; g++) {
      if (hs.groups[g].n_instances != 1) continue;
      const size_t at = cones.size();
      cones.resize(at + nl);
      int built = 0;
      double reach = 1e300;
      for (size_t l = 0; l < nl; l++) {
        DLightCone &C = cones[at + l];
        const DLightSample &LS = hs.light_samples[l];
        if (LS.type == FJ_POINT_LIGHT || LS.type == FJ_DOME_LIGHT) light_cone_build(LS.P, hs.groups[g].sbounds, &C);
        else std::memset(&C, 0, sizeof(C));
        if (C.count > 0) { built++; reach = std::min(reach, C.reach); }
      }
      if (!built) { cones.resize(at); continue; }
      for (size_t l = 0; l < nl; l++) cones[at + l].reach = reach;       // (read once per wave iteration: the row's smallest)
      rows[g] = (int32_t) (at / nl);
      cone_reach[g] = reach;
      sc->cone_rows++; sc->cone_records += built;
    }
    if (!cones.empty()) {
      e |= M.upload(cones.data(), cones.size(), &S.light_cones);
      e |= M.upload(rows.data(), rows.size(), &S.cone_rows);
    }
  }
  // per-light hull cones: the second table (build_light_hull_rows above)
  S.light_hulls = nullptr; S.hull_rows = nullptr;
  {
    std::vector<int32_t> rows;
    std::vector<DLightCone> hulls;
    build_light_hull_rows(hs, cone_reach, hulls, rows, &sc->hull_rows, &sc->hull_records);
    if (!hulls.empty()) {
      e |= M.upload(hulls.data(), hulls.size(), &S.light_hulls);
      e |= M.upload(rows.data(), rows.size(), &S.hull_rows);
    }
  }
  S.has_area = hs.area_lights.empty() ? 0 : 1;
  if (e) return fail(FJGPU_ENOMEM, "device allocation / upload failed while creating the scene");
  S.n_light_samples = (int) hs.light_samples.size();
  S.n_instances = (int) hs.instances.size();
  S.n_groups = (int) hs.groups.size();
  S.n_primsets = (int) hs.primsets.size();
  // FLAT groups: one world-space culling tree per group for the closest-hit walk of scenes with incoherent rays (fjgpu_dev_flat.h)
  int flat_stack_need = 0;
  S.flats = nullptr;
  {
    bool incoherent = false;         // (the rule of DScene.incoherent_rays below: two children per hit, or diffuse bounces)
    for (int i = 0; i < desc->n_shaders; i++) {
      const fj_shader_desc &sh = desc->shaders[i];
      auto lum = [](const float *c) { return .298912 * c[0] + .586611 * c[1] + .114478 * c[2] > 0.; };
      if (sh.type == FJ_SHADER_GLASS) incoherent = true;
      if (sh.type == FJ_SHADER_PATHTRACING && (lum(sh.diffuse) || (int) lum(sh.reflect) + (int) lum(sh.refract) >= 2)) incoherent = true;
    }
    std::vector<HostFlat> hf;
    // k_trace_closest_flat keeps M^-1 of every instance in its blocks' LDS (FJ_FLAT_LDS_INSTS of them; until round 5 it shared the phased walk's
    // copy of the whole instance level and its budget of 16 instances, while build_flat_group admits 32 per group: ADVICE round 4).  ONE decision,
    // made here: a scene beyond the budget, or with the inst_lds option off, builds no flat trees, S.flats stays null, and ray_sort_bits / the
    // closest_kernel query / the launcher all follow it.
    const bool flat_fits = S.inst_lds && S.n_instances <= FJ_FLAT_LDS_INSTS;
    // (option "flat_groups" 2 / FJGPU_FLAT_ALL: scenes with coherent closest-hit rays as well)
    const bool flat_wanted = incoherent || g_flat_groups >= 2 || getenv("FJGPU_FLAT_ALL");
    if (flat_wanted && flat_fits && g_flat_groups && !getenv("FJGPU_NO_FLAT") && FJ_CLOSEST_QNODES && build_flat_groups(hs, &hf)) {
      std::vector<DFlat> df(hf.size());
      for (size_t g = 0; g < hf.size() && !e; g++) {
        HostFlat &F = hf[g];
        DFlat &D = df[g];
        std::memset(&D, 0, sizeof(D));
        const DNode *d_nodes = nullptr;
        const size_t n_nodes = std::max<size_t>(1, F.tree.nodes.size());
        e |= M.upload(F.tree.nodes.data(), n_nodes, &d_nodes);
        DNodeQ *q = nullptr;
        if (!e && M.alloc(n_nodes, &q)) e = 1;
        if (!e && launch_quantize_nodes(nullptr, d_nodes, (uint32_t) n_nodes, &F.grid[0], &F.grid[3], q)) e = 1;
        D.nodes = q;
        e |= M.upload(F.refs.data(), F.refs.size(), &D.refs);
        e |= M.upload(F.refbox.data(), F.refbox.size(), &D.refbox);
        for (int a = 0; a < 3; a++) { D.qorigin[a] = F.grid[a]; D.qcell[a] = F.grid[3 + a]; }
        D.root = F.tree.root; D.n_inst = (int32_t) (F.refbox.size() / 6); D.n_prims = F.tree.n_prims;
        flat_stack_need = std::max(flat_stack_need, F.tree.stack_need);
      }
      if (!e) e |= M.upload(df.data(), df.size(), &S.flats);
      if (e) S.flats = nullptr;
      lap("flat groups");
    }
  }
  // traversal stack: entries beyond the LDS part live in a global overflow area sized for
  // the worst tree of the scene (usually none: stack_need <= FJ_STACK_LDS)
  {
    int need = S.flats ? flat_stack_need : 0;
    for (const auto &ps : hs.primsets) need = std::max(need, ps.stack_need);
    S.stack_overflow = nullptr;
    S.stack_overflow_shadow = nullptr;
    // (scenes with curve sets run the kernels that keep FJ_STACK_LDS_CURVES entries in LDS)
    bool any_curves = false;
    for (const auto &ps : hs.primsets) if (ps.type == FJ_PRIMSET_CURVE && ps.n_prims > 0) any_curves = true;
    (void) any_curves;
    const int lds_entries = FJ_STACK_LDS_MIN;      // the kernel with the fewest LDS entries decides
    if (need > lds_entries) {
      const size_t entries = (size_t) (need - lds_entries) * persistent_threads();
      if (M.alloc(entries, &S.stack_overflow) || M.alloc(entries, &S.stack_overflow_shadow)) return fail(FJGPU_ENOMEM, "device allocation failed for the traversal stack overflow area");
    }
    sc->stack_need = need;
    sc->tri_record_bytes = 36; sc->blas_nodes = 0;
    for (const auto &ps : hs.primsets) {
      sc->blas_nodes += ps.nodes.size();
      if (ps.type == FJ_PRIMSET_MESH && ps.n_prims > 0 && ps.tri_verts32.empty()) sc->tri_record_bytes = 72;
    }
    if (getenv("FJGPU_VERBOSE"))
      for (const auto &ps : hs.primsets)
        fprintf(stderr, "fjgpu: primset type %d prims %d nodes %zu binary depth %d stack need %d\n", ps.type, ps.n_prims,
            ps.nodes.size(), ps.max_depth, ps.stack_need);
  }
  S.has_curves = 0;
  S.all_opaque = 1;
  for (const auto &g : hs.groups) if (!g.all_opaque) S.all_opaque = 0;
  S.has_hair = 0;
  for (int i = 0; i < desc->n_shaders; i++) if (desc->shaders[i].type == FJ_SHADER_HAIR) S.has_hair = 1;
  for (const auto &ps : hs.primsets) if (ps.type == FJ_PRIMSET_CURVE && ps.n_prims > 0) S.has_curves = 1;
  S.target_group = hs.target_group;
  std::memcpy(S.cam_M, hs.cam_M, sizeof(S.cam_M));
  S.cam_znear = hs.cam_znear;
  S.cam_zfar = hs.cam_zfar;
  sc->cam_fov = hs.cam_fov;
  sc->camera = desc->camera;
  sc->n_light_samples = S.n_light_samples;
  sc->max_children = 0;
  sc->uses_sample_uid = S.has_motion || S.cam_xform != nullptr || S.has_area;
  sc->bounce_diffuse = sc->bounce_reflect = sc->bounce_refract = false;
  for (int i = 0; i < desc->n_shaders; i++) {
    const fj_shader_desc &sh = desc->shaders[i];
    if (sh.type == FJ_SHADER_PATHTRACING) sc->uses_sample_uid = true;
    if (sh.type == FJ_SHADER_GLASS || sh.type == FJ_SHADER_PATHTRACING) sc->has_filter_rays = true;     // (refraction children may carry a filter colour)
    auto lum = [](const float *c) { return .298912 * c[0] + .586611 * c[1] + .114478 * c[2] > 0.; };
    int k = 0;
    if (sh.type == FJ_SHADER_PLASTIC) { k = sh.do_reflect ? 1 : 0; if (k) sc->bounce_reflect = true; }
    else if (sh.type == FJ_SHADER_GLASS) { k = 2; sc->bounce_reflect = sc->bounce_refract = true; }
    else if (sh.type == FJ_SHADER_PATHTRACING) {
      k = (int) lum(sh.diffuse) + (int) lum(sh.reflect) + (int) lum(sh.refract);
      if (lum(sh.diffuse)) sc->bounce_diffuse = true;
      if (lum(sh.reflect)) sc->bounce_reflect = true;
      if (lum(sh.refract)) sc->bounce_refract = true;
    }
    sc->max_children = std::max(sc->max_children, k);
  }
  S.incoherent_rays = (sc->max_children >= 2 || sc->bounce_diffuse) ? 1 : 0;
  if (const char *e = getenv("FJGPU_PHASED_CLOSEST")) S.incoherent_rays = atoi(e) != 0;
  S.ray_perm = nullptr;
  S.trace_n_dev = nullptr;
  S.trace_ranges = nullptr;
  S.cam_uv = nullptr; S.cam_slot0 = 0; S.cam_tk = nullptr;
  S.shadow_join = nullptr;
  sc->split_shadow = S.multi_shadow_groups && S.all_opaque && !S.has_curves && !S.has_motion && S.blas_base && g_split_shadow;
  if (const char *e = getenv("FJGPU_SPLIT_SHADOW"))
    sc->split_shadow = atoi(e) != 0 && S.multi_shadow_groups && S.all_opaque && !S.has_curves && !S.has_motion && S.blas_base;
  {
    int kmax = 1;
    for (const auto &g : hs.groups) kmax = std::max(kmax, g.n_instances);
    sc->split_kfac = (uint32_t) std::min(kmax, 2);     // (more entries than that per (record, light) pair on average: overflow -> fallback;
                                                       //  C2 has 0.84; light-loop time at a bound of 2 / 3 / 4: 41 / 43 / 45 ms)
    if (const char *e = getenv("FJGPU_SPLIT_KFAC")) sc->split_kfac = (uint32_t) std::max(1, atoi(e));
  }
  for (int k = 0; k < 3; k++) { sc->scene_box[k] = DBL_MAX; sc->scene_box[3 + k] = -DBL_MAX; }
  for (const auto &I : hs.instances)
    for (int k = 0; k < 3; k++) { sc->scene_box[k] = std::min(sc->scene_box[k], I.wbounds[k]); sc->scene_box[3 + k] = std::max(sc->scene_box[3 + k], I.wbounds[3 + k]); }
  // default: scenes whose shaders scatter (diffuse bounces, two children per hit) sort their secondary rays
  // (not where the groups are flat: one walk per ray through one tree gains less from sorted rays than the sort costs -- C4 672 -> 653 ms without it)
  sc->ray_sort_bits = g_ray_sort >= 0 ? (int) g_ray_sort : (S.incoherent_rays && !S.has_curves && !S.has_motion && !S.flats ? FJ_RAY_SORT_BITS : 0);
  if (const char *e = getenv("FJGPU_RAY_SORT")) sc->ray_sort_bits = std::max(0, std::min(9, atoi(e)));
  HIP_TRY(hipDeviceSynchronize());
  lap("done");
  *out = sc.release();
  return 0;
}

static int build_host_scene(const fj_scene_desc *desc, fjgpu::HostScene *hs)
{
  std::string err;
  const auto t_build0 = std::chrono::steady_clock::now();
  // not set: the host's binned-SAH build where frames repeat (its tree traces 3-6 % faster), the GPU's clustering build for a scene that
  // renders one frame (0.03 s instead of 0.4 s at 7.2 M triangles; bin/scene on C3 end to end: 2.2 -> 1.5 s, profiles/r05_e2e_scene.txt)
  long device_mode = g_device_build >= 0 ? g_device_build : (g_single_frame ? 1 : 0);
  if (const char *e = getenv("FJGPU_DEVICE_BUILD")) device_mode = std::max(0, std::min(2, atoi(e)));
  const bool device_build = device_mode != 0;
  hs->device_build_quality = device_mode == 2 ? 0 : 1;
  long passes = g_treelet_passes;
  if (const char *e = getenv("FJGPU_TREELET_PASSES")) passes = std::max(0, std::min(8, atoi(e)));
  hs->device_build_treelet_passes = (int) passes;
  const int be = fjgpu::BuildHostScene(desc, hs, &err, device_build);
  if (getenv("FJGPU_VERBOSE"))
    fprintf(stderr, "fjgpu: host scene build (BLAS, transforms, lights) %.3f s\n",
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t_build0).count());
  if (be) return fail(be, err);
  return 0;
}

extern "C" {

int fjgpu_scene_create(const fj_scene_desc *desc, int device, fjgpu_scene **out)
{
  if (!out || !desc) return fail(FJGPU_EINVAL, "null argument");
  *out = nullptr;
  fjgpu::HostScene hs;
  if (const int be = build_host_scene(desc, &hs)) return be;
  return upload_scene(desc, hs, device, out);
}

int fjgpu_scene_create_multi(const fj_scene_desc *desc, const int *devices, int n_devices, fjgpu_scene **out)
{
  if (!out || !desc || !devices || n_devices < 1) return fail(FJGPU_EINVAL, "bad argument");
  for (int k = 0; k < n_devices; k++) out[k] = nullptr;
  fjgpu::HostScene hs;                         // built once (the BLAS build is the expensive part), replicated
  if (const int be = build_host_scene(desc, &hs)) return be;
  for (int k = 0; k < n_devices; k++) {
    const int e = upload_scene(desc, hs, devices[k], &out[k]);
    if (e) { for (int j = 0; j < k; j++) { fjgpu_scene_destroy(out[j]); out[j] = nullptr; } return e; }
  }
  return 0;
}

void fjgpu_scene_destroy(fjgpu_scene *scene)
{
  if (!scene) return;
  (void) hipSetDevice(scene->device);
  (void) hipDeviceSynchronize();
  if (getenv("FJGPU_PHASE_STATS")) debug_phase_stats();
  if (scene->shadow_stream) (void) hipStreamDestroy(scene->shadow_stream);
  if (scene->read_stream) (void) hipStreamDestroy(scene->read_stream);
  if (scene->ev_shaded) (void) hipEventDestroy(scene->ev_shaded);
  for (hipEvent_t e : scene->ev_shadow_done) if (e) (void) hipEventDestroy(e);
  for (hipEvent_t e : scene->ev_frame) if (e) (void) hipEventDestroy(e);
  for (hipEvent_t e : scene->ev_pool) (void) hipEventDestroy(e);
  if (scene->d_frame) (void) hipFree(scene->d_frame);
  if (scene->d_slab) (void) hipFree(scene->d_slab);
  if (scene->d_rects) (void) hipFree(scene->d_rects);
  delete scene;
}

int fjgpu_host_instance_level(const fj_scene_desc *desc, int group, int32_t *out_inst, int32_t *out_skip, double *out_box, int cap)
{
  if (!desc || group < 0 || group >= desc->n_groups) return fail(FJGPU_EINVAL, "bad instance-level query");
  fjgpu::HostScene hs;
  std::string err;
  // (meshes are not needed for the instance level: their BLAS build is bypassed like in a device build)
  const int e = fjgpu::BuildHostScene(desc, &hs, &err, true);
  if (e) return fail(e, err);
  const DGroup &G = hs.groups[group];
  for (int k = 0; k < G.count && k < cap; k++) {
    const DTNode &nd = hs.group_nodes[G.first + k];
    if (out_inst) out_inst[k] = nd.inst;
    if (out_skip) out_skip[k] = nd.inst < 0 ? nd.skip - G.first : 0;
    if (out_box) std::memcpy(out_box + 6 * (size_t) k, nd.box, sizeof(nd.box));
  }
  return G.count;
}

int fjgpu_host_light_hulls(const fj_scene_desc *desc, int group, void *out_records, double *out_Pl, int cap, double *out_M)
{
  if (!desc || group < 0 || group >= desc->n_groups) return fail(FJGPU_EINVAL, "bad light-hull query");
  fjgpu::HostScene hs;
  std::string err;
  const int e = fjgpu::BuildHostScene(desc, &hs, &err, true);
  if (e) return fail(e, err);
  std::vector<int32_t> rows;
  std::vector<DLightCone> hulls;
  int n_rows = 0, n_records = 0;
  std::vector<double> cone_reach(hs.groups.size(), -1.);       // (the uploaded records carry the smaller of the two rows' reaches: the same here)
  for (size_t g = 0; g < hs.groups.size(); g++) cone_reach[g] = box_cone_row_reach(hs, g);
  build_light_hull_rows(hs, cone_reach, hulls, rows, &n_rows, &n_records);
  if (out_M) {
    if (hs.groups[group].n_instances != 1) return fail(FJGPU_EINVAL, "light-hull query: the group has several instances");
    std::memcpy(out_M, hs.instances[hs.group_members[hs.group_member_first[group]]].M, 12 * sizeof(double));
  }
  const size_t nl = hs.light_samples.size();
  for (size_t l = 0; l < nl && (int) l < cap; l++) {
    if (out_records) {
      if (rows[group] >= 0) std::memcpy((char *) out_records + l * sizeof(DLightCone), &hulls[(size_t) rows[group] * nl + l], sizeof(DLightCone));
      else std::memset((char *) out_records + l * sizeof(DLightCone), 0, sizeof(DLightCone));
    }
    if (out_Pl) for (int k = 0; k < 3; k++) out_Pl[3 * l + k] = hs.light_samples[l].P[k];
  }
  return (int) nl;
}

int fjgpu_host_curve_blas(const fj_scene_desc *desc, int curve_set, int32_t *out_curve, float *out_capsule, int32_t *out_depth,
                          float *out_box, int cap, int32_t *out_grid_n, double *out_grid_cell, double *out_bounds)
{
  if (!desc || curve_set < 0 || curve_set >= desc->n_curves) return fail(FJGPU_EINVAL, "bad curve-BLAS query");
  fjgpu::HostPrimSet ps;
  std::string err;
  const int e = fjgpu::BuildCurveSet(desc->curves[curve_set], &ps, &err);
  if (e) return fail(e, err);
  const int n = ps.n_prims;
  for (int k = 0; k < 3; k++) {
    if (out_grid_n) out_grid_n[k] = ps.grid_n[k];
    if (out_grid_cell) out_grid_cell[k] = ps.grid_cell[k];
  }
  if (out_bounds) std::memcpy(out_bounds, ps.bounds, sizeof(ps.bounds));
  for (int s = 0; s < n && s < cap; s++) {
    if (out_curve) out_curve[s] = (int32_t) ps.prim_ids[s];
    if (out_capsule) std::memcpy(out_capsule + 7 * (size_t) s, &ps.curve_capsule[(size_t) s * 8], 7 * sizeof(float));
    if (out_depth) out_depth[s] = ps.curve_depth[s];
  }
  if (out_box && n > 0) {
    if (ps.root & FJ_LEAF_FLAG) {
      if (cap > 0) for (int k = 0; k < 6; k++) out_box[k] = (float) ps.bounds[k];
    } else {
      std::vector<char> seen((size_t) n, 0);
      std::vector<uint32_t> todo(1, ps.root);          // (from the root: the node storage is handed out in chunks, not all of it is used)
      while (!todo.empty()) {
        const uint32_t at = todo.back();
        todo.pop_back();
        if (at >= ps.nodes.size()) return fail(FJGPU_EINVAL, "curve-BLAS query: node index out of range");
        const DNode &nd = ps.nodes.data()[at];
        for (int k = 0; k < 4; k++) {
          const uint32_t c = nd.child[k];
          if (c == FJ_NO_CHILD) continue;
          if (!(c & FJ_LEAF_FLAG)) { todo.push_back(c); continue; }
          const uint32_t first = (c & ~FJ_LEAF_FLAG) >> 3, count = (c & 7u) + 1;
          for (uint32_t s = first; s < first + count && s < (uint32_t) n; s++) {
            seen[s] = 1;
            if ((int) s < cap) for (int a = 0; a < 3; a++) { out_box[6 * (size_t) s + a] = nd.box[k][2 * a]; out_box[6 * (size_t) s + 3 + a] = nd.box[k][2 * a + 1]; }
          }
        }
      }
      for (int s = 0; s < n; s++) if (!seen[s]) return fail(FJGPU_EINVAL, "curve-BLAS query: a slot has no leaf");
    }
  }
  return n;
}

int fjgpu_build_config(const char *name, double *value)
{
  if (!name || !value) return fail(FJGPU_EINVAL, "bad build_config call");
  if (!kernels_build_config(name, value)) return fail(FJGPU_EINVAL, std::string("unknown build_config name ") + name);
  return 0;
}

int fjgpu_scene_query(const fjgpu_scene *scene, const char *name, double *value)
{
  if (!scene || !name || !value) return fail(FJGPU_EINVAL, "bad query call");
  const std::string n(name);
  if (n == "node_record_bytes") { *value = (double) sizeof(DNode); return 0; }
  if (n == "anyhit_node_record_bytes") { *value = (double) sizeof(DNodeQ); return 0; }
  if (n == "tri_record_bytes") { *value = scene->tri_record_bytes; return 0; }
  if (n == "scene_bytes") { *value = (double) scene->mem.bytes; return 0; }
  if (n == "work_bytes") { *value = (double) (scene->work ? scene->work->bytes : 0); return 0; }
  if (n == "stack_need") { *value = scene->stack_need; return 0; }
  if (n == "sampler_seed") { *value = (double) scene->sampler_seed; return 0; }
  if (n == "blas_nodes") { *value = (double) scene->blas_nodes; return 0; }
  if (n == "blas_treelet_passes") { *value = (double) scene->blas_treelet_passes; return 0; }
  if (n == "blas_treelets_changed") { *value = (double) scene->blas_treelets_changed; return 0; }
  if (n == "blas_sah_cost_initial") { *value = scene->blas_sah_cost_initial; return 0; }
  if (n == "blas_sah_cost") { *value = scene->blas_sah_cost; return 0; }
  if (n == "stack_peak") { *value = (double) std::max(scene->stack_peak_closest, scene->stack_peak_shadow); return 0; }
  if (n == "stack_peak_closest") { *value = (double) scene->stack_peak_closest; return 0; }
  if (n == "stack_peak_shadow") { *value = (double) scene->stack_peak_shadow; return 0; }
  // entries a walk keeps in LDS before it goes to the overflow area, by kernel family
  if (n == "stack_lds") { *value = FJ_STACK_LDS; return 0; }
  if (n == "stack_lds_anyhit") { *value = FJ_STACK_LDS_ANYHIT; return 0; }
  if (n == "stack_lds_curves") { *value = FJ_STACK_LDS_CURVES; return 0; }
  if (n == "stack_lds_canyhit") { *value = FJ_STACK_LDS_CANYHIT; return 0; }
  if (n == "stack_lds_min") { *value = FJ_STACK_LDS_MIN; return 0; }
  // 1: shadow rays are walked by k_shadow_anyhit (every occluder opaque, no curves, no motion), 0: by k_shadow_trace
  // 1: shadow rays are walked by k_shadow_anyhit_curves (curve scene, every occluder opaque, no motion, instance level within the curve budget)
  if (n == "curve_anyhit") {
    const DScene &S = scene->S;
    *value = (S.has_curves && !S.has_motion && S.all_opaque && S.curve_anyhit && S.inst_lds && S.n_group_nodes <= FJ_INST_LDS_NODES_CURVES &&
              S.n_instances <= FJ_INST_LDS_INSTS_CURVES && S.n_groups <= FJ_INST_LDS_GROUPS_CURVES && FJ_CURVE_QNODES && FJ_CLOSEST_QNODES) ? 1 : 0;
    return 0;
  }
  if (n == "lean_anyhit") { *value = (scene->S.all_opaque && !scene->S.has_curves && !scene->S.has_motion && scene->S.blas_base) ? 1 : 0; return 0; }
  // which closest-hit kernel walks this scene (launch_trace_closest): 0 k_trace_closest<false, *, false>, 1 k_trace_closest_phased,
  // 2 k_trace_closest<true, *, false> (curve sets), 3 k_trace_closest<true, *, true> (time-sampled transforms / vertex velocities)
  // 4 k_trace_closest_flat (incoherent rays, every group flat, instance level within the phased walk's LDS budget)
  if (n == "closest_kernel") {
    const DScene &S = scene->S;
    const bool flat = !S.has_motion && !S.has_curves && S.flats;
    *value = S.has_motion ? 3 : (S.has_curves ? 2 : (flat ? 4 : (S.incoherent_rays ? 1 : 0)));
    return 0;
  }
  // ... and the node record it reads: the 64-byte quantised twin unless the ribbon test / motion instantiation runs
  if (n == "closest_node_record_bytes") { *value = (double) ((scene->S.has_motion || (scene->S.has_curves && !FJ_CURVE_QNODES) || !FJ_CLOSEST_QNODES) ? sizeof(DNode) : sizeof(DNodeQ)); return 0; }
  // per-light shadow cones: single-instance groups with a row in the table, records of those rows with at least one plane; and, in a
  // -DFJ_LIGHT_CONE_VALIDATE build, the light loop's verdicts since the library was loaded and how many of them the exact test contradicted
  // (every scene of the process; other builds: -1)
  if (n == "light_cone_rows") { *value = scene->cone_rows; return 0; }
  if (n == "light_cone_records") { *value = scene->cone_records; return 0; }
  if (n == "light_cone_verdicts" || n == "light_cone_contradictions") {
    double v = -1, c = -1;
    if (hipSetDevice(scene->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(FJGPU_ENODEV, "hipSetDevice / hipDeviceSynchronize");
    light_cone_validate_counts(&v, &c);
    *value = n == "light_cone_verdicts" ? v : c;
    return 0;
  }
  // per-light hull cones: groups with a row, records with planes, the pairs they settled in the last counting frame; and, in a
  // -DFJ_LIGHT_HULL_VALIDATE build, the settled pairs walked since the library was loaded and how many of those walks found a hit
  if (n == "light_hull_rows") { *value = scene->hull_rows; return 0; }
  if (n == "light_hull_records") { *value = scene->hull_records; return 0; }
  if (n == "light_hull_verdicts" || n == "light_hull_contradictions") {
    double v = -1, c = -1;
    if (hipSetDevice(scene->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(FJGPU_ENODEV, "hipSetDevice / hipDeviceSynchronize");
    light_hull_validate_counts(&v, &c);
    if (n == "light_hull_verdicts") *value = v >= 0 ? v : (double) scene->hull_verdicts;
    else *value = c;
    return 0;
  }
  // -DFJ_TRI_FILTER_VALIDATE build: the verdicts of the lean any-hit walk's f32 triangle filter since the library was loaded (or since the
  // FJGPU_PHASE_STATS print last reset them), the hits of the exact test behind them and the verdicts it contradicted; other builds: -1.  Read only.
  {
    static const char *const tf[5] = {"tri_filter_miss", "tri_filter_hit", "tri_filter_maybe", "tri_filter_exact_hits", "tri_filter_contradictions"};
    for (int k = 0; k < 5; k++)
      if (n == tf[k]) {
        double c[5];
        if (hipSetDevice(scene->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return fail(FJGPU_ENODEV, "hipSetDevice / hipDeviceSynchronize");
        tri_filter_validate_counts(c);
        *value = c[k];
        return 0;
      }
  }
  // batches of the last render call whose samples were cleared by a memset (the adaptive sampler's, or every batch with option shade_first_touch 0)
  if (n == "accum_memsets") { *value = (double) scene->accum_memsets; return 0; }
  if (n == "has_curves") { *value = scene->S.has_curves; return 0; }
  if (n == "has_motion") { *value = scene->S.has_motion; return 0; }
  return fail(FJGPU_EINVAL, "unknown query " + n);
}

int fjgpu_set_batch_callback(fjgpu_scene *scene, fjgpu_batch_fn fn, void *user)
{
  if (!scene) return fail(FJGPU_EINVAL, "null scene");
  scene->batch_fn = fn; scene->batch_user = fn ? user : nullptr;
  return 0;
}

int fjgpu_dev_rccl_selftest(int device, int n_floats)
{
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(FJGPU_ENODEV, "no such HIP device");
  if (n_floats < 1) return fail(FJGPU_EINVAL, "bad size");
  HIP_TRY(hipSetDevice(device));
  std::string why;
  const std::vector<Rccl::comm_t> *comms = rccl_comms(std::vector<int>{device}, &why);
  if (!comms) return fail(FJGPU_ENODEV, "RCCL: " + why);
  Rccl &R = rccl();
  DeviceBuffers M;
  std::vector<float> src((size_t) n_floats), got((size_t) n_floats, -1.f);
  for (int i = 0; i < n_floats; i++) src[(size_t) i] = (float) (i % 1013) * .5f;
  const float *d_src = nullptr;
  float *d_dst = nullptr;
  if (M.upload(src.data(), src.size(), &d_src) || M.alloc(src.size(), &d_dst)) return fail(FJGPU_ENOMEM, "device allocation failed");
  HIP_TRY(hipMemset(d_dst, 0xff, sizeof(float) * src.size()));
  // the exchange's own calls on a communicator of one rank: a send to, and the matching receive from, rank 0 in one group
  int e = R.GroupStart();
  if (!e) e = R.Send(d_src, src.size(), Rccl::kFloat, 0, (*comms)[0], nullptr);
  if (!e) e = R.Recv(d_dst, src.size(), Rccl::kFloat, 0, (*comms)[0], nullptr);
  const int e2 = R.GroupEnd();
  if (e || e2) return fail(FJGPU_ENODEV, std::string("RCCL self exchange: ") + (R.GetErrorString ? R.GetErrorString(e ? e : e2) : "error"));
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(got.data(), d_dst, sizeof(float) * got.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < got.size(); i++) if (got[i] != src[i]) return fail(FJGPU_ENODEV, "RCCL self exchange returned other data");
  return 0;
}

int fjgpu_dev_sort_pairs(int device, const uint32_t *keys, int n, int key_bits, uint32_t *keys_out, uint32_t *perm, int repeats, double *sort_ms)
{
  if (n < 0 || key_bits < 1 || key_bits > 32 || (n > 0 && !keys)) return fail(FJGPU_EINVAL, "bad sort call");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(FJGPU_ENODEV, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  if (sort_ms) *sort_ms = 0;
  if (n == 0) return 0;
  DeviceBuffers M;
  const uint32_t *d_keys = nullptr;
  uint32_t *d_out = nullptr, *d_perm = nullptr;
  char *d_tmp = nullptr;
  const size_t tmp_bytes = ray_sort_pairs_temp_bytes((uint32_t) n, key_bits);
  if (M.upload(keys, (size_t) n, &d_keys) || M.alloc((size_t) n, &d_out) || M.alloc((size_t) n, &d_perm) || M.alloc(tmp_bytes, &d_tmp))
    return fail(FJGPU_ENOMEM, "device allocation failed for the sort");
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  double best = 1e30;
  for (int k = 0; k < std::max(1, repeats); k++) {
    (void) hipEventRecord(e0, nullptr);
    if (ray_sort_pairs(nullptr, d_keys, (uint32_t) n, key_bits, d_out, d_perm, d_tmp, tmp_bytes, keys_out != nullptr)) { (void) hipEventDestroy(e0); (void) hipEventDestroy(e1); return fail(FJGPU_ENODEV, "the sort's launches failed"); }
    (void) hipEventRecord(e1, nullptr);
    if (hipEventSynchronize(e1) != hipSuccess) { (void) hipEventDestroy(e0); (void) hipEventDestroy(e1); return fail(FJGPU_ENODEV, std::string("sort: ") + hipGetErrorString(hipGetLastError())); }
    float ms = 0.f;
    (void) hipEventElapsedTime(&ms, e0, e1);
    best = std::min(best, (double) ms);
  }
  (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
  if (sort_ms) *sort_ms = best;
  if (keys_out) HIP_TRY(hipMemcpy(keys_out, d_out, sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost));
  if (perm) HIP_TRY(hipMemcpy(perm, d_perm, sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost));
  return 0;
}

int fjgpu_dev_slab32_batch(int device, int n, const double *rays, const double *grid, const uint32_t *words, void *out)
{
  if (n < 0 || (n > 0 && (!rays || !grid || !words || !out))) return fail(FJGPU_EINVAL, "bad slab32 batch call");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(FJGPU_ENODEV, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  if (n == 0) return 0;
  DeviceBuffers M;
  const double *d_rays = nullptr, *d_grid = nullptr;
  const uint32_t *d_words = nullptr;
  char *d_out = nullptr;
  if (M.upload(rays, (size_t) n * 8, &d_rays) || M.upload(grid, (size_t) n * 6, &d_grid) || M.upload(words, (size_t) n * 3, &d_words) || M.alloc((size_t) n * 128, &d_out))
    return fail(FJGPU_ENOMEM, "device allocation failed for the slab32 batch");
  if (launch_slab32_batch(nullptr, (uint32_t) n, d_rays, d_grid, d_words, d_out)) return fail(FJGPU_ENODEV, "the slab32 batch launch failed");
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(out, d_out, (size_t) n * 128, hipMemcpyDeviceToHost));
  return 0;
}

int fjgpu_dev_quantize_nodes(int device, int n, const void *nodes, const double *origin, const double *cell, void *out)
{
  if (n < 0 || !origin || !cell || (n > 0 && (!nodes || !out))) return fail(FJGPU_EINVAL, "bad quantize call");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return fail(FJGPU_ENODEV, "no such HIP device");
  HIP_TRY(hipSetDevice(device));
  if (n == 0) return 0;
  DeviceBuffers M;
  const DNode *d_nodes = nullptr;
  DNodeQ *d_out = nullptr;
  if (M.upload((const DNode *) nodes, (size_t) n, &d_nodes) || M.alloc((size_t) n, &d_out)) return fail(FJGPU_ENOMEM, "device allocation failed for the quantiser");
  if (launch_quantize_nodes(nullptr, d_nodes, (uint32_t) n, origin, cell, d_out)) return fail(FJGPU_ENODEV, "the quantiser's launch failed");
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(out, d_out, sizeof(DNodeQ) * (size_t) n, hipMemcpyDeviceToHost));
  return 0;
}

int fjgpu_set_option(fjgpu_scene *scene, const char *name, long value)
{
  if (!scene || !name) return fail(FJGPU_EINVAL, "bad option call");
  const std::string n(name);
  if (n == "batch_tiles") { scene->batch_tiles = value; return 0; }
  if (n == "batch_samples") { scene->batch_samples = value < 0 ? 0 : value; return 0; }
  if (n == "aov_batch_samples") { scene->aov_batch_samples = value < 0 ? 0 : value; return 0; }
  if (n == "count_nodes") { scene->count_events = value != 0; return 0; }
  if (n == "count_all_shadow") { scene->count_all_shadow = value != 0; return 0; }
  if (n == "light_cones") { scene->light_cones = value != 0; return 0; }
  if (n == "light_hulls") { scene->light_hulls = value != 0; return 0; }
  if (n == "shade_first_touch") {
    if (value != 0 && value != 1) return fail(FJGPU_EINVAL, "shade_first_touch: 0 (memset and atomic adds at the camera level) or 1 (one store per sample)");
    scene->shade_first_touch = value;
    return 0;
  }
  if (n == "sampler_seed") {
    if (value < 0 || value > 65535) return fail(FJGPU_EINVAL, "sampler_seed: " + std::to_string(value) + " is outside 0..65535 (0: the unseeded streams)");
    scene->sampler_seed = value;      // (the tables follow at the next call that reads them: ensure_work)
    return 0;
  }
  if (n == "overlap_shadow") {
    if (value < 0 || value > 2) return fail(FJGPU_EINVAL, "overlap_shadow: 0 off, 1 on, 2 by the batch size");
    scene->overlap = value;
    return 0;
  }
  if (n == "release_work") {
    // the work arena back to the driver (the scene stays): a host that keeps its scene but renders nothing for a while -- or, like bench.py's
    // counter passes, wants another process to find the memory this one found.  The next render call allocates again.
    if (value && scene->work) {
      if (hipSetDevice(scene->device) != hipSuccess) return fail(FJGPU_ENODEV, "hipSetDevice");
      (void) hipDeviceSynchronize();
      fjgpu::ForgetWorkArena(scene);
    }
    return 0;
  }
  return fail(FJGPU_EINVAL, "unknown option " + n);
}

// One frame on G devices of this process: the reference's worker pool (execute_rendering,
// src/fj_renderer.cc:747-791; MtRunParallelLoop, src/fj_multi_thread.cc:86-132) with GPUs for
// workers.  Tile k of the list goes to scene k % G (interleaved deal: neighbouring tiles cost
// alike), every device renders its share on its own host thread, packs the finished tiles into
// one slab, and the slab crosses xGMI as one peer copy into the first device, which scatters it
// into the frame; the frame goes to the host once.
int fjgpu_render_frame_multi(fjgpu_scene *const *scenes, int n_scenes, const fj_render_desc *r,
    const int32_t *tile_ids, int n_tiles, float *h_fb, fjgpu_stats *stats)
{
  if (!scenes || n_scenes < 1 || !r || !h_fb) return fail(FJGPU_EINVAL, "null argument");
  for (int k = 0; k < n_scenes; k++) if (!scenes[k]) return fail(FJGPU_EINVAL, "null scene");
  if (const char *why = bad_render(r)) return fail(FJGPU_EINVAL, why);
  std::vector<fjgpu::TileRect> all;
  fjgpu::GenerateTiles(*r, &all);
  std::vector<int32_t> ids;
  if (const int e = listed_tiles(tile_ids, n_tiles, all.size(), &ids)) return e;
  const int G = n_scenes;
  const size_t npx = (size_t) r->xres * r->yres;
  const int tile_px = r->tile_w * r->tile_h;
  std::vector<std::vector<int32_t>> mine(G);
  for (size_t k = 0; k < ids.size(); k++) mine[k % G].push_back(ids[k]);
  fjgpu_scene *first = scenes[0];

  // the first device's frame and the staging area for the other devices' slabs
  HIP_TRY(hipSetDevice(first->device));
  if (grow((void **) &first->d_frame, &first->d_frame_n, npx * 4, sizeof(float))) return fail(FJGPU_ENOMEM, "device allocation failed for the frame");
  HIP_TRY(hipMemset(first->d_frame, 0, npx * 4 * sizeof(float)));
  std::vector<size_t> stage_off(G, 0);
  size_t stage_px = 0, rects_n = 0;
  for (int d = 1; d < G; d++) { stage_off[d] = stage_px; stage_px += mine[d].size() * (size_t) tile_px; rects_n += mine[d].size(); }
  if (G > 1) {
    if (grow((void **) &first->d_slab, &first->d_slab_n, stage_px * 4, sizeof(float)) ||
        grow((void **) &first->d_rects, &first->d_rects_n, rects_n * 4, sizeof(int32_t)))
      return fail(FJGPU_ENOMEM, "device allocation failed for the tile slabs");
  }

  // The exchange: one peer copy per device (default: nothing to bring up for a frame), or -- option "multi_exchange" 1 / FJGPU_MULTI_RCCL=1, devices all
  // distinct -- RCCL's grouped point-to-point calls: every device's thread sends its slab to rank 0, whose thread posts all receives in one group
  // (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd over xGMI).  A communicator set that cannot be created falls back to the peer copies.
  const std::vector<Rccl::comm_t> *comms = nullptr;
  {
    bool want = g_multi_exchange == 1;
    if (const char *e = getenv("FJGPU_MULTI_RCCL")) want = atoi(e) != 0;
    std::vector<int> devs(G);
    for (int d = 0; d < G; d++) devs[d] = scenes[d]->device;
    std::vector<int> uniq = devs;
    std::sort(uniq.begin(), uniq.end());
    const bool distinct = std::adjacent_find(uniq.begin(), uniq.end()) == uniq.end();
    if (want && G > 1 && distinct) {
      std::string why;
      comms = rccl_comms(devs, &why);
      if (!comms && getenv("FJGPU_VERBOSE")) fprintf(stderr, "fjgpu: RCCL exchange not available (%s): peer copies\n", why.c_str());
    }
  }
  std::vector<int> rcs(G, 0);
  std::vector<std::string> errs(G);
  std::vector<fjgpu_stats> sts(G);
  auto work = [&](int d) {
    fjgpu_scene *sc = scenes[d];
    fjgpu_stats &st = sts[d];
    std::memset(&st, 0, sizeof(st));
    auto bad = [&](int code, const std::string &m) { rcs[d] = code; errs[d] = m; };
    if (hipSetDevice(sc->device) != hipSuccess) return bad(FJGPU_ENODEV, "hipSetDevice failed");
    if (mine[d].empty()) return;
    float *fb = first->d_frame;
    if (d > 0) {
      // (a second scene on the first device -- a test set-up -- still renders into its own frame)
      if (grow((void **) &sc->d_frame, &sc->d_frame_n, npx * 4, sizeof(float)) ||
          grow((void **) &sc->d_slab, &sc->d_slab_n, mine[d].size() * (size_t) tile_px * 4, sizeof(float)) ||
          grow((void **) &sc->d_rects, &sc->d_rects_n, mine[d].size() * 4, sizeof(int32_t)))
        return bad(FJGPU_ENOMEM, "device allocation failed for a device's frame");
      fb = sc->d_frame;
      // (tiles a batch callback keeps from being rendered are packed and sent all the same: they read 0)
      if (sc->batch_fn && hipMemset(fb, 0, npx * 4 * sizeof(float)) != hipSuccess) return bad(FJGPU_ENODEV, "frame clear failed");
    }
    const int e = fjgpu_render_tiles(sc, r, mine[d].data(), (int) mine[d].size(), fb, nullptr, &st);
    if (e) return bad(e, fjgpu_last_error());
    if (d > 0) {
      std::vector<int32_t> rects(mine[d].size() * 4);
      for (size_t k = 0; k < mine[d].size(); k++) {
        const fjgpu::TileRect &t = all[mine[d][k]];
        rects[4 * k] = t.xmin; rects[4 * k + 1] = t.ymin; rects[4 * k + 2] = t.xmax; rects[4 * k + 3] = t.ymax;
      }
      if (hipMemcpy(sc->d_rects, rects.data(), rects.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess)
        return bad(FJGPU_ENODEV, "rect upload failed");
      if (launch_move_tiles(nullptr, false, fb, r->xres, sc->d_rects, (int) mine[d].size(), tile_px, sc->d_slab)) return bad(FJGPU_ENODEV, "pack launch failed");
      // one peer copy per device: over xGMI when peer access is available, staged by the runtime otherwise.  (The RCCL exchange is NOT posted here:
      // a device whose frame failed would leave its partner waiting in the group for ever -- it runs below, after the join, once every device succeeded.)
      const size_t bytes = mine[d].size() * (size_t) tile_px * 4 * sizeof(float);
      if (comms) { if (hipStreamSynchronize(nullptr) != hipSuccess) return bad(FJGPU_ENODEV, "tile pack failed"); }
      else if (hipMemcpyPeer(first->d_slab + stage_off[d] * 4, first->device, sc->d_slab, sc->device, bytes) != hipSuccess)
        return bad(FJGPU_ENODEV, std::string("peer copy of a tile slab: ") + hipGetErrorString(hipGetLastError()));
    }
  };
  if (G == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int d = 0; d < G; d++) th.emplace_back(work, d);
    for (auto &t : th) t.join();
  }
  for (int d = 0; d < G; d++) if (rcs[d]) return fail(rcs[d], "device " + std::to_string(scenes[d]->device) + ": " + errs[d]);

  if (comms) {
    // The slab exchange in RCCL's spelling, collective over SUCCESS: it is entered only when every device rendered and packed its share (checked above),
    // from this one thread, as ONE group -- every non-empty device's send to rank 0 on its own communicator and rank 0's receives, also when rank 0
    // itself holds no tile -- so no rank can be left waiting for a partner that returned early.
    Rccl &R = rccl();
    int e = R.GroupStart();
    for (int q = 1; q < G && !e; q++) {
      if (mine[q].empty()) continue;
      const size_t count = mine[q].size() * (size_t) tile_px * 4;
      e = R.Send(scenes[q]->d_slab, count, Rccl::kFloat, 0, (*comms)[q], nullptr);
      if (!e) e = R.Recv(first->d_slab + stage_off[q] * 4, count, Rccl::kFloat, q, (*comms)[0], nullptr);
    }
    const int e2 = R.GroupEnd();
    if (e || e2) return fail(FJGPU_ENODEV, std::string("RCCL exchange of the tile slabs: ") + (R.GetErrorString ? R.GetErrorString(e ? e : e2) : "error"));
    for (int d = 0; d < G; d++) {
      HIP_TRY(hipSetDevice(scenes[d]->device));
      HIP_TRY(hipStreamSynchronize(nullptr));
    }
  }
  HIP_TRY(hipSetDevice(first->device));
  if (G > 1) {
    std::vector<int32_t> rects;
    for (int d = 1; d < G; d++)
      for (int32_t id : mine[d]) { const fjgpu::TileRect &t = all[id]; rects.insert(rects.end(), {t.xmin, t.ymin, t.xmax, t.ymax}); }
    if (!rects.empty()) {
      HIP_TRY(hipMemcpy(first->d_rects, rects.data(), rects.size() * sizeof(int32_t), hipMemcpyHostToDevice));
      if (launch_move_tiles(nullptr, true, first->d_frame, r->xres, first->d_rects, (int) (rects.size() / 4), tile_px, first->d_slab))
        return fail(FJGPU_ENODEV, "unpack launch failed");
    }
  }
  HIP_TRY(hipMemcpy(h_fb, first->d_frame, npx * 4 * sizeof(float), hipMemcpyDeviceToHost));
  if (stats) for (int d = 0; d < G; d++) stats[d] = sts[d];
  return 0;
}

int fjgpu_pack_tiles(const float *d_fb, int xres, const int32_t *d_rects, int n_tiles, int tile_px, float *d_slab, void *hip_stream)
{
  if (!d_fb || !d_rects || !d_slab || xres <= 0 || tile_px <= 0 || n_tiles < 0) return fail(FJGPU_EINVAL, "bad tile slab arguments");
  if (launch_move_tiles(static_cast<hipStream_t>(hip_stream), false, const_cast<float *>(d_fb), xres, d_rects, n_tiles, tile_px, d_slab))
    return fail(FJGPU_ENODEV, "tile pack launch failed");
  return 0;
}

int fjgpu_unpack_tiles(float *d_fb, int xres, const int32_t *d_rects, int n_tiles, int tile_px, const float *d_slab, void *hip_stream)
{
  if (!d_fb || !d_rects || !d_slab || xres <= 0 || tile_px <= 0 || n_tiles < 0) return fail(FJGPU_EINVAL, "bad tile slab arguments");
  if (launch_move_tiles(static_cast<hipStream_t>(hip_stream), true, d_fb, xres, d_rects, n_tiles, tile_px, const_cast<float *>(d_slab)))
    return fail(FJGPU_ENODEV, "tile unpack launch failed");
  return 0;
}

int fjgpu_render_frame(fjgpu_scene *sc, const fj_render_desc *r, float *h_fb, fjgpu_stats *stats)
{
  fjgpu_scene *one[1] = {sc};
  if (!sc) return fail(FJGPU_EINVAL, "null argument");
  return fjgpu_render_frame_multi(one, 1, r, nullptr, 0, h_fb, stats);
}

int fjgpu_trace(fjgpu_scene *sc, int group, int n, const double *rays, double *out_t, int32_t *out_ids,
    double *out_uv, fjgpu_stats *stats)
{
  if (!sc || !rays || !out_t || !out_ids || n < 0) return fail(FJGPU_EINVAL, "null argument");
  if (group < 0 || group >= sc->S.n_groups) return fail(FJGPU_EINVAL, "group out of range");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(sc->device));
  DeviceBuffers W;
  DRay *d_rays; DHit *d_hits; DCounters *d_cnt;
  double *d_ranges;
  if (W.alloc((size_t) n, &d_rays) || W.alloc((size_t) n * 2, &d_ranges) || W.alloc((size_t) n, &d_hits) || W.alloc(1, &d_cnt))
    return fail(FJGPU_ENOMEM, "device allocation failed");
  {
    // the caller's rays are Ray records of 8 doubles (o, d, tmin, tmax: include/fjgpu.h); the device keeps origin / direction and the ranges apart
    std::vector<DRay> hr((size_t) n);
    std::vector<double> hg((size_t) n * 2);
    for (int i = 0; i < n; i++) {
      for (int k = 0; k < 3; k++) { hr[i].o[k] = rays[8 * (size_t) i + k]; hr[i].d[k] = rays[8 * (size_t) i + 3 + k]; }
      hg[2 * (size_t) i] = rays[8 * (size_t) i + 6]; hg[2 * (size_t) i + 1] = rays[8 * (size_t) i + 7];
    }
    HIP_TRY(hipMemcpy(d_rays, hr.data(), sizeof(DRay) * (size_t) n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_ranges, hg.data(), sizeof(double) * 2 * (size_t) n, hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemset(d_cnt, 0, sizeof(DCounters)));
  DScene S = sc->S;
  S.target_group = group;
  S.trace_ranges = d_ranges;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  (void) hipEventRecord(e0, nullptr);
  const int le = launch_trace_closest(nullptr, S, d_rays, nullptr, d_hits, (uint32_t) n, d_cnt, (int) sc->count_events);
  (void) hipEventRecord(e1, nullptr);
  if (le) return fail(FJGPU_ENODEV, std::string("trace launch: ") + hipGetErrorString((hipError_t) le));
  HIP_TRY(hipDeviceSynchronize());
  float ms = 0;
  (void) hipEventElapsedTime(&ms, e0, e1);
  (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
  std::vector<DHit> h((size_t) n);
  HIP_TRY(hipMemcpy(h.data(), d_hits, sizeof(DHit) * (size_t) n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; i++) {
    out_t[i] = h[i].inst >= 0 ? h[i].t : DBL_MAX;
    out_ids[2 * i] = h[i].inst;
    out_ids[2 * i + 1] = h[i].inst >= 0 ? h[i].prim : -1;
    if (out_uv) { out_uv[2 * i] = h[i].inst >= 0 ? h[i].u : 0; out_uv[2 * i + 1] = h[i].inst >= 0 ? h[i].v : 0; }
  }
  sc->stack_peak_closest = sc->stack_peak_shadow = 0;
  DCounters hc;
  if (stats || sc->count_events) {
    HIP_TRY(hipMemcpy(&hc, d_cnt, sizeof(hc), hipMemcpyDeviceToHost));
    sc->stack_peak_closest = hc.stack_peak;
  }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->nodes_visited = hc.nodes; stats->prims_tested = hc.prims; stats->insts_tested = hc.insts; stats->rays_traced = hc.traced;
    stats->trace_ms = ms; stats->total_ms = ms; stats->trace_launches = 1;
  }
  return 0;
}

// ---- first-hit AOV pass.  Shaped like fjgpu_trace, not like the wavefront loop: transient buffers per call, nothing of the scene's work arena,
// options or call counters is touched, so the beauty renders around it see the scene they saw before.
#ifndef FJ_AOV_BATCH_SAMPLES
#define FJ_AOV_BATCH_SAMPLES ((long) 4 << 20)      // 132 bytes per sample: uv, ray, path and hit records of half a GB per batch
#endif

// what fjgpu_render_aov and fjgpu_camera_samples share: the refusals, the tiling, the sampler's parameters, the per-call DScene
struct AovSetup {
  std::vector<fjgpu::TileRect> all;
  int margin[2];
  GenParams gp;
  DScene S;
};
static int aov_setup(fjgpu_scene *sc, const fj_render_desc *r, const char *who, AovSetup *a)
{
  if (r->sampler_type == 1) return fail(FJGPU_EUNSUPPORTED, std::string(who) + ": the adaptive sampler is not supported (fixed-grid sampler only)");
  if (r->sampler_type != 0) return fail(FJGPU_EINVAL, "unknown sampler_type");
  if (const char *why = bad_render(r)) return fail(FJGPU_EINVAL, why);
  if (sc->S.cam_xform) return fail(FJGPU_EUNSUPPORTED, std::string(who) + ": a time-sampled camera is not supported (static cameras only)");
  if (sc->S.has_motion) return fail(FJGPU_EUNSUPPORTED, std::string(who) + ": a scene with motion (time-sampled transforms or vertex velocities) is not supported (static scenes only)");
  fjgpu::GenerateTiles(*r, &a->all);
  fjgpu::SamplerMargin(*r, a->margin);
  a->gp = gen_params(r, a->margin);
  a->S = sc->S;
  camera_uv_size(sc->cam_fov, r, a->S.cam_uv_size);
  a->S.time_start = r->time_start; a->S.time_end = r->time_end;
  a->S.lrec_hair = nullptr;
  a->S.cam_uv = nullptr; a->S.cam_tk = nullptr; a->S.cam_slot0 = 0;
  a->S.trace_ranges = nullptr; a->S.trace_n_dev = nullptr; a->S.ray_perm = nullptr;
  a->S.shadow_join = nullptr;
  return 0;
}

// the body of fjgpu_render_aov and fjgpu_render_aov_albedo: one camera-ray generation and one closest-hit walk per batch, then k_aov_reduce
// where a member of `out` is set, then k_aov_albedo where d_albedo is set, then k_aov_matte (fjgpu_matte.hip) where `matte` is set
// (fjgpu_render_aov_matte: its description and buffers, checked by the caller).  `who` is the entry point's name in the messages.
struct MatteCall { const fjgpu_matte_desc *desc; const fjgpu_matte_buffers *out; };
static int render_aov_body(const char *who_, fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    const fjgpu_aov_buffers *out, float *d_albedo, void *hip_stream, fjgpu_stats *stats, const MatteCall *matte = nullptr)
{
  const std::string who(who_);
  const bool reduce = out && (out->depth || out->position || out->normal || out->uv || out->ids || out->coverage);
  if (!reduce && !d_albedo && !matte) return fail(FJGPU_EINVAL, who + ": every buffer pointer is NULL, nothing to write");
  if (tile_ids && n_tiles < 0) return fail(FJGPU_EINVAL, who + ": negative tile count");
  AovSetup A;
  if (const int e = aov_setup(sc, r, who_, &A)) return e;
  HIP_TRY(hipSetDevice(sc->device));
  hipStream_t st = static_cast<hipStream_t>(hip_stream);

  std::vector<int32_t> ids;
  if (const int e = listed_tiles(tile_ids, n_tiles, A.all.size(), &ids)) return e;
  fjgpu_stats acc;
  std::memset(&acc, 0, sizeof(acc));
  if (ids.empty()) { if (stats) *stats = acc; return 0; }

  // batches: tiles in list order, at most `limit` samples each (a batch holds at least one tile; the tile index is grid.y: at most 65535)
  const size_t limit = (size_t) std::min<long>(sc->aov_batch_samples > 0 ? sc->aov_batch_samples : FJ_AOV_BATCH_SAMPLES, 0x7fffffffL);
  struct Batch { size_t first; int n; uint32_t samples, max_ts; int max_px; };
  std::vector<TileDesc> td(ids.size());
  std::vector<Batch> batches;
  size_t cap_samples = 0, tab_len = 0;
  for (size_t k = 0; k < ids.size(); k++) {
    const fjgpu::TileRect &t = A.all[ids[k]];
    TileDesc d = fixed_grid_tile(sc, r, t, A.margin, 0);
    const size_t ts = (size_t) d.nx * (size_t) d.ny;
    if (ts > 0x7fffffffu) return fail(FJGPU_EINVAL, who + ": a tile of more than 2^31 samples: lower the tilesize");
    if (batches.empty() || batches.back().n >= 65535 || (size_t) batches.back().samples + ts > limit) batches.push_back(Batch{k, 0, 0u, 0u, 0});
    Batch &b = batches.back();
    d.sample_offset = b.samples;
    td[k] = d;
    b.n++; b.samples += (uint32_t) ts;
    b.max_ts = std::max(b.max_ts, (uint32_t) ts);
    b.max_px = std::max(b.max_px, (t.xmax - t.xmin) * (t.ymax - t.ymin));
    cap_samples = std::max(cap_samples, (size_t) b.samples);
    tab_len = std::max(tab_len, ts);
  }

  DeviceBuffers W;
  double *d_suv; DRay *d_rays; DPath *d_paths; DHit *d_hits; DCounters *d_cnt; TileDesc *d_tiles;
  const double *d_jit = nullptr;
  if (W.alloc(cap_samples * 2, &d_suv) || W.alloc(cap_samples, &d_rays) || W.alloc(cap_samples, &d_paths) || W.alloc(cap_samples, &d_hits) ||
      W.alloc(1, &d_cnt) || W.alloc(td.size(), &d_tiles))
    return fail(FJGPU_ENOMEM, who + ": device allocation failed: lower the aov_batch_samples option");
  {
    // the per-tile XorShift stream as a table (draw k is the same number in every tile): two draws per sample of the largest tile
    std::vector<double> draws;
    fjgpu::XorShiftTableSeeded((unsigned) sc->sampler_seed, 2 * tab_len, &draws);
    if (W.upload(draws.data(), 2 * tab_len, &d_jit)) return fail(FJGPU_ENOMEM, who + ": device allocation failed");
  }
  HIP_TRY(hipMemcpy(d_tiles, td.data(), sizeof(TileDesc) * td.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_cnt, 0, sizeof(DCounters)));
  DScene S = A.S;
  S.time_tab = d_jit;      // (never read: no motion, a static camera)
  AovParams ap;
  ap.xres = r->xres; ap.rate_x = r->rate_x; ap.rate_y = r->rate_y; ap.margin_x = A.margin[0]; ap.margin_y = A.margin[1]; ap.pad = 0;
  ap.depth = ap.position = ap.normal = ap.uv = ap.coverage = nullptr; ap.ids = nullptr;
  if (reduce) { ap.depth = out->depth; ap.position = out->position; ap.normal = out->normal; ap.uv = out->uv; ap.ids = out->ids; ap.coverage = out->coverage; }
  AlbedoParams bp;
  bp.xres = r->xres; bp.rate_x = r->rate_x; bp.rate_y = r->rate_y; bp.margin_x = A.margin[0]; bp.margin_y = A.margin[1]; bp.pad = 0;
  bp.lanes = 1; bp.lanes_log2 = 0;      // lanes per pixel: the smallest power of two >= min(samples per pixel, 64)
  while (bp.lanes < 64 && (long) bp.lanes < (long) r->rate_x * r->rate_y) { bp.lanes <<= 1; bp.lanes_log2++; }
  bp.albedo = d_albedo;
  ResolveParams mrp;       // the frame and the filter window as the beauty pass's resolve sees them
  MatteParams mp;
  std::memset(&mrp, 0, sizeof(mrp));
  std::memset(&mp, 0, sizeof(mp));
  if (matte) {
    mrp.xres = r->xres; mrp.yres = r->yres; mrp.rate_x = r->rate_x; mrp.rate_y = r->rate_y;
    mrp.npx_x = r->rate_x + 2 * A.margin[0]; mrp.npx_y = r->rate_y + 2 * A.margin[1];
    mrp.fw = (double) r->filter_w; mrp.fh = (double) r->filter_h;
    mp.key = matte->desc->key; mp.ranks = matte->desc->ranks; mp.filtered = matte->desc->filtered ? 1 : 0;
    mp.margin_x = A.margin[0]; mp.margin_y = A.margin[1];
    mp.ids = matte->out->ids; mp.coverage = matte->out->coverage; mp.rest = matte->out->rest; mp.distinct = matte->out->distinct;
  }

  // event pairs around every launch, turned into durations after the one synchronisation at the end
  struct Span { hipEvent_t a, b; double *bucket; };
  std::vector<Span> spans;
  hipEvent_t ev_all[2] = {nullptr, nullptr};
  auto drop_events = [&]() {
    for (Span &sp : spans) { (void) hipEventDestroy(sp.a); (void) hipEventDestroy(sp.b); }
    for (hipEvent_t e : ev_all) if (e) (void) hipEventDestroy(e);
  };
  auto timed = [&](double *bucket, auto &&launch) -> int {
    Span sp{nullptr, nullptr, bucket};
    if (hipEventCreate(&sp.a) != hipSuccess) return -1;
    if (hipEventCreate(&sp.b) != hipSuccess) { (void) hipEventDestroy(sp.a); return -1; }
    spans.push_back(sp);
    (void) hipEventRecord(sp.a, st);
    const int le = launch();
    (void) hipEventRecord(sp.b, st);
    return le;
  };
  int rc = 0;
  if (hipEventCreate(&ev_all[0]) != hipSuccess || hipEventCreate(&ev_all[1]) != hipSuccess) rc = -1;
  if (!rc) (void) hipEventRecord(ev_all[0], st);
  for (size_t b = 0; b < batches.size() && rc == 0; b++) {
    const Batch &B = batches[b];
    const TileDesc *tiles = d_tiles + B.first;
    rc = timed(&acc.gen_ms, [&]() { return launch_gen_camera(st, S, A.gp, tiles, B.n, B.max_ts, d_jit, d_jit, d_suv, d_rays, d_paths); });
    if (rc) break;
    rc = timed(&acc.closest_ms, [&]() { return launch_trace_closest(st, S, d_rays, d_paths, d_hits, B.samples, d_cnt, (int) sc->count_events); });
    if (rc) break;
    if (reduce) rc = timed(&acc.resolve_ms, [&]() { return launch_aov_reduce(st, S, ap, tiles, B.n, B.max_px, d_rays, d_hits); });
    if (rc) break;
    if (d_albedo) rc = timed(&acc.resolve_ms, [&]() { return launch_aov_albedo(st, S, bp, tiles, B.n, B.max_px, d_hits); });
    if (rc) break;
    if (matte) rc = timed(&acc.resolve_ms, [&]() { return launch_aov_matte(st, S.instances, mrp, mp, tiles, B.n, B.max_px, d_suv, d_hits); });
    if (rc) break;
    acc.rays.camera += B.samples;
    acc.trace_launches++; acc.closest_launches++; acc.batches++;
  }
  if (ev_all[1]) (void) hipEventRecord(ev_all[1], st);
  const hipError_t se = hipStreamSynchronize(st);      // (also before the transient buffers go away)
  if (rc == 0 && se == hipSuccess) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev_all[0], ev_all[1]) == hipSuccess) acc.total_ms = ms;
    for (const Span &sp : spans) if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) *sp.bucket += ms;
    acc.trace_ms = acc.closest_ms;
  }
  drop_events();
  if (rc) return fail(FJGPU_ENODEV, who + ": HIP failure: " + hipGetErrorString(rc > 0 ? (hipError_t) rc : hipGetLastError()));
  if (se != hipSuccess) return fail(FJGPU_ENODEV, who + ": stream synchronize: " + hipGetErrorString(se));
  if (stats) {
    DCounters hc;
    HIP_TRY(hipMemcpy(&hc, d_cnt, sizeof(hc), hipMemcpyDeviceToHost));
    acc.nodes_visited = hc.nodes; acc.prims_tested = hc.prims; acc.insts_tested = hc.insts; acc.rays_traced = hc.traced;
    *stats = acc;
  }
  return 0;
}

int fjgpu_render_aov(fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    const fjgpu_aov_buffers *out, void *hip_stream, fjgpu_stats *stats)
{
  if (!sc || !r || !out) return fail(FJGPU_EINVAL, "fjgpu_render_aov: null argument");
  return render_aov_body("fjgpu_render_aov", sc, r, tile_ids, n_tiles, out, nullptr, hip_stream, stats);
}

int fjgpu_render_aov_albedo(fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    const fjgpu_aov_buffers *out, float *d_albedo, void *hip_stream, fjgpu_stats *stats)
{
  if (!sc || !r) return fail(FJGPU_EINVAL, "fjgpu_render_aov_albedo: null argument (scene and render are required)");
  return render_aov_body("fjgpu_render_aov_albedo", sc, r, tile_ids, n_tiles, out, d_albedo, hip_stream, stats);
}

int fjgpu_render_aov_matte(fjgpu_scene *sc, const fj_render_desc *r, const int32_t *tile_ids, int n_tiles,
    const fjgpu_matte_desc *matte, const fjgpu_matte_buffers *out, void *hip_stream, fjgpu_stats *stats)
{
  if (!sc || !r) return fail(FJGPU_EINVAL, "fjgpu_render_aov_matte: null argument (scene and render are required)");
  if (!matte) return fail(FJGPU_EINVAL, "fjgpu_render_aov_matte: null matte description");
  if (!out) return fail(FJGPU_EINVAL, "fjgpu_render_aov_matte: null buffer struct");
  if (!out->ids || !out->coverage) return fail(FJGPU_EINVAL, "fjgpu_render_aov_matte: the ids and coverage buffers are required (NULL pointer)");
  if (matte->key != FJGPU_MATTE_KEY_INSTANCE && matte->key != FJGPU_MATTE_KEY_SHADER)
    return fail(FJGPU_EINVAL, "fjgpu_render_aov_matte: unknown key " + std::to_string(matte->key) + " (FJGPU_MATTE_KEY_INSTANCE or FJGPU_MATTE_KEY_SHADER)");
  if (matte->ranks < 1 || matte->ranks > FJGPU_MATTE_MAX_RANKS)
    return fail(FJGPU_EINVAL, "fjgpu_render_aov_matte: ranks " + std::to_string(matte->ranks) + " outside 1.." + std::to_string(FJGPU_MATTE_MAX_RANKS));
  const MatteCall mc{matte, out};
  return render_aov_body("fjgpu_render_aov_matte", sc, r, tile_ids, n_tiles, nullptr, nullptr, hip_stream, stats, &mc);
}

int fjgpu_camera_samples(fjgpu_scene *sc, const fj_render_desc *r, int tile_id, double *rays8, int cap)
{
  if (!sc || !r || (!rays8 && cap > 0) || cap < 0) return fail(FJGPU_EINVAL, "fjgpu_camera_samples: null argument");
  AovSetup A;
  if (const int e = aov_setup(sc, r, "fjgpu_camera_samples", &A)) return e;
  if (tile_id < 0 || tile_id >= (int) A.all.size()) return fail(FJGPU_EINVAL, "tile id out of range");
  const TileDesc d = fixed_grid_tile(sc, r, A.all[tile_id], A.margin, 0);
  const size_t n = (size_t) d.nx * (size_t) d.ny;
  if (n > 0x7fffffffu) return fail(FJGPU_EINVAL, "fjgpu_camera_samples: a tile of more than 2^31 samples");
  if (cap == 0) return (int) n;
  HIP_TRY(hipSetDevice(sc->device));
  DeviceBuffers W;
  double *d_suv; DRay *d_rays; DPath *d_paths;
  const double *d_jit = nullptr; const TileDesc *d_tile = nullptr;
  std::vector<double> draws;
  fjgpu::XorShiftTableSeeded((unsigned) sc->sampler_seed, 2 * n, &draws);
  if (W.alloc(n * 2, &d_suv) || W.alloc(n, &d_rays) || W.alloc(n, &d_paths) || W.upload(draws.data(), 2 * n, &d_jit) || W.upload(&d, 1, &d_tile))
    return fail(FJGPU_ENOMEM, "fjgpu_camera_samples: device allocation failed");
  DScene S = A.S;
  S.time_tab = d_jit;
  const int le = launch_gen_camera(nullptr, S, A.gp, d_tile, 1, (uint32_t) n, d_jit, d_jit, d_suv, d_rays, d_paths);
  if (le) return fail(FJGPU_ENODEV, std::string("fjgpu_camera_samples: launch: ") + hipGetErrorString((hipError_t) le));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<DRay> h(n);
  HIP_TRY(hipMemcpy(h.data(), d_rays, sizeof(DRay) * n, hipMemcpyDeviceToHost));
  const size_t m = std::min(n, (size_t) cap);
  for (size_t i = 0; i < m; i++) {
    for (int k = 0; k < 3; k++) { rays8[8 * i + k] = h[i].o[k]; rays8[8 * i + 3 + k] = h[i].d[k]; }
    rays8[8 * i + 6] = S.cam_znear; rays8[8 * i + 7] = S.cam_zfar;      // the range of a camera ray (Camera::GetRay, src/fj_camera.cc:105-106)
  }
  return (int) n;
}

// ---- camera of a resident scene.  Host state only: the four fields every render call copies into its launch parameters.
int fjgpu_scene_get_camera(const fjgpu_scene *sc, fj_camera_desc *out)
{
  if (!sc || !out) return fail(FJGPU_EINVAL, "fjgpu_scene_get_camera: null argument");
  *out = sc->camera;
  return 0;
}

int fjgpu_scene_set_camera(fjgpu_scene *sc, const fj_camera_desc *camera)
{
  if (!sc || !camera) return fail(FJGPU_EINVAL, "fjgpu_scene_set_camera: null argument");
  const fj_xform_desc &cx = camera->xform;
  for (const int cnt : {cx.n_translate, cx.n_rotate, cx.n_scale})
    if (cnt < 1 || cnt > FJ_MAX_XFORM_SAMPLES) return fail(FJGPU_EINVAL, "fjgpu_scene_set_camera: camera transform sample count out of range");
  if (cx.n_translate != 1 || cx.n_rotate != 1 || cx.n_scale != 1)
    return fail(FJGPU_EUNSUPPORTED, "fjgpu_scene_set_camera: a time-sampled camera is not supported (static cameras only)");
  if (sc->S.cam_xform)
    return fail(FJGPU_EUNSUPPORTED, "fjgpu_scene_set_camera: the scene was created with a time-sampled camera (its buffers and random streams were sized for that)");
  // what BuildHostScene derives from desc->camera and upload_scene copies, with the same statements
  double M[16], Minv[16];
  fjgpu::MakeTransform(cx, 0, M, Minv);
  std::memcpy(sc->S.cam_M, M, sizeof(sc->S.cam_M));
  sc->S.cam_znear = camera->znear;
  sc->S.cam_zfar = camera->zfar;
  sc->cam_fov = camera->fov;
  sc->camera = *camera;
  return 0;
}

int fjgpu_scene_view(const fjgpu_scene *sc, const fj_render_desc *r, fjgpu_view *out)
{
  if (!sc || !r || !out) return fail(FJGPU_EINVAL, "fjgpu_scene_view: null argument");
  if (r->sampler_type == 1) return fail(FJGPU_EUNSUPPORTED, "fjgpu_scene_view: the adaptive sampler is not supported (fixed-grid sampler only)");
  if (r->sampler_type != 0) return fail(FJGPU_EINVAL, "unknown sampler_type");
  if (const char *why = bad_render(r)) return fail(FJGPU_EINVAL, why);
  if (sc->S.cam_xform) return fail(FJGPU_EUNSUPPORTED, "fjgpu_scene_view: a time-sampled camera is not supported (static cameras only)");
  if (sc->S.has_motion) return fail(FJGPU_EUNSUPPORTED, "fjgpu_scene_view: a scene with motion (time-sampled transforms or vertex velocities) is not supported (static scenes only)");
  double M[16], Minv[16];
  fjgpu::MakeTransform(sc->camera.xform, 0, M, Minv);
  std::memcpy(out->world_to_camera, Minv, sizeof(out->world_to_camera));
  camera_uv_size(sc->cam_fov, r, out->uv_size);
  out->xres = r->xres; out->yres = r->yres;
  return 0;
}

}  // extern "C"
