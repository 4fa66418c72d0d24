// light_hull_host.cc -- validation tool: the per-light hull cones of the light loop (device/fjgpu_light_hull.h, the SAME source the kernels
// and the scene upload compile) built for the host, so that tests/test_light_hull_cpu.py can hold their verdicts against the oracle's trace of
// the occluder without a GPU.  Not part of the product path.
#include <math.h>
#include <stdint.h>
#include <vector>
#include "fjgpu_light_hull.h"

extern "C" {

int fj_light_hull_record_bytes(void) { return (int) sizeof(DLightCone); }

// One record per light: Pl [nl][3]; the mesh's object-space vertices v [nv][3] and the instance's matrix M (3 x 4, rows) -- the world images
// are M v in FP64 as the scene upload computes them --; box [6]: the group's reference box.  Returns the number of records with planes.
int fj_light_hull_build_batch(int64_t nl, const double *Pl, int64_t nv, const double *v, const double *M, const double *box, DLightCone *out)
{
  std::vector<double> P((size_t) (nv > 0 ? nv : 0) * 3);
  for (int64_t i = 0; i < nv; i++) light_hull_world(M, v + 3 * i, &P[3 * (size_t) i]);
  int built = 0;
  for (int64_t l = 0; l < nl; l++) built += light_hull_build(Pl + 3 * l, P.data(), nv, box, &out[l]) > 0;
  return built;
}

// Pair i is (record hull_of[i], its light's position Pl[hull_of[i]], surface point Ps[i]).  out [n]: 1 = settled (unoccluded), 0 = not decided.
// Ln = Pl - Ps; normalise != 0: divided by its length with the light loop's statements first (what k_shadow_cull hands to the test).
void fj_light_hull_test_batch(int64_t n, const DLightCone *hulls, const double *Pl, const int32_t *hull_of, const double *Ps, int normalise, int8_t *out)
{
  for (int64_t i = 0; i < n; i++) {
    const DLightCone &C = hulls[hull_of[i]];
    const double *pl = Pl + 3 * (int64_t) hull_of[i], *ps = Ps + 3 * i;
    double lx = pl[0] - ps[0], ly = pl[1] - ps[1], lz = pl[2] - ps[2];
    if (normalise) {
      const double distance = sqrt(lx * lx + ly * ly + lz * lz);
      if (distance > 0) { const double inv = 1. / distance; lx *= inv; ly *= inv; lz *= inv; }
    }
    out[i] = (int8_t) (C.count > 0 && light_cone_usable(C.reach, ps, lx, ly, lz) && light_cone_sure_miss(C, lx, ly, lz));
  }
}

}
