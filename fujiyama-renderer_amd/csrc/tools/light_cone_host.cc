// light_cone_host.cc -- validation tool: the per-light shadow cones of the light loop (device/fjgpu_light_cone.h, the SAME source the
// kernels and the scene upload compile) built for the host, so that tests/test_light_cone_cpu.py can hold their verdicts against the
// reference's box test on millions of (point, light, box) triples without a GPU.  Not part of the product path.
#include <math.h>
#include <stdint.h>
#include "fjgpu_light_cone.h"

extern "C" {

int fj_light_cone_record_bytes(void) { return (int) sizeof(DLightCone); }

// Pl [n][3], box [n][6] (min xyz, max xyz) -> cones [n]
void fj_light_cone_build_batch(int64_t n, const double *Pl, const double *box, DLightCone *cones)
{
  for (int64_t i = 0; i < n; i++) light_cone_build(Pl + 3 * i, box + 6 * i, &cones[i]);
}

// Pair i is (cone cone_of[i], its light's position Pl[cone_of[i]], surface point Ps[i]).  out [n]: 1 = surely misses, 0 = not decided by the
// cone.  Ln = Pl - Ps; normalise != 0: divided by its length with the light loop's statements first (what k_shadow_cull hands to the test).
void fj_light_cone_test_batch(int64_t n, const DLightCone *cones, const double *Pl, const int32_t *cone_of, const double *Ps, int normalise, int8_t *out)
{
  for (int64_t i = 0; i < n; i++) {
    const DLightCone &C = cones[cone_of[i]];
    const double *pl = Pl + 3 * (int64_t) cone_of[i], *ps = Ps + 3 * i;
    double lx = pl[0] - ps[0], ly = pl[1] - ps[1], lz = pl[2] - ps[2];
    if (normalise) {
      const double distance = sqrt(lx * lx + ly * ly + lz * lz);
      if (distance > 0) { const double inv = 1. / distance; lx *= inv; ly *= inv; lz *= inv; }
    }
    out[i] = (int8_t) (C.count > 0 && light_cone_usable(C.reach, ps, lx, ly, lz) && light_cone_sure_miss(C, lx, ly, lz));
  }
}

}
