// fjgpu_light_cone.h -- per-light shadow cones: which surface points' rays to a FIXED light position can touch a FIXED box.
//
// The light loop (k_shadow_cull, fjgpu_dev_shadow.h) asks, for every (surface point Ps, light sample l) pair, whether the ray from Ps to the
// light's position Pl passes the reference box of the shadow group's one instance (BoxRayIntersect, reference src/fj_box.cc:73-138, restated
// as box_ray_ref in fjgpu_dev_math.h).  On the headline frame 2.15 G of 2.55 G pairs miss it.  Box and Pl are scene constants (DGroup.sbounds;
// DLightSample.P of a point or dome light), so the set of points whose segment to Pl can touch the box is worked out ONCE per (single-instance
// group, light sample): it lies inside the convex cone with apex Pl through the box's silhouette -- at most six planes through Pl.  Per pair that
// leaves dot products of Ln = Pl - Ps with wave-uniform normals, no reciprocal and no per-lane state.
//
// Verdict (light_cone_sure_miss): "surely misses" iff for some plane j
//     n_j . (Ps - Pl)  >  1e-9 (|Ln.x| + |Ln.y| + |Ln.z|)
// n_j unit length, the box on its non-positive side.  The test is homogeneous in Ln (the normalised direction serves as well as Pl - Ps) and
// the margin purely relative.  The caller uses the verdict only for a direction without a zero component (plain_dir: no negative zero either)
// and for a point within the record's `reach` (below); everything else takes the exact path.
//
// CONTRACT, one-sided: a "surely misses" verdict implies that box_ray_ref(box, Ps, normalize(Ln), 1e-4, |Ln|) returns false.  Nothing is said
// of the other verdict.  tests/test_light_cone_cpu.py compiles THIS file for the host (tools/light_cone_host.cc) and holds it against the
// oracle's pinned box test; a -DFJ_LIGHT_CONE_VALIDATE build of the kernels runs the exact test behind every verdict of whole frames.
//
// Derivation.  Write u = Ln / |Ln|, D = |Ln|, so that the ray is P(t) = Ps + t u and Pl = P(D).
//  (a) Geometry, exact arithmetic.  Every box point X has n_j . (X - Pl) <= 0 for every plane.  With c = -n_j . u the verdict says
//      c > 1e-9 (|u.x| + |u.y| + |u.z|) >= 1e-9, and n_j . (P(t) - Pl) = (D - t) c: on t <= D the ray is OUTSIDE plane j by (D - t) c, i.e. by
//      more than 1e-9 of its distance from the light.  Beyond the light (t > D) the line may enter the box, no sooner than at t = D + gap, gap =
//      the distance from Pl to the box.
//  (b) What the reference computes.  Each of its six slab bounds is (b - o) / d: one subtraction, one division, on a direction whose components
//      carry the rounding of 1 / D and a product.  A computed bound t' = t (1 + e), |e| <= 4 x 2^-53, is the EXACT bound of the plane moved to
//      b' with b' - o = (b - o)(1 + e): the reference's comparisons are exact comparisons of exact bounds of a box B' whose faces lie within
//      e (|Ps|inf + |box|inf) of the box's, against the line through Ps with the rounded direction u', which leaves the true line by at most
//      2^-52 t at parameter t.  Overflow to +-inf (a component of u' near zero) is the bound of a plane at infinity: the same argument.  A zero
//      component (0 x inf, the -0 quirk) is kept out by the caller.
//  (c) Together.  With E = 4 x 2^-53 (|Ps|inf + |box|inf) + 2^-52 D the rounded line stays outside B' wherever the true ray is outside plane j
//      by more than E: on t <= D - r, r = 1e9 E.  For D - r < t < D + gap - r it is within r + E of Pl, and B' no nearer than gap - E.  So if
//      gap > 2 r the reference's slab interval is empty or starts beyond its `ray_tmax` = fl(D) <= D (1 + 2^-52): it returns false.
//      r <= 1e9 x 8.2e-16 (|Ps|inf + ext) with ext = max(|box|inf, |Pl|inf) and D <= sqrt(3) (|Ps|inf + ext); the build function admits a cone
//      only where gap >= 1e-3 ext and sets reach = 2e4 gap - ext, so a point with |Ps|inf <= reach has r <= 0.0164 gap: a factor of 30 to spare.
//      (The unit normals and the dot products are themselves good to a few 2^-53 of their terms, seven orders below the 1e-9 margin.)
//
// Build (light_cone_build): ext = the largest |coordinate| of box and Pl; per axis Pl is beyond the max face, beyond the min face or strictly
// between the faces, each by more than 1e-9 ext -- anything else is ambiguous and gives no cone, as does a light between the faces on all
// three axes.  An edge is a silhouette edge iff exactly one of its two faces faces Pl; its plane's normal is normalize(cross(p0 - Pl, p1 - Pl)),
// evaluated as cross(p0 - Pl, p1 - p0) with p1 - p0 along one axis (two components of p0 - Pl: no cancellation for an edge that looks short
// from the light), oriented so that the box's centre is on the negative side.  Four or six planes, in an order that lets the first four
// settle nearly every pair (below).
//
// The margin and the two guards cost nothing where it matters: a light nearer to the box than a thousandth of the scene's size, or a point
// tens of thousands of box distances away, takes the exact test it always took.
#ifndef FJGPU_LIGHT_CONE_H
#define FJGPU_LIGHT_CONE_H

#include <stdint.h>

#ifdef __HIPCC__
#define FJ_LC_FN __host__ __device__ __forceinline__
#else
#define FJ_LC_FN static inline
#endif

#define FJ_LC_MAX_PLANES 6
#define FJ_LC_MARGIN 1e-9         // relative margin of the verdict, and of the classification of Pl against the face planes
#define FJ_LC_MIN_GAP 1e-3        // a cone is built only where the light is at least this fraction of `ext` away from the box
#define FJ_LC_REACH 2e4           // reach = FJ_LC_REACH * gap - ext (derivation (c))
#define FJ_LC_MAX_DIST 1e5        // ... and no farther than this many box diagonals: beyond, the 1e-9 margin is wider than the box and decides nothing

// one (single-instance group, light sample) pair; 160 bytes.  count == 0: no cone, always take the exact test
struct DLightCone {
  double n[FJ_LC_MAX_PLANES][3];   // unit normals of planes through the light's position, the box on the non-positive side
  double reach;                    // the verdict holds for points with max |coordinate| <= reach.  In the device table: the smallest reach of the
                                   // row's cones, the same value in every record of the row (the light loop reads it once per wave iteration)
  int32_t count;                   // planes in use
  int32_t pad;
};
static_assert(sizeof(DLightCone) == 160 && sizeof(DLightCone) % 16 == 0, "DLightCone layout");

FJ_LC_FN double lc_abs(double x) { return __builtin_fabs(x); }
FJ_LC_FN double lc_max(double a, double b) { return a > b ? a : b; }

// The cone of the box b[6] = (min xyz, max xyz) seen from Pl.  Returns the plane count (0: no cone).
FJ_LC_FN int light_cone_build(const double *Pl, const double *b, DLightCone *out)
{
  for (int j = 0; j < FJ_LC_MAX_PLANES; j++) out->n[j][0] = out->n[j][1] = out->n[j][2] = 0.;
  out->reach = 0.; out->count = 0; out->pad = 0;
  double ext = 0.;
  for (int k = 0; k < 6; k++) ext = lc_max(ext, lc_abs(b[k]));
  for (int k = 0; k < 3; k++) ext = lc_max(ext, lc_abs(Pl[k]));
  if (!(ext > 0.) || !(ext < 1e300)) return 0;            // (NaN, inf, everything at the origin)
  for (int k = 0; k < 3; k++) if (!(b[k] < b[3 + k])) return 0;      // a flat or inverted box has no silhouette to speak of
  const double delta = FJ_LC_MARGIN * ext;
  // side[k]: +1 beyond the max face, -1 beyond the min face, 0 strictly between the faces (each by more than delta); else ambiguous
  int side[3];
  double gap2 = 0.;
  for (int k = 0; k < 3; k++) {
    if (Pl[k] > b[3 + k] + delta) { side[k] = 1; const double g = Pl[k] - b[3 + k]; gap2 += g * g; }
    else if (Pl[k] < b[k] - delta) { side[k] = -1; const double g = b[k] - Pl[k]; gap2 += g * g; }
    else if (Pl[k] > b[k] + delta && Pl[k] < b[3 + k] - delta) side[k] = 0;
    else return 0;
  }
  if (side[0] == 0 && side[1] == 0 && side[2] == 0) return 0;         // the light is in the box
  const double gap = __builtin_sqrt(gap2);                            // distance from Pl to the box
  const double dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
  const double diag = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
  if (!(gap >= FJ_LC_MIN_GAP * ext) || !(gap <= FJ_LC_MAX_DIST * diag)) return 0;
  const double ctr[3] = {.5 * (b[0] + b[3]), .5 * (b[1] + b[4]), .5 * (b[2] + b[5])};
  // The twelve edges: edge (a, s1, s2) runs along axis a at the min (0) / max (1) faces of the two other axes a1 < a2, from corner c0 to corner
  // c1 (bit k of a corner: 0 = min, 1 = max on axis k).  Its adjacent faces are (a1, s1) and (a2, s2); face (k, max) faces Pl iff side[k] > 0,
  // face (k, min) iff side[k] < 0.  Silhouette: exactly one of the two does.
  int ec0[FJ_LC_MAX_PLANES], ec1[FJ_LC_MAX_PLANES], n_edges = 0;
  for (int a = 0; a < 3; a++) {
    const int a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;
    for (int s1 = 0; s1 < 2; s1++)
      for (int s2 = 0; s2 < 2; s2++) {
        const bool f1 = s1 ? side[a1] > 0 : side[a1] < 0;
        const bool f2 = s2 ? side[a2] > 0 : side[a2] < 0;
        if (f1 == f2) continue;
        if (n_edges == FJ_LC_MAX_PLANES) return 0;          // (cannot happen: a box's silhouette has four or six edges)
        ec0[n_edges] = (s1 << a1) | (s2 << a2); ec1[n_edges] = ec0[n_edges] | (1 << a);
        n_edges++;
      }
  }
  // The silhouette is one closed loop: put the edges in the order of a walk around it, then -- six edges -- every second one first.  The light
  // loop evaluates the planes four at a time: a point that is inside planes 0, 2, 4 of a hexagonal cone lies in it or in one of three small
  // wedges beside it, so the second trip (planes 1, 3, 5 in walk order) is rare; a four-sided cone is settled in one trip.
  int order[FJ_LC_MAX_PLANES];
  {
    bool used[FJ_LC_MAX_PLANES] = {false, false, false, false, false, false};
    int at = 0, corner = ec1[0], walk[FJ_LC_MAX_PLANES];
    for (int k = 0; k < n_edges; k++) {
      walk[k] = at; used[at] = true;
      int nx = -1;
      for (int e = 0; e < n_edges && nx < 0; e++) if (!used[e] && (ec0[e] == corner || ec1[e] == corner)) nx = e;
      if (nx < 0) { if (k + 1 < n_edges) return 0; break; }                 // (cannot happen: the loop closes after the last edge)
      corner = ec0[nx] == corner ? ec1[nx] : ec0[nx];
      at = nx;
    }
    if (n_edges == 6) { order[0] = walk[0]; order[1] = walk[2]; order[2] = walk[4]; order[3] = walk[1]; order[4] = walk[3]; order[5] = walk[5]; }
    else for (int k = 0; k < n_edges; k++) order[k] = walk[k];
  }
  int count = 0;
  for (int k = 0; k < n_edges; k++) {
    // normalize(cross(p0 - Pl, p1 - Pl)) = normalize(cross(p0 - Pl, p1 - p0)), and p1 - p0 runs along axis a: the product is two components of
    // p0 - Pl, one subtraction each -- no cancellation, however thin the edge looks from the light
    const int c0 = ec0[order[k]], a = (c0 ^ ec1[order[k]]) >> 1;
    const double e0[3] = {b[3 * (c0 & 1)] - Pl[0], b[3 * ((c0 >> 1) & 1) + 1] - Pl[1], b[3 * ((c0 >> 2) & 1) + 2] - Pl[2]};
    const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
    // (scaled first: coordinates may be anything up to 1e300)
    const double sc = 1. / lc_max(lc_max(lc_abs(e0[a1]), lc_abs(e0[a2])), 1e-300);
    double n[3];
    n[a] = 0.; n[a1] = e0[a2] * sc; n[a2] = -(e0[a1] * sc);
    const double len = __builtin_sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(len > 0.)) { for (int j = 0; j < FJ_LC_MAX_PLANES; j++) out->n[j][0] = out->n[j][1] = out->n[j][2] = 0.; return 0; }
    const double inv = 1. / len;
    n[0] *= inv; n[1] *= inv; n[2] *= inv;
    const double c = n[0] * (ctr[0] - Pl[0]) + n[1] * (ctr[1] - Pl[1]) + n[2] * (ctr[2] - Pl[2]);
    if (c > 0.) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
    out->n[count][0] = n[0]; out->n[count][1] = n[1]; out->n[count][2] = n[2];
    count++;
  }
  out->count = count;
  out->reach = FJ_LC_REACH * gap - ext;
  return count;
}

// One plane of the verdict: n . (Ps - Pl) > margin, with Ln = Pl - Ps (or any positive multiple of it) and margin = 1e-9 |Ln|_1.
FJ_LC_FN bool light_cone_plane_out(double nx, double ny, double nz, double lx, double ly, double lz, double margin)
{
  return -__builtin_fma(nz, lz, __builtin_fma(ny, ly, nx * lx)) > margin;
}
FJ_LC_FN double light_cone_margin(double lx, double ly, double lz) { return FJ_LC_MARGIN * ((lc_abs(lx) + lc_abs(ly)) + lc_abs(lz)); }

// The verdict of the planes alone (the caller has checked the direction and the reach: light_cone_usable).
FJ_LC_FN bool light_cone_sure_miss(const DLightCone &C, double lx, double ly, double lz)
{
  const double m = light_cone_margin(lx, ly, lz);
  bool out = false;
  for (int j = 0; j < C.count && j < FJ_LC_MAX_PLANES; j++) out = out || light_cone_plane_out(C.n[j][0], C.n[j][1], C.n[j][2], lx, ly, lz, m);
  return out;
}
// ... and what the caller checks first: no zero component in the direction, the point within reach
FJ_LC_FN bool light_cone_usable(double reach, const double *Ps, double lx, double ly, double lz)
{
  return lx != 0 && ly != 0 && lz != 0 && lc_max(lc_max(lc_abs(Ps[0]), lc_abs(Ps[1])), lc_abs(Ps[2])) <= reach;
}

#endif
