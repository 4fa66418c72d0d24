// fjgpu_light_hull.h -- per-light HULL cones: which surface points' rays to a FIXED light position can touch a FIXED occluder mesh.
//
// The box cones of fjgpu_light_cone.h settle the (surface point Ps, light Pl) pairs whose segment misses the reference BOX of the shadow group's
// one instance.  That box is the world box of a rotated mesh and loose: on the headline frame 193 M pairs pass it, are queued and walked, and
// most of them pass beside the mesh.  All of the occluder's geometry, seen from Pl, lies inside a convex cone with apex Pl; a point outside one
// plane of that cone cannot be shadowed by the occluder.  The record is a DLightCone (six unit normals of planes through Pl, a reach, a count)
// and the verdict is the box cones' (light_cone_plane_out with light_cone_margin): per pair a few dot products with wave-uniform normals.
//
// Build, once per (single-instance static mesh group, point light sample), from the world images w_i = M v_i - Pl of ALL vertices of the mesh:
//   axis c = normalize(centroid of M v_i - Pl), a and b complete the frame;
//   every vertex must have c . w >= gap > 0 (gap = the smallest c . w: a lower bound of the distance from Pl to the hull), and gap obeys the
//     box cones' rules against ext = the largest |coordinate| of the group's box and Pl: gap >= FJ_LC_MIN_GAP ext, gap <= FJ_LC_MAX_DIST box
//     diagonals; reach = FJ_LC_REACH gap - ext.  A light in or near the hull, level with it (vertices behind the axis plane) or too far: no record;
//   six in-plane directions e_j = cos(j 60deg) a + sin(j 60deg) b, s_j = max_i (e_j . w_i) / (c . w_i), plane normal normalize(e_j - s_j' c) with
//     s_j' = s_j + FJ_LH_PUSH (1 + s_j^2) (the plane pushed outward: every vertex is inside it by about FJ_LH_PUSH of its distance from Pl);
//   stored in the order 0, 2, 4, 1, 3, 5: the light loop's first trip of four planes settles everything outside the enclosing triangle;
//   VERIFY: a second pass over all vertices with the finished normals, n_j . w_i <= -FJ_LH_SLACK |w_i|_1 for every plane.  A plane that fails is
//     widened (its push times 16) and the pass repeated, at most FJ_LH_WIDENINGS times; then the record is dropped.  The contract rests on this
//     pass and not on the rounding of the first.
//
// CONTRACT, one-sided: a verdict (some plane j with n_j . (Ps - Pl) > 1e-9 |Ln|_1, Ln = Pl - Ps or its normalised form; direction without a zero
// component, point within reach -- light_cone_usable) implies that the reference finds no triangle of the instance on the ray the light loop
// builds: direction normalize(Pl - Ps), range 1e-4 .. |Pl - Ps|, TriRayIntersect in object space after Minv.  Nothing is said of the other verdict.
//
// Derivation, with u = Ln / |Ln|, D = |Ln|, P(t) = Ps + t u, Pl = P(D), as in fjgpu_light_cone.h.
//  (a) Exact arithmetic.  Every point X of every triangle is a convex combination of vertices, so n_j . (X - Pl) <= 0 and c . (X - Pl) >= gap.
//      The verdict says n_j . (P(t) - Pl) = (D - t) c_j with c_j = -n_j . u > 1e-9: on t <= D the ray is outside plane j by more than 1e-9 of
//      its distance from the light, and a point of the ray within r of Pl is farther than gap - r from every triangle.
//  (b) What the reference computes.  It carries origin and direction to object space with Minv and tests the object-space triangle; read in
//      world space that is an exact test of a triangle whose vertices moved by the roundings of M v (the build's), of Minv (o, d) and of the
//      test's own products: E = a few 2^-53 (|Ps|inf + ext), times the condition of M for the object-space part -- for the transforms a scene
//      description produces seven orders below the 1e-9 margin.  The rounded ray leaves the true one by 2^-52 t.
//  (c) Together, exactly as the box cones' (c): the ray is outside the moved triangles wherever the true ray is outside plane j by more than E,
//      that is on t <= D - r with r = 1e9 E; the rest of the range lies within r + E of Pl while the triangles stay gap - E away, and the rules
//      gap >= 1e-3 ext, |Ps|inf <= reach = 2e4 gap - ext give r <= 0.0164 gap.  No hit in [1e-4, D]: the pair is unoccluded.
//  (d) The reference's instance box plays no part: a ray that misses it is unoccluded, one that passes it finds no triangle -- unoccluded
//      either way, including the mirrored boxes of negative scales.
//
// tests/test_light_hull_cpu.py compiles THIS file for the host (tools/light_hull_host.cc) and holds it against the oracle's scene trace; a
// -DFJ_LIGHT_HULL_VALIDATE build of the kernels walks every settled pair of whole frames and counts the walks that find a hit.
#ifndef FJGPU_LIGHT_HULL_H
#define FJGPU_LIGHT_HULL_H

#include "fjgpu_light_cone.h"

#define FJ_LH_PLANES 6
#define FJ_LH_PUSH 1e-9           // a plane's tangent is pushed outward by this times (1 + s^2)
#define FJ_LH_SLACK 1e-12         // the verify pass: every vertex inside every plane by this fraction of |w|_1
#define FJ_LH_WIDENINGS 3         // a plane that fails the verify pass is widened (push x 16) this many times before the record is dropped

// the frame of one light and what the first vertex pass gathers
struct LightHullAcc {
  double Pl[3], c[3], e[FJ_LH_PLANES][3];   // apex, axis, the six in-plane directions
  double s[FJ_LH_PLANES];                   // max (e_j . w) / (c . w)
  double gap;                               // min c . w
  double push[FJ_LH_PLANES];                // the outward push of plane j (widened by the verify pass)
  int32_t ok;                               // 0: no record (degenerate frame, a vertex not in front of the axis plane, not finite)
  int32_t pad;
};

// world image of an object-space vertex: rows of M (DInstance.M, 3 x 4)
FJ_LC_FN void light_hull_world(const double *M, const double *v, double *w)
{
  for (int a = 0; a < 3; a++) w[a] = M[4 * a] * v[0] + M[4 * a + 1] * v[1] + M[4 * a + 2] * v[2] + M[4 * a + 3];
}

// axis from Pl to the vertex centroid, and the six directions
FJ_LC_FN void light_hull_frame(const double *Pl, const double *centroid, LightHullAcc *A)
{
  for (int j = 0; j < FJ_LH_PLANES; j++) { A->s[j] = -1e300; A->push[j] = FJ_LH_PUSH; A->e[j][0] = A->e[j][1] = A->e[j][2] = 0.; }
  A->gap = 1e300; A->ok = 0; A->pad = 0;
  double c[3] = {centroid[0] - Pl[0], centroid[1] - Pl[1], centroid[2] - Pl[2]};
  for (int k = 0; k < 3; k++) { A->Pl[k] = Pl[k]; A->c[k] = 0.; }
  const double m = lc_max(lc_max(lc_abs(c[0]), lc_abs(c[1])), lc_abs(c[2]));
  if (!(m > 0.) || !(m < 1e300)) return;
  for (int k = 0; k < 3; k++) c[k] /= m;
  const double len = __builtin_sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  for (int k = 0; k < 3; k++) c[k] /= len;
  // a: the coordinate axis of c's smallest component, made orthogonal to c; b = c x a
  int k0 = 0;
  if (lc_abs(c[1]) < lc_abs(c[k0])) k0 = 1;
  if (lc_abs(c[2]) < lc_abs(c[k0])) k0 = 2;
  double a[3] = {0., 0., 0.};
  a[k0] = 1.;
  const double ca = c[k0];
  for (int k = 0; k < 3; k++) a[k] -= ca * c[k];
  const double la = __builtin_sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  if (!(la > 0.)) return;
  for (int k = 0; k < 3; k++) a[k] /= la;
  const double b[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
  const double h = .86602540378443864676;     // sin 60deg
  const double cs[FJ_LH_PLANES] = {1., .5, -.5, -1., -.5, .5}, sn[FJ_LH_PLANES] = {0., h, h, 0., -h, -h};
  for (int j = 0; j < FJ_LH_PLANES; j++) for (int k = 0; k < 3; k++) A->e[j][k] = cs[j] * a[k] + sn[j] * b[k];
  for (int k = 0; k < 3; k++) A->c[k] = c[k];
  A->ok = 1;
}

// first pass, one world vertex P = M v.  (The frame is not exactly orthonormal and need not be: the verify pass is the proof.)
FJ_LC_FN void light_hull_add(LightHullAcc *A, const double *P)
{
  const double w[3] = {P[0] - A->Pl[0], P[1] - A->Pl[1], P[2] - A->Pl[2]};
  const double cw = A->c[0] * w[0] + A->c[1] * w[1] + A->c[2] * w[2];
  if (!(cw > 0.) || !(cw < 1e300)) { A->ok = 0; return; }
  if (cw < A->gap) A->gap = cw;
  const double inv = 1. / cw;
  for (int j = 0; j < FJ_LH_PLANES; j++) {
    const double t = (A->e[j][0] * w[0] + A->e[j][1] * w[1] + A->e[j][2] * w[2]) * inv;
    if (t > A->s[j]) A->s[j] = t;
  }
}
// two accumulators of one frame (vertex ranges gathered by different threads)
FJ_LC_FN void light_hull_merge(LightHullAcc *A, const LightHullAcc *B)
{
  if (!B->ok) A->ok = 0;
  if (B->gap < A->gap) A->gap = B->gap;
  for (int j = 0; j < FJ_LH_PLANES; j++) if (B->s[j] > A->s[j]) A->s[j] = B->s[j];
}

// The record after the first pass (and again after a widening): the rules on gap, the planes in the order 0, 2, 4, 1, 3, 5.  b[6]: the group's
// reference box (min xyz, max xyz), the scale the rules are written against.  Returns the plane count (0: no record).
FJ_LC_FN int light_hull_finish(const LightHullAcc *A, const double *b, DLightCone *out)
{
  for (int j = 0; j < FJ_LC_MAX_PLANES; j++) out->n[j][0] = out->n[j][1] = out->n[j][2] = 0.;
  out->reach = 0.; out->count = 0; out->pad = 0;
  if (!A->ok) return 0;
  double ext = 0.;
  for (int k = 0; k < 6; k++) ext = lc_max(ext, lc_abs(b[k]));
  for (int k = 0; k < 3; k++) ext = lc_max(ext, lc_abs(A->Pl[k]));
  if (!(ext > 0.) || !(ext < 1e300)) return 0;
  const double dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
  const double diag = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
  const double gap = A->gap;
  if (!(gap >= FJ_LC_MIN_GAP * ext) || !(gap <= FJ_LC_MAX_DIST * diag)) return 0;
  const int order[FJ_LH_PLANES] = {0, 2, 4, 1, 3, 5};
  for (int q = 0; q < FJ_LH_PLANES; q++) {
    const int j = order[q];
    const double s = A->s[j];
    if (!(s > -1e150) || !(s < 1e150)) { for (int i = 0; i < FJ_LC_MAX_PLANES; i++) out->n[i][0] = out->n[i][1] = out->n[i][2] = 0.; return 0; }
    const double sp = s + A->push[j] * (1. + s * s);
    double n[3] = {A->e[j][0] - sp * A->c[0], A->e[j][1] - sp * A->c[1], A->e[j][2] - sp * A->c[2]};
    const double m = lc_max(lc_max(lc_abs(n[0]), lc_abs(n[1])), lc_abs(n[2]));
    if (!(m > 0.)) { for (int i = 0; i < FJ_LC_MAX_PLANES; i++) out->n[i][0] = out->n[i][1] = out->n[i][2] = 0.; return 0; }
    for (int k = 0; k < 3; k++) n[k] /= m;
    const double inv = 1. / __builtin_sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    out->n[q][0] = n[0] * inv; out->n[q][1] = n[1] * inv; out->n[q][2] = n[2] * inv;
  }
  out->count = FJ_LH_PLANES;
  out->reach = FJ_LC_REACH * gap - ext;
  return FJ_LH_PLANES;
}

// verify pass, one world vertex: bit q set = stored plane q does NOT hold the vertex with the slack
FJ_LC_FN uint32_t light_hull_verify(const DLightCone *C, const double *Pl, const double *P)
{
  const double w[3] = {P[0] - Pl[0], P[1] - Pl[1], P[2] - Pl[2]};
  const double lim = -FJ_LH_SLACK * ((lc_abs(w[0]) + lc_abs(w[1])) + lc_abs(w[2]));
  uint32_t bad = 0;
  for (int q = 0; q < FJ_LH_PLANES; q++)
    if (!(C->n[q][0] * w[0] + C->n[q][1] * w[1] + C->n[q][2] * w[2] <= lim)) bad |= 1u << q;
  return bad;
}
// the planes of a verify mask get a wider push (stored plane q is direction order[q])
FJ_LC_FN void light_hull_widen(LightHullAcc *A, uint32_t bad)
{
  const int order[FJ_LH_PLANES] = {0, 2, 4, 1, 3, 5};
  for (int q = 0; q < FJ_LH_PLANES; q++) if (bad & (1u << q)) A->push[order[q]] *= 16.;
}

// The whole build in one thread: world vertices P [n][3].  (The scene upload runs the same functions over vertex ranges on worker threads.)
FJ_LC_FN int light_hull_build(const double *Pl, const double *P, int64_t n, const double *b, DLightCone *out)
{
  for (int j = 0; j < FJ_LC_MAX_PLANES; j++) out->n[j][0] = out->n[j][1] = out->n[j][2] = 0.;
  out->reach = 0.; out->count = 0; out->pad = 0;
  if (n <= 0) return 0;
  double ctr[3] = {0., 0., 0.};
  for (int64_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) ctr[k] += P[3 * i + k];
  for (int k = 0; k < 3; k++) ctr[k] /= (double) n;
  LightHullAcc A;
  light_hull_frame(Pl, ctr, &A);
  for (int64_t i = 0; i < n && A.ok; i++) light_hull_add(&A, P + 3 * i);
  for (int round = 0; round <= FJ_LH_WIDENINGS; round++) {
    if (!light_hull_finish(&A, b, out)) return 0;
    uint32_t bad = 0;
    for (int64_t i = 0; i < n; i++) bad |= light_hull_verify(out, Pl, P + 3 * i);
    if (!bad) return out->count;
    light_hull_widen(&A, bad);
  }
  for (int j = 0; j < FJ_LC_MAX_PLANES; j++) out->n[j][0] = out->n[j][1] = out->n[j][2] = 0.;
  out->reach = 0.; out->count = 0;
  return 0;
}

#endif
