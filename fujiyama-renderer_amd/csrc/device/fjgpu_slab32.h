// fjgpu_slab32.h -- the conservative slab tests of the BLAS walks: the f64 test, the f32 test on f32 node boxes (DNode) and
// the f32 test on 16-bit quantised boxes (DNodeQ), with the quantiser's per-axis arithmetic.
//
// One source for the kernels (fjgpu_dev_math.h includes it; k_trace_closest, _phased, _flat, k_shadow_anyhit, k_shadow_anyhit_curves and
// k_quantize_nodes compile these statements) and for the host: tools/slab32_host.cc builds the same file with the ROCm clang++, so that
// tests/test_slab32_cpu.py can hold every constant, plane value and verdict against exact arithmetic without a GPU, and
// tests/test_gpu_slab32.py can hold the device's results against the host's bit for bit.  The contract is one-sided: whatever the exact
// box test accepts, these accept (for distances |t| <= 1e30, the interval of an axis that never culls).
// On the host the two device builtins have plain stand-ins: v_perm_b32 is a byte select, v_alignbit_b32 a rotate.
#ifndef FJGPU_SLAB32_H
#define FJGPU_SLAB32_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define FJ_S32_FN __device__ __forceinline__
#define FJ_S32_BITS(x) __float_as_uint(x)
#define FJ_S32_FLOAT(x) __uint_as_float(x)
#define FJ_S32_PERM(a, b, sel) __builtin_amdgcn_perm(a, b, sel)
#define FJ_S32_ALIGNBIT(a, b, sh) __builtin_amdgcn_alignbit(a, b, sh)
#else
#define FJ_S32_FN static inline
static inline uint32_t fj_s32_bits(float x) { union { float f; uint32_t u; } c; c.f = x; return c.u; }
static inline float fj_s32_float(uint32_t x) { union { float f; uint32_t u; } c; c.u = x; return c.f; }
// v_perm_b32: result byte k = byte sel_k of the eight bytes {b (0..3), a (4..7)}; selectors 0..7 only (the constant-generating ones are not used)
static inline uint32_t fj_s32_perm(uint32_t a, uint32_t b, uint32_t sel)
{
  const uint64_t src = ((uint64_t) a << 32) | b;
  uint32_t r = 0;
  for (int k = 0; k < 4; k++) r |= (uint32_t) ((src >> (8 * ((sel >> (8 * k)) & 7u))) & 0xffu) << (8 * k);
  return r;
}
// v_alignbit_b32: the low 32 bits of {a, b} >> (sh & 31)
static inline uint32_t fj_s32_alignbit(uint32_t a, uint32_t b, uint32_t sh) { return (uint32_t) ((((uint64_t) a << 32) | b) >> (sh & 31u)); }
#define FJ_S32_BITS(x) fj_s32_bits(x)
#define FJ_S32_FLOAT(x) fj_s32_float(x)
#define FJ_S32_PERM(a, b, sel) fj_s32_perm(a, b, sel)
#define FJ_S32_ALIGNBIT(a, b, sh) fj_s32_alignbit(a, b, sh)
#endif

struct V3 { double x, y, z; };
typedef float fj_v2f __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------ culling tests
// Conservative slab test (culling only).  NaN from 0 * inf is ignored by
// fmin/fmax, which return the non-NaN operand.
FJ_S32_FN bool slab(const double bmin[3], const double bmax[3], V3 o, V3 inv,
    double tmin, double tmax, double *tnear)
{
  const double x0 = (bmin[0] - o.x) * inv.x, x1 = (bmax[0] - o.x) * inv.x;
  const double y0 = (bmin[1] - o.y) * inv.y, y1 = (bmax[1] - o.y) * inv.y;
  const double z0 = (bmin[2] - o.z) * inv.z, z1 = (bmax[2] - o.z) * inv.z;
  const double tn = fmax(fmax(fmin(x0, x1), fmin(y0, y1)), fmax(fmin(z0, z1), tmin));
  const double tf = fmin(fmin(fmax(x0, x1), fmax(y0, y1)), fmin(fmax(z0, z1), tmax));
  *tnear = tn;
  return tn <= tf;
}

// ---- conservative f32 slab test on the BLAS node boxes (culling only).
// DNode stores a child's box as three (min, max) pairs, so one packed fma yields both plane
// distances of an axis.  Per (ray, instance) and axis a the entry code keeps
//   i = (float)(1/od_a),  o = (float)(oo_a/od_a),  e = 3.6e-7 (Bmax_a |i| + |o|),
//   l = -(o + e),  h = e - o,     Bmax_a >= |any box coordinate| of the primitive set.
// For a box plane b (f32) the exact distance is t = (b - oo_a)/od_a.  t~ = fmaf(b, i, -o)
// differs from t by at most |b/od| 2^-24 (rounding of i) + |oo/od| 2^-24 (rounding of o; the
// f64 reciprocal and product before it are good to 2^-49) + |t~| 2^-24 (the fma's rounding)
// <= 2^-23 (Bmax |i| + |o|)(1 + 2^-18) =: E.  e is 3 E; folding it into the addend costs
// another 2^-24 |o + e|, so fmaf(b, i, l) <= t - E' and fmaf(b, i, h) >= t + E' with E' > E:
// [min over the two planes of the l-variant, max of the h-variant] contains the exact slab
// interval, and the f64 interval of slab_f32box (own error ~2^-52).  Whatever the f64 test
// accepts this one accepts: it can only cull less.  An axis whose e is not a finite number
// below 1e30 (direction component zero or denormal: 1/od = inf) gets i = 0, l = -1e30,
// h = 1e30: interval [-1e30, 1e30], it never culls.  With e < 1e30 every product is finite or
// an infinity of one sign: no NaN can arise (box coordinates are finite).
// one axis: t_lo = fmaf(b, i, l), t_hi = fmaf(b, i, h).  (Plain values, no pointers into a
// struct: the compiler kept a by-reference Slab32 in scratch memory.)
struct Slab32Axis { float i, l, h; };
struct Slab32 { Slab32Axis x, y, z; };

// inv = 1/od good to 2^-49 (filter_rcp) or exact
FJ_S32_FN Slab32Axis slab32_axis(double inv, double oo, double bmax_abs)
{
  const float i = (float) inv, o = (float) (oo * inv);
  // (node boxes are rounded outward from the f64 bounds by up to 2 ulp: the factor covers 8)
  const float e = 3.6e-7f * ((float) bmax_abs * 1.000001f * fabsf(i) + fabsf(o));
  const bool ok = e < 1e30f;
  Slab32Axis a;
  a.i = ok ? i : 0.f;
  a.l = ok ? -(o + e) : -1e30f;
  a.h = ok ? e - o : 1e30f;
  return a;
}

// bounds = {min xyz, max xyz} of the primitive set (every node box lies inside)
FJ_S32_FN Slab32 slab32_setup(V3 oo, V3 inv, const double *bounds)
{
  Slab32 s;
  s.x = slab32_axis(inv.x, oo.x, fmax(fabs(bounds[0]), fabs(bounds[3])));
  s.y = slab32_axis(inv.y, oo.y, fmax(fabs(bounds[1]), fabs(bounds[4])));
  s.z = slab32_axis(inv.z, oo.z, fmax(fabs(bounds[2]), fabs(bounds[5])));
  return s;
}

// The same constants for QUANTISED boxes (DNodeQ): a plane is g0 + q cell with q an integer in
// [0, 65535], so t = (g0 + q cell - oo)/od = q (cell/od) + (g0 - oo)/od, and
//   t~ = fmaf((float) q, A, B),  A = (float)(cell/od),  B = (float)((g0 - oo)/od)
// is off by at most 2^-23 (65535 |A| + |B|)(1 + 2^-18) (roundings of A, of B, of the fma; (float) q
// is exact).  i = A, l = B - e, h = B + e with e three times that bound, as above.
//
// FJ_SLAB_PERM (default): the integer reaches the fma WITHOUT a conversion instruction.  A byte permute
// (v_perm_b32) drops the 16-bit coordinate into the mantissa of 2^23: as_float(0x4B000000 | q) IS the
// number 8388608 + q, exactly.  The fma then computes (8388608 + q) A + c' with the shifted addend
// c' = fmaf(-8388608, A, c), c = fl(B -+ e') the addend of the unshifted form with a WIDER margin e' = e + p.  Error budget, every rounding
// counted at its own magnitude:
//   (1) c' is ONE rounding of the exact sum -8388608 A + c, whose magnitude is up to 2^23 |A| + |c| -- NOT that of t.  Its ulp is about |A| when
//       |c| is small against 2^23 |A| (origins within ~100 grid extents) and 2 |A| once c carries the sum over the next power of two; farther out
//       it is 2^-23 |c|.  The rounding costs up to 2^-24 (2^23 |A| + |c|), in either direction.
//   (2) A pad added to c' AFTERWARDS is a second rounding at the same magnitude: below half an ulp of c' it rounds away entirely (an earlier
//       version padded by .51 |A| there and lost planes by up to 0.43 cell for origins 1 to 32 extents away, where ulp(c') = 2 |A| and e,
//       ~3.6e-7 |B|, is only a fraction of |A|).  So the pad goes in BEFORE that rounding, as part of the margin:
//         p = 5.97e-8 (2^23 |A| + |B| + e)     (5.97e-8 = 2^-24 x 1.0016: the three float operations that compute p are good to 2^-22 relative)
//       With |c| <= (|B| + e + p)(1 + 2^-24), the rounding (1) costs at most 2^-24 (2^23 |A| + |c|) <= p.
//   (3) The l side, in exact terms (the h side mirrors it): c_l = fl(B - e') <= B - e' + 2^-24 (|B| + e'), so by (2)
//         c'_l <= -2^23 A + c_l + p <= -2^23 A + B - e + 2^-24 (|B| + e'):
//       the pad is used up by the shift, and what is left is the unshifted form's addend with ITS rounding.
//   (4) The test's fma rounds S = (8388608 + q) A + c'_l once; product and sum are exact before that.  By (3) S <= q A + B - e + 2^-24 (|B| + e'),
//       rounding is monotonic and costs 2^-24 (65535 |A| + |B| + e) at most, and t >= q A + B - 2^-24 (65535 |A| + |B|) (roundings of A and B).
//       Hence fl(S) <= t as soon as e >= 2^-24 (2 x 65535 |A| + 3 |B| + e + e'), about 2^-23 (65535 |A| + 1.5 |B|): half of e = 3 E.
// The box grows by p per side, |A| / 2 + 2^-24 |B|: half a grid cell (of 65536 per axis) near the grid, as the old pad meant to; far away it is a
// sixth of e.  An axis never culls unless e' < 1e30, which also keeps 2^23 |A| < 2^24 e' finite (e < 1e30 alone allows |A| = 4.2e31, where
// c' would be an infinity of A's sign on BOTH sides and the axis would cull everything).
// Per child and axis: two permutes instead of a rotate and two SDWA conversions.
#ifndef FJ_SLAB_PERM
#define FJ_SLAB_PERM 1
#endif
FJ_S32_FN Slab32Axis slab32q_axis(double inv, double oo, double g0, double cell)
{
  const float A = (float) (cell * inv), B = (float) ((g0 - oo) * inv);
#if FJ_SLAB_PERM
  // e' = e + p with both terms' coefficients merged (two operations): |A|: 3.6e-7 x 65535.07 + 5.97e-8 x (2^23 + 3.6e-7 x 65535.07) = 0.5243925,
  // |B|: 3.6e-7 + 5.97e-8 x (1 + 3.6e-7) = 4.197000e-7; rounded up, with 1e-5 relative to spare for the two float operations
  const float e = fmaf(.52440f, fabsf(A), 4.1971e-7f * fabsf(B));
#else
  const float e = 3.6e-7f * (65535.f * 1.000001f * fabsf(A) + fabsf(B));
#endif
  const bool ok = e < 1e30f;
  Slab32Axis a;
  a.i = ok ? A : 0.f;
#if FJ_SLAB_PERM
  a.l = ok ? fmaf(-8388608.f, A, B - e) : -1e30f;
  a.h = ok ? fmaf(-8388608.f, A, B + e) : 1e30f;
#else
  a.l = ok ? B - e : -1e30f;
  a.h = ok ? B + e : 1e30f;
#endif
  return a;
}
FJ_S32_FN Slab32 slab32q_setup(V3 oo, V3 inv, const double *g0, const double *cell)
{
  Slab32 s;
  s.x = slab32q_axis(inv.x, oo.x, g0[0], cell[0]);
  s.y = slab32q_axis(inv.y, oo.y, g0[1], cell[1]);
  s.z = slab32q_axis(inv.z, oo.z, g0[2], cell[2]);
  return s;
}
// (min, max) pair of grid coordinates packed in one 32-bit word -> two floats
FJ_S32_FN fj_v2f unpack_q(uint32_t w) { fj_v2f p; p.x = (float) (w & 0xffffu); p.y = (float) (w >> 16); return p; }

// px py pz = the (min, max) pairs of a child box; tmin32 <= tmin and tmax32 >= tmax of the ray.
// *tnear = conservative entry distance (an ordering key for the closest-hit walk).
FJ_S32_FN bool slab32_test(fj_v2f px, fj_v2f py, fj_v2f pz, const Slab32 s, float tmin32, float tmax32, float *tnear)
{
  const fj_v2f lx = __builtin_elementwise_fma(px, (fj_v2f) (s.x.i), (fj_v2f) (s.x.l));
  const fj_v2f hx = __builtin_elementwise_fma(px, (fj_v2f) (s.x.i), (fj_v2f) (s.x.h));
  const fj_v2f ly = __builtin_elementwise_fma(py, (fj_v2f) (s.y.i), (fj_v2f) (s.y.l));
  const fj_v2f hy = __builtin_elementwise_fma(py, (fj_v2f) (s.y.i), (fj_v2f) (s.y.h));
  const fj_v2f lz = __builtin_elementwise_fma(pz, (fj_v2f) (s.z.i), (fj_v2f) (s.z.l));
  const fj_v2f hz = __builtin_elementwise_fma(pz, (fj_v2f) (s.z.i), (fj_v2f) (s.z.h));
  const float tn = fmaxf(fmaxf(fmaxf(fminf(lx.x, lx.y), fminf(ly.x, ly.y)), fminf(lz.x, lz.y)), tmin32);
  const float tf = fminf(fminf(fminf(fmaxf(hx.x, hx.y), fmaxf(hy.x, hy.y)), fmaxf(hz.x, hz.y)), tmax32);
  *tnear = tn;
  return tn <= tf;
}
// The same test on a QUANTISED box with the direction signs of the ray used up front: wx wy wz are the
// (min, max) words of one child; sh* (slab32_shift) say which half of a word is the NEAR plane on that
// axis -- the low one unless the ray runs towards smaller coordinates.  With the near plane in the first
// and the far plane in the second element, one packed fma per axis yields (entry, exit) directly --
// fma(b, i, l) is monotonic in b, hence min(fma(min, i, l), fma(max, i, l)) IS fma(near, i, l) and
// likewise for the exit side: the same numbers as slab32_test, 4 instead of 6 instructions per axis.
//   FJ_SLAB_PERM 1: sh = the v_perm_b32 selector that builds as_float(0x4B000000 | near half) -- result bytes 3, 2 =
//                   bytes 3, 2 of the constant (selector values 7, 6), bytes 1, 0 = the word's (1, 0) or (3, 2); the
//                   far half's selector is sh ^ 0x0202
//   FJ_SLAB_PERM 0: sh = 16 or 0, the word is rotated (v_alignbit_b32) and converted (2 SDWA cvt)
#if FJ_SLAB_PERM
FJ_S32_FN uint32_t slab32_shift(float i) { return 0x07060100u ^ ((FJ_S32_BITS(i) >> 31) * 0x0202u); }
FJ_S32_FN fj_v2f slab32q_planes(uint32_t w, uint32_t sh)
{
  fj_v2f p;
  p.x = FJ_S32_FLOAT(FJ_S32_PERM(0x4B000000u, w, sh));
  p.y = FJ_S32_FLOAT(FJ_S32_PERM(0x4B000000u, w, sh ^ 0x0202u));
  return p;
}
#else
FJ_S32_FN uint32_t slab32_shift(float i) { return (FJ_S32_BITS(i) >> 31) << 4; }
FJ_S32_FN fj_v2f slab32q_planes(uint32_t w, uint32_t sh) { return unpack_q(FJ_S32_ALIGNBIT(w, w, sh)); }
#endif
FJ_S32_FN bool slab32q_test(uint32_t wx, uint32_t wy, uint32_t wz, const Slab32 s, uint32_t shx, uint32_t shy, uint32_t shz,
    float tmin32, float tmax32, float *tnear = nullptr)
{
  const fj_v2f px = slab32q_planes(wx, shx);
  const fj_v2f py = slab32q_planes(wy, shy);
  const fj_v2f pz = slab32q_planes(wz, shz);
  fj_v2f cx, cy, cz;
  cx.x = s.x.l; cx.y = s.x.h; cy.x = s.y.l; cy.y = s.y.h; cz.x = s.z.l; cz.y = s.z.h;
  const fj_v2f tx = __builtin_elementwise_fma(px, (fj_v2f) (s.x.i), cx);
  const fj_v2f ty = __builtin_elementwise_fma(py, (fj_v2f) (s.y.i), cy);
  const fj_v2f tz = __builtin_elementwise_fma(pz, (fj_v2f) (s.z.i), cz);
  const float tn = fmaxf(fmaxf(fmaxf(tx.x, ty.x), tz.x), tmin32);
  const float tf = fminf(fminf(fminf(tx.y, ty.y), tz.y), tmax32);
  if (tnear) *tnear = tn;
  return tn <= tf;
}
// the same with the slab constants held the way the packed fma wants them: (l, h) of an axis as ONE two-float value (a register pair: built
// per test from two scalars it cost the any-hit walk ten moves per iteration), the slope as a scalar (broadcast by the instruction's op_sel)
struct Slab32P { float ix, iy, iz; fj_v2f lhx, lhy, lhz; };
FJ_S32_FN Slab32P slab32p(const Slab32 s)
{
  Slab32P p;
  p.ix = s.x.i; p.iy = s.y.i; p.iz = s.z.i;
  p.lhx.x = s.x.l; p.lhx.y = s.x.h; p.lhy.x = s.y.l; p.lhy.y = s.y.h; p.lhz.x = s.z.l; p.lhz.y = s.z.h;
  return p;
}
FJ_S32_FN bool slab32q_test(uint32_t wx, uint32_t wy, uint32_t wz, const Slab32P s, uint32_t shx, uint32_t shy, uint32_t shz,
    float tmin32, float tmax32)
{
  const fj_v2f tx = __builtin_elementwise_fma(slab32q_planes(wx, shx), (fj_v2f) (s.ix), s.lhx);
  const fj_v2f ty = __builtin_elementwise_fma(slab32q_planes(wy, shy), (fj_v2f) (s.iy), s.lhy);
  const fj_v2f tz = __builtin_elementwise_fma(slab32q_planes(wz, shz), (fj_v2f) (s.iz), s.lhz);
  const float tn = fmaxf(fmaxf(fmaxf(tx.x, ty.x), tz.x), tmin32);
  const float tf = fminf(fminf(fminf(tx.y, ty.y), tz.y), tmax32);
  return tn <= tf;
}
// f32 bounds of an f64 ray range: down / up to the neighbouring float
FJ_S32_FN float f32_below(double x) { const float f = (float) x; return (double) f <= x ? f : nextafterf(f, -INFINITY); }
FJ_S32_FN float f32_above(double x) { const float f = (float) x; return (double) f >= x ? f : nextafterf(f, INFINITY); }

// ---- the quantiser's arithmetic for one axis of one child box (k_quantize_nodes): [lo, hi] (f32 planes, widened) outward onto the
// grid origin + q cell, q in [0, 65535].  floor / ceil in f64, then checked against the decoded plane and stepped outward if a rounding
// went the wrong way.  Planes outside the grid clamp; the empty slots' +-FLT_MAX / NaN come out as the inverted box (65535, 0).
FJ_S32_FN void slab32_quantize_axis(double lo, double hi, double origin, double cell, uint16_t *ql_out, uint16_t *qh_out)
{
  double ql = floor((lo - origin) / cell), qh = ceil((hi - origin) / cell);
  // (the negated comparisons come first: they also catch the NaN of an empty slot, which must end as ql = 65535, qh = 0 like +-FLT_MAX --
  //  clamped the other way round first, a NaN slot decoded to the WHOLE grid, a box every ray through the grid passes)
  if (!(ql <= 65535)) ql = 65535;
  if (!(qh >= 0)) qh = 0;
  if (ql < 0) ql = 0;
  if (qh > 65535) qh = 65535;
  if (origin + ql * cell > lo && ql > 0) ql -= 1;
  if (origin + qh * cell < hi && qh < 65535) qh += 1;
  *ql_out = (uint16_t) ql;
  *qh_out = (uint16_t) qh;
}

// ---- one (ray, box) pair through every member of the family, for the batch entries that tests compare bit for bit: fjgpu_dev_slab32_batch
// (the device, which computes inv with its own filter_rcp) and fj_slab32_probe_batch (the host tool, fed the device's inv).
//   ray   o xyz, inv xyz, tmin, tmax;   grid  g0 xyz, cell xyz;   words  the (min, max) words of x, y, z
// The f32 path runs on the box decoded from the words, each plane rounded to f32, with the grid's own extent as the primitive set's bounds.
// verdict: bit 0 slab32q_test (Slab32), bit 1 slab32q_test (Slab32P), bit 2 slab32_test.
struct Slab32Probe {
  double inv[3];
  float q[9], f[9];            // (i, l, h) of x, y, z: slab32q_setup, slab32_setup
  float tnear_q, tnear_f;
  uint32_t verdict;
  uint32_t sh[3];              // slab32_shift of the quantised form's slopes
  uint32_t pad[2];
};
static_assert(sizeof(Slab32Probe) == 128, "Slab32Probe must be 128 bytes");

FJ_S32_FN void slab32_probe(const double *ray, const double *grid, const uint32_t *words, Slab32Probe *out)
{
  V3 o, inv;
  o.x = ray[0]; o.y = ray[1]; o.z = ray[2]; inv.x = ray[3]; inv.y = ray[4]; inv.z = ray[5];
  const float tmin32 = f32_below(ray[6]), tmax32 = f32_above(ray[7]);
  Slab32Probe r;
  r.inv[0] = inv.x; r.inv[1] = inv.y; r.inv[2] = inv.z;
  const Slab32 sq = slab32q_setup(o, inv, grid, grid + 3);
  const uint32_t shx = slab32_shift(sq.x.i), shy = slab32_shift(sq.y.i), shz = slab32_shift(sq.z.i);
  const bool v0 = slab32q_test(words[0], words[1], words[2], sq, shx, shy, shz, tmin32, tmax32, &r.tnear_q);
  const bool v1 = slab32q_test(words[0], words[1], words[2], slab32p(sq), shx, shy, shz, tmin32, tmax32);
  double bounds[6];
  fj_v2f p[3];
  for (int a = 0; a < 3; a++) {
    bounds[a] = grid[a]; bounds[3 + a] = grid[a] + 65535.0 * grid[3 + a];
    p[a].x = (float) (grid[a] + (double) (words[a] & 0xffffu) * grid[3 + a]);
    p[a].y = (float) (grid[a] + (double) (words[a] >> 16) * grid[3 + a]);
  }
  const Slab32 sf = slab32_setup(o, inv, bounds);
  const bool v2 = slab32_test(p[0], p[1], p[2], sf, tmin32, tmax32, &r.tnear_f);
  r.q[0] = sq.x.i; r.q[1] = sq.x.l; r.q[2] = sq.x.h; r.q[3] = sq.y.i; r.q[4] = sq.y.l; r.q[5] = sq.y.h; r.q[6] = sq.z.i; r.q[7] = sq.z.l; r.q[8] = sq.z.h;
  r.f[0] = sf.x.i; r.f[1] = sf.x.l; r.f[2] = sf.x.h; r.f[3] = sf.y.i; r.f[4] = sf.y.l; r.f[5] = sf.y.h; r.f[6] = sf.z.i; r.f[7] = sf.z.l; r.f[8] = sf.z.h;
  r.verdict = (v0 ? 1u : 0u) | (v1 ? 2u : 0u) | (v2 ? 4u : 0u);
  r.sh[0] = shx; r.sh[1] = shy; r.sh[2] = shz;
  r.pad[0] = r.pad[1] = 0;
  *out = r;
}

#endif
