// fjgpu_temporal_math.h -- the arithmetic of fjgpu_denoise_temporal (include/fjgpu.h): the temporal accumulation of SVGF (Schied et al.,
// HPG 2017, 4.1): the world position of a pixel is projected into the previous frame, the history found there -- colour, the two luminance
// moments, the history length -- is fetched bilinearly over the taps that still show the same surface, and the new frame is blended in.
//
// ONE source for the device kernel (fjgpu_temporal.hip: k_tp_accumulate), for the host twin the CPU tests run (tools/temporal_host.cc) and
// for tests/temporal_model.py, which restates it in numpy.  f32 under -ffp-contract=off, every sum left to right; the projection alone is
// f64.  A pixel is one call of fj_tp_pixel -- fj_tp_fetch, then fj_tp_finish --: kernel and twin differ in who calls it, not in a
// statement of it.  fjgpu_denoise_temporal_clamped puts fj_tp_clamp between the two (fj_tp_pixel_clamped; k_tp_accumulate_clamped and
// the twin's fj_denoise_temporal_clamped_host; tests/temporal_clamp_model.py restates it).
//
//   projection of the world point P through the view (world_to_camera M, rows of a 3 x 4 matrix; uv_size; xres, yres), f64:
//     c_k = ((M[4k] P.x + M[4k+1] P.y) + M[4k+2] P.z) + M[4k+3];      visible only if c.z < 0
//     fx = (c.x / -c.z / uv_size[0] + .5) xres - .5;    fy = (.5 - c.y / -c.z / uv_size[1]) yres - .5       (both must be finite)
//   luminance   L = l(D), l of fjgpu_denoise_var_math.h; D = C.rgb / max(albedo, albedo_floor) per channel with an albedo, else C.rgb
//   fetch       x0 = floor(fx), y0 = floor(fy), a = (float) (fx - x0), b = (float) (fy - y0); taps q = (x0 + i, y0 + j), j outer, i inner,
//               w = (i ? a : 1.f - a) * (j ? b : 1.f - b).  A tap counts if it lies in the region, prev_ids[q][0] == ids[p][0],
//               |prev_position[q] - P|^2 <= tol_position^2 (term on), dot(prev_normal[q], N) >= cos_normal (term on), prev length[q] >= 1.
//               wsum += w, H += w X_q for the seven history values; then H /= wsum.  No history where wsum <= 1e-4f.
//   blend       n = min(H_len + 1, max_history), alpha = max(1.f / n, alpha_min), X' = H + alpha (X - H) for X in {C (4), L, L L}; len' = n
//   no history  C' = C, m1 = L, m2 = L L, len' = 1
//   variance    v = max(0, m2' - m1' m1'); where len' < min_history_variance and there is a spatial variance: that
//   clamp       (the clamped entry, pixels with a history, after H /= wsum) taps q = p + (dx, dy), dy = -r..r outer, dx = -r..r inner, of
//               the CURRENT frame; a tap counts if it lies in the region and (stop_at_ids) ids[q][0] == ids[p][0].  For X in {C_q (4), L_q}:
//               cnt += 1.f, s1 += X_q, m = s1 / cnt; then over the same taps d = X_q - m, s2 += d d, sd = sqrtf(s2 / cnt);
//               lo = m - gamma sd, hi = m + gamma sd;  H' = H < lo ? lo : (H > hi ? hi : H) for the colour and, against L's box, for h1;
//               h2' = h2 where h1' == h1, else (h2 - h1 h1) + h1' h1';  amount = max |H' - H| over r, g, b;  blend and variance from H'
#ifndef FJGPU_TEMPORAL_MATH_H
#define FJGPU_TEMPORAL_MATH_H

#include "fjgpu_denoise_var_math.h"

#define FJ_TP_MIN_WEIGHT 1e-4f

typedef float tp_v4f __attribute__((ext_vector_type(4)));

// everything of a call that is not a buffer
struct TpParams {
  double w2c[12];                  // the previous frame's view
  double uv_size[2];
  int32_t view_xres, view_yres;
  int32_t xres, yres;              // the frame the buffers describe
  int32_t x0, y0, x1, y1;          // region
  float alpha_min, max_history;
  float tol2;                      // tol_position^2 (position_on)
  float cos_normal;                // (normal_on)
  float min_history_variance, albedo_floor;
  int32_t position_on, normal_on;
};

// the frames of a call: pointers to pixel (0, 0) of [yres][xres][channels] arrays -- device memory in the kernel, host memory in the twin
struct TpBuffers {
  const float *color, *position, *normal;
  const int32_t *ids;
  const float *albedo, *variance_spatial;                  // or null
  const float *prev_position, *prev_normal;
  const int32_t *prev_ids;
  const float *prev_color, *prev_moments, *prev_length;    // all null: first frame
  float *next_color, *next_moments, *next_length;
  float *variance_out;                                     // or null
};

FJ_DN_FN void fj_tp_terms(float tol_position, float cos_normal, TpParams *k)
{
  k->position_on = (tol_position > 0.f && tol_position != INFINITY) ? 1 : 0;
  k->tol2 = k->position_on ? tol_position * tol_position : 0.f;
  k->normal_on = cos_normal > -1.f ? 1 : 0;
  k->cos_normal = cos_normal;
}

// (fx, fy) of the world point through the previous view; false: behind the camera or not finite
FJ_DN_FN bool fj_tp_project(const TpParams &k, float px, float py, float pz, double *fx, double *fy)
{
  const double X = (double) px, Y = (double) py, Z = (double) pz;
  const double *M = k.w2c;
  const double cx = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[3];
  const double cy = ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7];
  const double cz = ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11];
  if (!(cz < 0.)) return false;
  const double d = -cz;
  *fx = (cx / d / k.uv_size[0] + .5) * (double) k.view_xres - .5;
  *fy = (.5 - cy / d / k.uv_size[1]) * (double) k.view_yres - .5;
  return isfinite(*fx) && isfinite(*fy);
}

FJ_DN_FN float fj_tp_blend(float h, float x, float alpha) { return h + alpha * (x - h); }

// what the fetch leaves of a pixel: the current colour and luminance and -- where have -- the history at its projection, already divided
// by the valid weight
struct TpFetched {
  tp_v4f C;
  float L;
  bool have;                       // wsum > FJ_TP_MIN_WEIGHT
  float hr, hg, hb, ha, h1, h2, hl;
};

// L of the pixel at index `at` whose colour is C: the luminance of every statement above, and of the clamp's window
FJ_DN_FN float fj_tp_luminance(const TpParams &k, const TpBuffers &B, size_t at, const tp_v4f &C)
{
  float dr = C.x, dg = C.y, db = C.z;
  if (B.albedo) {
    dr = fj_dn_demodulate(C.x, fj_dn_albedo_clamp(B.albedo[3 * at], k.albedo_floor));
    dg = fj_dn_demodulate(C.y, fj_dn_albedo_clamp(B.albedo[3 * at + 1], k.albedo_floor));
    db = fj_dn_demodulate(C.z, fj_dn_albedo_clamp(B.albedo[3 * at + 2], k.albedo_floor));
  }
  return fj_dnv_luminance(dr, dg, db);
}

// the region pixel (x, y) up to and including H /= wsum
FJ_DN_FN TpFetched fj_tp_fetch(const TpParams &k, const TpBuffers &B, int x, int y)
{
  const size_t at = (size_t) y * (size_t) k.xres + (size_t) x;
  const tp_v4f C = *(const tp_v4f *) (B.color + 4 * at);
  const float L = fj_tp_luminance(k, B, at, C);
  const int32_t I = B.ids[4 * at];
  float wsum = 0.f, hr = 0.f, hg = 0.f, hb = 0.f, ha = 0.f, h1 = 0.f, h2 = 0.f, hl = 0.f;
  if (B.prev_color && I >= 0) {
    const float px = B.position[3 * at], py = B.position[3 * at + 1], pz = B.position[3 * at + 2];
    double fx, fy;
    if (isfinite(px) && isfinite(py) && isfinite(pz) && fj_tp_project(k, px, py, pz, &fx, &fy)) {
      const double xf = floor(fx), yf = floor(fy);
      // (a footprint that touches the region; also what keeps the conversions to int in range)
      if (xf >= (double) (k.x0 - 1) && xf < (double) k.x1 && yf >= (double) (k.y0 - 1) && yf < (double) k.y1) {
        const int qx0 = (int) xf, qy0 = (int) yf;
        const float a = (float) (fx - xf), b = (float) (fy - yf);
        const float nx = B.normal[3 * at], ny = B.normal[3 * at + 1], nz = B.normal[3 * at + 2];
        // Everything the four taps may need is loaded before anything of it is looked at -- a tap outside the region from the nearest
        // pixel inside it, where it does not count --, so that a pixel waits for one round of loads, not for one per test and tap; a tap
        // that does not count adds nothing: each sum is selected, which is what skipping the tap gives.
#pragma unroll
        for (int t = 0; t < 4; t++) {
          const int i = t & 1, j = t >> 1;                     // j outer, i inner
          const int qx = qx0 + i, qy = qy0 + j;
          const bool in_region = qx >= k.x0 && qx < k.x1 && qy >= k.y0 && qy < k.y1;
          const int cx = qx < k.x0 ? k.x0 : (qx >= k.x1 ? k.x1 - 1 : qx), cy = qy < k.y0 ? k.y0 : (qy >= k.y1 ? k.y1 - 1 : qy);
          const size_t q = (size_t) cy * (size_t) k.xres + (size_t) cx;
          const int32_t qi = B.prev_ids[4 * q];
          const float qpx = B.prev_position[3 * q], qpy = B.prev_position[3 * q + 1], qpz = B.prev_position[3 * q + 2];
          const float qnx = B.prev_normal[3 * q], qny = B.prev_normal[3 * q + 1], qnz = B.prev_normal[3 * q + 2];
          const float len = B.prev_length[q];
          const tp_v4f H = *(const tp_v4f *) (B.prev_color + 4 * q);
          const float q1 = B.prev_moments[2 * q], q2 = B.prev_moments[2 * q + 1];
          const float d2 = fj_dn_dist2(px, py, pz, qpx, qpy, qpz);
          const float dn = qnx * nx + qny * ny + qnz * nz;
          const bool valid = in_region & (qi == I) & (!k.position_on | (d2 <= k.tol2)) & (!k.normal_on | (dn >= k.cos_normal)) & (len >= 1.f);
          const float w = (i ? a : 1.f - a) * (j ? b : 1.f - b);
          wsum = valid ? wsum + w : wsum;
          hr = valid ? hr + w * H.x : hr; hg = valid ? hg + w * H.y : hg; hb = valid ? hb + w * H.z : hb; ha = valid ? ha + w * H.w : ha;
          h1 = valid ? h1 + w * q1 : h1; h2 = valid ? h2 + w * q2 : h2;
          hl = valid ? hl + w * len : hl;
        }
      }
    }
  }
  TpFetched F;
  F.C = C; F.L = L;
  F.have = wsum > FJ_TP_MIN_WEIGHT;
  F.hr = hr; F.hg = hg; F.hb = hb; F.ha = ha; F.h1 = h1; F.h2 = h2; F.hl = hl;
  if (F.have) {
    F.hr = hr / wsum; F.hg = hg / wsum; F.hb = hb / wsum; F.ha = ha / wsum; F.h1 = h1 / wsum; F.h2 = h2 / wsum; F.hl = hl / wsum;
  }
  return F;
}

// blend, variance and the stores of the region pixel (x, y) from what was fetched (and, in the clamped pass, rectified)
FJ_DN_FN void fj_tp_finish(const TpParams &k, const TpBuffers &B, int x, int y, const TpFetched &F)
{
  const size_t at = (size_t) y * (size_t) k.xres + (size_t) x;
  const tp_v4f C = F.C;
  const float L = F.L;
  const float L2 = L * L;
  tp_v4f O = C;
  float m1 = L, m2 = L2, n = 1.f;
  if (F.have) {
    const float n1 = F.hl + 1.f;
    n = n1 < k.max_history ? n1 : k.max_history;
    const float r = 1.f / n;
    const float alpha = r > k.alpha_min ? r : k.alpha_min;
    O.x = fj_tp_blend(F.hr, C.x, alpha); O.y = fj_tp_blend(F.hg, C.y, alpha); O.z = fj_tp_blend(F.hb, C.z, alpha); O.w = fj_tp_blend(F.ha, C.w, alpha);
    m1 = fj_tp_blend(F.h1, L, alpha);
    m2 = fj_tp_blend(F.h2, L2, alpha);
  }
  *(tp_v4f *) (B.next_color + 4 * at) = O;
  B.next_moments[2 * at] = m1;
  B.next_moments[2 * at + 1] = m2;
  B.next_length[at] = n;
  if (B.variance_out) {
    float v = m2 - m1 * m1;
    v = v > 0.f ? v : 0.f;
    if (B.variance_spatial && n < k.min_history_variance) v = B.variance_spatial[at];
    B.variance_out[at] = v;
  }
}

// ---- the history rectification of fjgpu_denoise_temporal_clamped (variance clipping, Salvi 2016), between fetch and finish.
// Its window is read as RECORDS of FJ_TP_REC words -- C.r C.g C.b C.a, L, the bits of ids[q][0] --, one per pixel, through a pointer to
// the centre's record and the strides of a row and of a pixel in words: the kernel points it into its LDS tile, the twin into the records
// of the caller's frame.  fj_tp_record writes one; a record outside the region is never written and never read.
#define FJ_TP_REC 6
#define FJ_TP_CLAMP_MAX_RADIUS 3

// what fjgpu_temporal_clamp says, for the kernel
struct TpClamp {
  int32_t radius, stop_at_ids;
  float gamma;
  float *amount;                   // pixel (0, 0) of [yres][xres], or null
};

FJ_DN_FN void fj_tp_record(const TpParams &k, const TpBuffers &B, int x, int y, float *rec)
{
  const size_t at = (size_t) y * (size_t) k.xres + (size_t) x;
  const tp_v4f C = *(const tp_v4f *) (B.color + 4 * at);
  const int32_t I = B.ids[4 * at];
  rec[0] = C.x; rec[1] = C.y; rec[2] = C.z; rec[3] = C.w;
  rec[4] = fj_tp_luminance(k, B, at, C);
  __builtin_memcpy(rec + 5, &I, 4);
}

FJ_DN_FN float fj_tp_clip(float h, float lo, float hi) { return h < lo ? lo : (h > hi ? hi : h); }

// whether the tap at (qx, qy), whose record is `q`, counts in the window of a pixel with id I; the record of a tap outside the region is not read
FJ_DN_FN bool fj_tp_tap_counts(const TpParams &k, int stop_at_ids, int32_t I, const float *q, int qx, int qy)
{
  if (qx < k.x0 || qx >= k.x1 || qy < k.y0 || qy >= k.y1) return false;
  int32_t qi;
  __builtin_memcpy(&qi, q + 5, 4);
  return !stop_at_ids || qi == I;
}

// the pixel (x, y), which has a history: F's colour and moments clipped to the box of the window around `centre`; returns the amount
template <int radius>
FJ_DN_FN float fj_tp_clamp(const TpParams &k, float gamma, int stop_at_ids, const float *centre, int row, int px, int x, int y,
    TpFetched &F)
{
  int32_t I;
  __builtin_memcpy(&I, centre + 5, 4);
  float cnt = 0.f, s1[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, s2[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, m[5];
#pragma unroll
  for (int dy = -radius; dy <= radius; dy++) {
#pragma unroll
    for (int dx = -radius; dx <= radius; dx++) {
      const float *q = centre + dy * row + dx * px;
      if (fj_tp_tap_counts(k, stop_at_ids, I, q, x + dx, y + dy)) {
        cnt += 1.f;
#pragma unroll
        for (int c = 0; c < 5; c++) s1[c] += q[c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 5; c++) m[c] = s1[c] / cnt;
#pragma unroll
  for (int dy = -radius; dy <= radius; dy++) {
#pragma unroll
    for (int dx = -radius; dx <= radius; dx++) {
      const float *q = centre + dy * row + dx * px;
      if (fj_tp_tap_counts(k, stop_at_ids, I, q, x + dx, y + dy)) {
#pragma unroll
        for (int c = 0; c < 5; c++) {
          const float d = q[c] - m[c];
          s2[c] += d * d;
        }
      }
    }
  }
  float lo[5], hi[5];
#pragma unroll
  for (int c = 0; c < 5; c++) {
    const float sd = sqrtf(s2[c] / cnt);
    lo[c] = m[c] - gamma * sd;
    hi[c] = m[c] + gamma * sd;
  }
  const float hr = fj_tp_clip(F.hr, lo[0], hi[0]), hg = fj_tp_clip(F.hg, lo[1], hi[1]), hb = fj_tp_clip(F.hb, lo[2], hi[2]);
  const float ha = fj_tp_clip(F.ha, lo[3], hi[3]);
  const float h1 = fj_tp_clip(F.h1, lo[4], hi[4]);
  const float ar = fabsf(hr - F.hr), ag = fabsf(hg - F.hg), ab = fabsf(hb - F.hb);
  float amount = ar;
  amount = ag > amount ? ag : amount;
  amount = ab > amount ? ab : amount;
  if (h1 != F.h1) F.h2 = (F.h2 - F.h1 * F.h1) + h1 * h1;
  F.hr = hr; F.hg = hg; F.hb = hb; F.ha = ha; F.h1 = h1;
  return amount;
}

// the region pixel (x, y) of fjgpu_denoise_temporal_clamped with c.radius == radius; `centre`, `row`, `px`: its record in the window's records
template <int radius>
FJ_DN_FN void fj_tp_pixel_clamped(const TpParams &k, const TpBuffers &B, const TpClamp &c, const float *centre, int row, int px, int x, int y)
{
  TpFetched F = fj_tp_fetch(k, B, x, y);
  float amount = 0.f;
  if (F.have) amount = fj_tp_clamp<radius>(k, c.gamma, c.stop_at_ids, centre, row, px, x, y, F);
  if (c.amount) c.amount[(size_t) y * (size_t) k.xres + (size_t) x] = amount;
  fj_tp_finish(k, B, x, y, F);
}

// the region pixel (x, y) of fjgpu_denoise_temporal
FJ_DN_FN void fj_tp_pixel(const TpParams &k, const TpBuffers &B, int x, int y)
{
  fj_tp_finish(k, B, x, y, fj_tp_fetch(k, B, x, y));
}

#endif
