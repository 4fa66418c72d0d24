// fjgpu_matte_math.h -- the definition of fjgpu_render_aov_matte (include/fjgpu.h): per pixel, the `ranks` keys (instance or shader) with the
// greatest share of the pixel and those shares.  One source for the kernel k_aov_matte (fjgpu_matte.hip) and for the host twin of the CPU
// tests (csrc/tools/matte_host.cc); tests/matte_model.py restates this text in numpy f64.  Compiled with -ffp-contract=off.
//
// A pixel p, its samples s, each with a key k_s and a weight w_s:
//   filtered = 1   the npx_x * npx_y samples of the window k_resolve (fjgpu_kernels.hip) reads for p -- its `base`, its row-major order --,
//                  w_s = fj_sv_weight (fjgpu_sample_var_math.h): k_resolve's Gaussian weight in f64.  The shares are then the shares the
//                  beauty pixel's blend gives the keys.
//   filtered = 0   the pixel's own rate_x * rate_y samples (k_aov_reduce's k0), w_s = 1: every sum is a count, exact in f64.
//   k_s   -1 for a sample that hit nothing.  Key "instance": the hit's instance.  Key "shader": the shader slot as k_aov_reduce computes
//         ids[3] -- the face group of the hit primitive for a mesh, group 0 for a curve, then fj_mt_shader_key, the slot rules of
//         ObjectInstance::GetShader (src/fj_object_instance.cc:177-191).  A hit whose shader is UNASSIGNED (slot 0 empty) has key -1 too:
//         like a miss it is never ranked and counts neither in `rest` nor in `distinct`; its weight is in W only.
//   W = sum of w_s over ALL samples, misses included.
// Keys are visited in ascending order, which fixes the order of every sum and resolves ties:
//   1  last = -1, R = 0, the list empty
//   2  key = min { k_s : k_s > last }; stop when there is none
//   3  A = sum of w_s with k_s == key
//   4  insert (key, A) into the list of `ranks` entries before the first entry whose weight is strictly smaller (an empty entry is smaller
//      than any weight): equal weights stay in ascending key order
//   5  the entry that leaves the list -- the last one, or (key, A) itself where the list is full and nothing in it is smaller -- adds its
//      weight to R; last = key, go to 2
// Outputs: ids[r], coverage[r] = (float) (A_r / W) rank by rank, -1 and 0 for an empty rank; rest = (float) (R / W): the share of the hit
// keys that did not fit into `ranks`; distinct = the number of keys visited.  With filtered = 0 the quotients are written
// (float) count / (float) nown, the statement k_aov_reduce uses for its coverage (coverage and rest alike).
// The sums are f64; the order inside step 3 and inside W is the caller's (the kernel: per lane in sample order, then a butterfly; the twin:
// row-major).
#ifndef FJGPU_MATTE_MATH_H
#define FJGPU_MATTE_MATH_H

#include <stddef.h>
#include <stdint.h>

#include "fjgpu_sample_var_math.h"

#define FJ_MT_MAX_RANKS 16          // FJGPU_MATTE_MAX_RANKS (include/fjgpu.h; held equal by fjgpu_matte.hip and matte_host.cc)
#define FJ_MT_KEY_INSTANCE 0        // FJGPU_MATTE_KEY_INSTANCE
#define FJ_MT_KEY_SHADER 1          // FJGPU_MATTE_KEY_SHADER

// the ranked list.  Every loop over it has constant bounds and is unrolled, so that the kernel keeps it in registers.
struct MtList {
  int32_t key[FJ_MT_MAX_RANKS];
  double w[FJ_MT_MAX_RANKS];        // -1: an empty entry (a weight is >= 0)
};

FJ_DN_FN void fj_mt_clear(MtList &L)
{
#pragma unroll
  for (int r = 0; r < FJ_MT_MAX_RANKS; r++) { L.key[r] = -1; L.w[r] = -1.; }
}

// ObjectInstance::GetShader's slot rules on an instance's shader list: a group out of range or an unassigned slot gives slot 0; -1 where
// that is unassigned too
template <typename ShaderList>
FJ_DN_FN int32_t fj_mt_shader_key(int sg, int n_shaders, ShaderList shaders)
{
  int sid;
  if (sg < 0 || sg >= n_shaders) sid = shaders[0];
  else { sid = shaders[sg]; if (sid < 0) sid = shaders[0]; }
  return sid < 0 ? -1 : sid;
}

// steps 4 and 5: (key, A) travels down the list; from the first entry it displaces on it carries the displaced entry
FJ_DN_FN void fj_mt_insert(MtList &L, int ranks, int32_t key, double A, double &R)
{
  bool moving = false;
#pragma unroll
  for (int r = 0; r < FJ_MT_MAX_RANKS; r++) {
    const int32_t k2 = L.key[r];
    const double w2 = L.w[r];
    if (r < ranks && (moving || w2 < A)) { L.key[r] = key; L.w[r] = A; key = k2; A = w2; moving = true; }
  }
  if (key >= 0) R += A;
}

FJ_DN_FN float fj_mt_share(int filtered, double A, double W, int nown)
{
  return filtered ? (float) (A / W) : (float) A / (float) nown;
}

// the pixel's outputs; ids / coverage: the pixel's `ranks` entries, rest / distinct: the pixel's entry or null
FJ_DN_FN void fj_mt_write(const MtList &L, int ranks, int filtered, double W, int nown, double R, int ndistinct, int32_t *ids, float *coverage,
    float *rest, int32_t *distinct)
{
#pragma unroll
  for (int r = 0; r < FJ_MT_MAX_RANKS; r++)
    if (r < ranks) {
      ids[r] = L.key[r];
      coverage[r] = L.key[r] < 0 ? 0.f : fj_mt_share(filtered, L.w[r], W, nown);
    }
  if (rest) *rest = fj_mt_share(filtered, R, W, nown);
  if (distinct) *distinct = ndistinct;
}

// the whole pixel over arrays, samples in row-major order: `first` is the first sample of the pixel's window (filtered: k_resolve's `base`;
// else the tile's first slot + k_aov_reduce's k0), `row` the samples per row of the tile (TileDesc.nx); s_uv [.][2] f64 (not read with
// filtered = 0), keys [.] the key of every sample
FJ_DN_FN void fj_mt_pixel(const SvFrame &f, int filtered, int ranks, int px, int py, size_t first, int row, const double *s_uv,
    const int32_t *keys, int32_t *ids, float *coverage, float *rest, int32_t *distinct)
{
  const int nwx = filtered ? f.npx_x : f.rate_x, nwy = filtered ? f.npx_y : f.rate_y;
  auto weight = [&](size_t s) { return filtered ? fj_sv_weight(f, px, py, s_uv[2 * s], s_uv[2 * s + 1]) : 1.; };
  double W = 0, R = 0;
  for (int sy = 0; sy < nwy; sy++)
    for (int sx = 0; sx < nwx; sx++) W += weight(first + (size_t) sy * row + sx);
  MtList L;
  fj_mt_clear(L);
  int32_t last = -1;
  int n = 0;
  for (;;) {
    int32_t key = INT32_MAX;
    bool any = false;
    for (int sy = 0; sy < nwy; sy++)
      for (int sx = 0; sx < nwx; sx++) {
        const int32_t k = keys[first + (size_t) sy * row + sx];
        if (k > last && (!any || k < key)) { key = k; any = true; }
      }
    if (!any) break;
    double A = 0;
    for (int sy = 0; sy < nwy; sy++)
      for (int sx = 0; sx < nwx; sx++) {
        const size_t s = first + (size_t) sy * row + sx;
        if (keys[s] == key) A += weight(s);
      }
    fj_mt_insert(L, ranks, key, A, R);
    n++;
    last = key;
  }
  fj_mt_write(L, ranks, filtered, W, nwx * nwy, R, n, ids, coverage, rest, distinct);
}

#endif
