// slab32_host.cc -- validation tool: the slab tests of the BLAS walks and the node quantiser (device/fjgpu_slab32.h, the SAME source the
// kernels compile) built for the host, so that tests/test_slab32_cpu.py can hold every constant, plane value and verdict against exact
// arithmetic without a GPU, and tests/test_gpu_slab32.py the device's results against these bit for bit.  Built with the ROCm clang++
// (ext_vector_type, __builtin_elementwise_fma -> fmaf: one rounding, like v_pk_fma_f32), once per FJ_SLAB_PERM setting
// (lib/libfj_slab32_host.so: 1, the default; lib/libfj_slab32_host_perm0.so: 0).  Not part of the product path.
#include <stdint.h>
#include "fjgpu_types.h"
#include "fjgpu_slab32.h"

static inline void put_axis(const Slab32Axis a, float tlo, float thi, float *out) { out[0] = a.i; out[1] = a.l; out[2] = a.h; out[3] = tlo; out[4] = thi; }
static inline void put_consts(const Slab32 s, float *c)
{
  c[0] = s.x.i; c[1] = s.x.l; c[2] = s.x.h; c[3] = s.y.i; c[4] = s.y.l; c[5] = s.y.h; c[6] = s.z.i; c[7] = s.z.l; c[8] = s.z.h;
}
static inline void get_ray(const double *r, V3 *o, V3 *inv) { o->x = r[0]; o->y = r[1]; o->z = r[2]; inv->x = r[3]; inv->y = r[4]; inv->z = r[5]; }

extern "C" {

int fj_slab32_perm(void) { return FJ_SLAB_PERM; }

// (a) per-axis constants and plane values.  out [n][5]: i, l, h, t_lo, t_hi
// f32 boxes: plane b, the statement of slab32_test
void fj_slab32_axis_batch(int64_t n, const double *inv, const double *oo, const double *bmax_abs, const float *b, float *out)
{
  for (int64_t k = 0; k < n; k++) {
    const Slab32Axis a = slab32_axis(inv[k], oo[k], bmax_abs[k]);
    fj_v2f p; p.x = b[k]; p.y = b[k];
    const fj_v2f lo = __builtin_elementwise_fma(p, (fj_v2f) (a.i), (fj_v2f) (a.l));
    const fj_v2f hi = __builtin_elementwise_fma(p, (fj_v2f) (a.i), (fj_v2f) (a.h));
    put_axis(a, lo.x, hi.y, out + 5 * k);
  }
}
// quantised boxes: plane g0 + q cell, the statements of slab32q_test (q as both halves of the word, through slab32_shift / slab32q_planes)
void fj_slab32q_axis_batch(int64_t n, const double *inv, const double *oo, const double *g0, const double *cell, const uint16_t *q, float *out)
{
  for (int64_t k = 0; k < n; k++) {
    const Slab32Axis a = slab32q_axis(inv[k], oo[k], g0[k], cell[k]);
    const uint32_t w = (uint32_t) q[k] | ((uint32_t) q[k] << 16);
    fj_v2f c; c.x = a.l; c.y = a.h;
    const fj_v2f t = __builtin_elementwise_fma(slab32q_planes(w, slab32_shift(a.i)), (fj_v2f) (a.i), c);
    put_axis(a, t.x, t.y, out + 5 * k);
  }
}

// (b) whole-box verdict and tnear.  rays [n][8]: o xyz, inv xyz, tmin, tmax (f64; the entries round the range outward with f32_below /
// f32_above as the walks do).  consts [n][9] (may be null): (i, l, h) of x, y, z.
// quantised: grid [n][6] g0 xyz, cell xyz; words [n][3]; verdict bit 0: the Slab32 overload, bit 1: the Slab32P overload
void fj_slab32q_box_batch(int64_t n, const double *rays, const double *grid, const uint32_t *words, uint8_t *verdict, float *tnear, float *consts)
{
  for (int64_t k = 0; k < n; k++) {
    const double *r = rays + 8 * k, *g = grid + 6 * k;
    const uint32_t *w = words + 3 * k;
    V3 o, inv;
    get_ray(r, &o, &inv);
    const Slab32 s = slab32q_setup(o, inv, g, g + 3);
    const uint32_t shx = slab32_shift(s.x.i), shy = slab32_shift(s.y.i), shz = slab32_shift(s.z.i);
    const float tmin32 = f32_below(r[6]), tmax32 = f32_above(r[7]);
    float tn = 0.f;
    const bool v0 = slab32q_test(w[0], w[1], w[2], s, shx, shy, shz, tmin32, tmax32, &tn);
    const bool v1 = slab32q_test(w[0], w[1], w[2], slab32p(s), shx, shy, shz, tmin32, tmax32);
    verdict[k] = (uint8_t) ((v0 ? 1 : 0) | (v1 ? 2 : 0));
    tnear[k] = tn;
    if (consts) put_consts(s, consts + 9 * k);
  }
}
// f32 boxes: bounds [n][6] min xyz, max xyz of the primitive set; boxes [n][6]: (min, max) pairs of x, y, z
void fj_slab32_box_batch(int64_t n, const double *rays, const double *bounds, const float *boxes, uint8_t *verdict, float *tnear, float *consts)
{
  for (int64_t k = 0; k < n; k++) {
    const double *r = rays + 8 * k;
    const float *b = boxes + 6 * k;
    V3 o, inv;
    get_ray(r, &o, &inv);
    const Slab32 s = slab32_setup(o, inv, bounds + 6 * k);
    fj_v2f px, py, pz;
    px.x = b[0]; px.y = b[1]; py.x = b[2]; py.y = b[3]; pz.x = b[4]; pz.y = b[5];
    float tn = 0.f;
    verdict[k] = slab32_test(px, py, pz, s, f32_below(r[6]), f32_above(r[7]), &tn) ? 1 : 0;
    tnear[k] = tn;
    if (consts) put_consts(s, consts + 9 * k);
  }
}
// the f64 slab(): boxes [n][6] min xyz, max xyz
void fj_slab_f64_batch(int64_t n, const double *rays, const double *boxes, uint8_t *verdict, double *tnear)
{
  for (int64_t k = 0; k < n; k++) {
    const double *r = rays + 8 * k;
    V3 o, inv;
    get_ray(r, &o, &inv);
    double tn = 0;
    verdict[k] = slab(boxes + 6 * k, boxes + 6 * k + 3, o, inv, r[6], r[7], &tn) ? 1 : 0;
    tnear[k] = tn;
  }
}
// the record of fjgpu_dev_slab32_batch (include/fjgpu.h), computed here: rays as above (inv given), out [n] Slab32Probe (128 bytes each)
void fj_slab32_probe_batch(int64_t n, const double *rays, const double *grid, const uint32_t *words, void *out)
{
  for (int64_t k = 0; k < n; k++) slab32_probe(rays + 8 * k, grid + 6 * k, words + 3 * k, (Slab32Probe *) out + k);
}

// (c) the quantiser: k_quantize_nodes on an array of DNode (128 bytes each) -> DNodeQ (64 bytes each)
void fj_slab32_quantize_batch(int64_t n, const void *nodes, const double *origin, const double *cell, void *out)
{
  const DNode *nd = (const DNode *) nodes;
  DNodeQ *oq = (DNodeQ *) out;
  for (int64_t i = 0; i < n; i++) {
    DNodeQ q;
    for (int k = 0; k < 4; k++) {
      q.child[k] = nd[i].child[k];
      for (int a = 0; a < 3; a++)
        slab32_quantize_axis((double) nd[i].box[k][2 * a], (double) nd[i].box[k][2 * a + 1], origin[a], cell[a], &q.q[k][2 * a], &q.q[k][2 * a + 1]);
    }
    oq[i] = q;
  }
}

}
