// fjgpu_dev_aov.h -- the first-hit AOV pass (fjgpu_render_aov, include/fjgpu.h): the samples of a pixel reduced to the nearest one,
// its geometry written out.  Part of the kernels translation unit: included by fjgpu_kernels.hip only (device code, compiled with
// -ffp-contract=off; see the header of that file).
#ifndef FJGPU_DEV_AOV_H
#define FJGPU_DEV_AOV_H

// ---------------------------------------------------------------- k_aov_reduce
// One wave per pixel, like k_resolve -- but over the pixel's OWN rate_x * rate_y samples, not its filter window: the lanes take them
// row-major (a load instruction covers whole sample rows: rate_x hit records of 32 bytes, contiguous), each lane keeps the smallest
// (t, k) it has seen -- k = index of the sample in its tile, so that equal t resolves to the sample generated first -- and counts its
// hits; a butterfly reduces the pairs lexicographically and adds the counts.  Lane 0 then fetches the winner's hit record, ray and
// instance and computes the attributes with the statements k_shade uses for its hit (fjgpu_dev_shade.h: trace_surface's
// SurfaceInput setup) -- restated here, not shared: the shading kernel keeps compiling to what it compiles to.
// The attribute tail is one lane of 64 (dependent gathers: hit -> instance -> indices -> normals); the reduction reads 12 bytes of every
// sample's 32-byte hit record.  C3 at full size: 3.1 ms for 141 M samples, a sixth of the walk in front of it (profiles/aov_pass.txt).
__global__ void __launch_bounds__(BLOCK) k_aov_reduce(DScene S, AovParams ap, const TileDesc *tiles, const DRay *rays, const DHit *hits)
{
  const TileDesc T = tiles[blockIdx.y];
  const int tw = T.xmax - T.xmin, th = T.ymax - T.ymin;
  const int pk = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);     // pixel of this wave
  if (pk >= tw * th) return;
  const unsigned lane = __lane_id();
  const int px = T.xmin + pk % tw, py = T.ymin + pk / tw;
  // first own sample of the pixel: FixedGridSampler's window without its margin
  const uint32_t k0 = (uint32_t) (ap.margin_y + (py - T.ymin) * ap.rate_y) * (uint32_t) T.nx + (uint32_t) (ap.margin_x + (px - T.xmin) * ap.rate_x);
  const int nown = ap.rate_x * ap.rate_y;
  const FJ_GLOBAL DHit *gh = FJ_G(DHit, hits) + T.sample_offset;

  double best_t = DBL_MAX;
  uint32_t best_k = 0xffffffffu;       // no hit so far
  uint32_t nhit = 0;
  for (int w = (int) lane; w < nown; w += 64) {
    const int sy = w / ap.rate_x, sx = w - sy * ap.rate_x;
    const uint32_t k = k0 + (uint32_t) sy * (uint32_t) T.nx + (uint32_t) sx;
    const int inst = gh[k].inst;
    const double t = gh[k].t;
    if (inst >= 0) {
      nhit++;
      if (t < best_t || (t == best_t && k < best_k)) { best_t = t; best_k = k; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ot = __shfl_xor(best_t, off);
    const uint32_t ok = __shfl_xor(best_k, off);
    nhit += __shfl_xor(nhit, off);
    if (ot < best_t || (ot == best_t && ok < best_k)) { best_t = ot; best_k = ok; }
  }
  if (lane != 0) return;

  const size_t at = (size_t) py * ap.xres + px;
  float depth = INFINITY;
  float Pf[3] = {0.f, 0.f, 0.f}, Nf[3] = {0.f, 0.f, 0.f}, tuv[2] = {0.f, 0.f};
  int32_t id[4] = {-1, -1, -1, -1};
  if (best_k != 0xffffffffu) {
    const FJ_GLOBAL DHit *hp = gh + best_k;
    DHit h;
    h.t = hp->t; h.u = hp->u; h.v = hp->v; h.inst = hp->inst; h.prim = hp->prim;
    const FJ_GLOBAL double *rp = FJ_G(double, rays) + 6 * ((size_t) T.sample_offset + best_k);      // DRay: o xyz, d xyz
    const DInstance *I = &S.instances[h.inst];
    const V3 ro = ld3(rp), rd = ld3(rp + 3);
    const double *IM = I->M, *IMinv = I->Minv;       // static scenes only: the host-built matrices
    const V3 oo = xpoint(IMinv, ro);
    const V3 od = xvector(IMinv, rd);
    V3 N = mk(0, 0, 0);
    float tu = 0.f, tv = 0.f;
    int sg = 0;
    if (I->sh_type != FJ_PRIMSET_CURVE) {
      // --- Mesh::ray_intersect attribute part (src/fj_mesh.cc:267-305) in object space
      int i0 = 0, i1 = 0, i2 = 0;
      if (!I->sh_vN || I->sh_uv) { const FJ_GLOBAL int32_t *ix = FJ_G(int32_t, I->sh_indices) + 3 * (size_t) h.prim; i0 = ix[0]; i1 = ix[1]; i2 = ix[2]; }
      V3 n0 = mk(0, 0, 0), n1 = n0, n2 = n0;
      // compute_shading_normal, src/fj_mesh.cc:108-120: per-corner normals where the mesh has them, else its point normals
      if (I->sh_vN) { const FJ_GLOBAL double *vn = FJ_G(double, I->sh_vN) + 9 * (size_t) h.prim; n0 = ld3(vn); n1 = ld3(vn + 3); n2 = ld3(vn + 6); }
      else if (I->sh_N) { n0 = ld3(FJ_G(double, I->sh_N) + 3 * (size_t) i0); n1 = ld3(FJ_G(double, I->sh_N) + 3 * (size_t) i1); n2 = ld3(FJ_G(double, I->sh_N) + 3 * (size_t) i2); }
      N = (1 - h.u - h.v) * n0 + h.u * n1 + h.v * n2;            // TriComputeNormal, src/fj_triangle.cc:44-49
      if (I->sh_uv) {
        const float t0u = FJ_G(float, I->sh_uv)[2 * (size_t) i0], t0v = FJ_G(float, I->sh_uv)[2 * (size_t) i0 + 1];
        const float t1u = FJ_G(float, I->sh_uv)[2 * (size_t) i1], t1v = FJ_G(float, I->sh_uv)[2 * (size_t) i1 + 1];
        const float t2u = FJ_G(float, I->sh_uv)[2 * (size_t) i2], t2v = FJ_G(float, I->sh_uv)[2 * (size_t) i2 + 1];
        const float tt = (float) (1 - h.u - h.v);                  // f32 barycentric, src/fj_mesh.cc:285
        tu = (float) (tt * t0u + h.u * t1u + h.v * t2u);
        tv = (float) (tt * t0v + h.u * t1v + h.v * t2v);
      }
      sg = I->sh_face_group ? FJ_G(int32_t, I->sh_face_group)[h.prim] : 0;
    }
    // (a curve hit: N / uv stay zero as Curve::ray_intersect leaves them, src/fj_curve.cc:211-229; the shading group is 0)
    V3 Pw = oo + h.t * od;                                       // RayPointAt in object space
    // --- ObjectInstance::RayIntersect back-transform (src/fj_object_instance.cc:231-240)
    Pw = xpoint(IM, Pw);
    N = normalize(xvector(IM, N));                               // (normalize leaves a zero vector as it is)
    // --- shader lookup: ObjectInstance::GetShader (src/fj_object_instance.cc:177-191)
    int sid;
    if (sg < 0 || sg >= I->n_shaders) sid = I->shaders[0];
    else { sid = I->shaders[sg]; if (sid < 0) sid = I->shaders[0]; }

    depth = (float) h.t;
    Pf[0] = (float) Pw.x; Pf[1] = (float) Pw.y; Pf[2] = (float) Pw.z;
    Nf[0] = (float) N.x; Nf[1] = (float) N.y; Nf[2] = (float) N.z;
    tuv[0] = tu; tuv[1] = tv;
    id[0] = h.inst; id[1] = h.prim; id[2] = sg; id[3] = sid < 0 ? -1 : sid;
  }
  if (ap.depth) ap.depth[at] = depth;
  if (ap.position) { ap.position[3 * at] = Pf[0]; ap.position[3 * at + 1] = Pf[1]; ap.position[3 * at + 2] = Pf[2]; }
  if (ap.normal) { ap.normal[3 * at] = Nf[0]; ap.normal[3 * at + 1] = Nf[1]; ap.normal[3 * at + 2] = Nf[2]; }
  if (ap.uv) { ap.uv[2 * at] = tuv[0]; ap.uv[2 * at + 1] = tuv[1]; }
  if (ap.ids) { ap.ids[4 * at] = id[0]; ap.ids[4 * at + 1] = id[1]; ap.ids[4 * at + 2] = id[2]; ap.ids[4 * at + 3] = id[3]; }
  if (ap.coverage) ap.coverage[at] = (float) nhit / (float) nown;
}

#endif
