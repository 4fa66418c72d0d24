// fjgpu_dev_albedo.h -- the albedo AOV (fjgpu_render_aov_albedo, include/fjgpu.h): the surface colour of every camera sample, without
// light, averaged over the pixel's OWN samples.  Part of the kernels translation unit: included by fjgpu_kernels.hip only (device code,
// compiled with -ffp-contract=off; see the header of that file), after fjgpu_dev_aov.h.
#ifndef FJGPU_DEV_ALBEDO_H
#define FJGPU_DEV_ALBEDO_H

// Albedo of one sample that hit, with the statements k_shade uses for the same quantities (fjgpu_dev_shade.h) -- restated here, not shared,
// as in fjgpu_dev_aov.h: the shading kernel keeps compiling to what it compiles to.  Every product is ONE f32 multiply.  The dependent
// gathers: hit (the caller's) -> instance -> face group, shader -> indices, uv (only where the shader looks up a texture) -> texel.
__device__ __forceinline__ void aov_sample_albedo(const DScene &S, int inst, int prim, double hu, double hv, float a[3])
{
  const FJ_GLOBAL DInstance *I = FJ_G(DInstance, S.instances) + inst;
  const bool curve = I->sh_type == FJ_PRIMSET_CURVE;
  // --- shader lookup: ObjectInstance::GetShader (src/fj_object_instance.cc:177-191); a curve hit's shading group is 0
  int sg = 0;
  if (!curve && I->sh_face_group) sg = FJ_G(int32_t, I->sh_face_group)[prim];
  int sid;
  if (sg < 0 || sg >= I->n_shaders) sid = I->shaders[0];
  else { sid = I->shaders[sg]; if (sid < 0) sid = I->shaders[0]; }
  a[0] = .5f; a[1] = 1.f; a[2] = 0.f;                              // NO_SHADER_COLOR, src/fj_shading.cc:24
  if (sid < 0) return;
  const FJ_GLOBAL fj_shader_desc *sh = FJ_G(fj_shader_desc, S.shaders) + sid;
  const int type = sh->type;
  const float d0 = sh->diffuse[0], d1 = sh->diffuse[1], d2 = sh->diffuse[2];
  int map = -1;                                                    // the texture this shader's colour looks up, if any
  if (type == FJ_SHADER_CONSTANT) map = sh->texture;
  else if (type == FJ_SHADER_PLASTIC || type == FJ_SHADER_PATHTRACING) map = sh->diffuse_map;

  float Cd[3] = {1.f, 1.f, 1.f};                                   // Intersection default
  float tu = 0.f, tv = 0.f;
  if (curve) {
    // Curve::ray_intersect (src/fj_curve.cc:211-229): Cd = lerp of the piece's end colours; hit.v is the piece, hit.u the parameter
    if (type == FJ_SHADER_HAIR || type == FJ_SHADER_PATHTRACING) {
      const FJ_GLOBAL DPrimSet *P = FJ_G(DPrimSet, S.primsets) + I->primset;
      const size_t sl = (size_t) hv;
      const float tl = (float) hu;
      const FJ_GLOBAL float *cd = FJ_G(float, P->curve_Cd) + sl * 6;
      Cd[0] = (1 - tl) * cd[0] + tl * cd[3];
      Cd[1] = (1 - tl) * cd[1] + tl * cd[4];
      Cd[2] = (1 - tl) * cd[2] + tl * cd[5];
    }
  } else if (map >= 0 && I->sh_uv) {
    // Mesh::ray_intersect (src/fj_mesh.cc:285-290): the f32 texture coordinates
    const FJ_GLOBAL int32_t *ix = FJ_G(int32_t, I->sh_indices) + 3 * (size_t) prim;
    const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
    const FJ_GLOBAL float *uv = FJ_G(float, I->sh_uv);
    const float t0u = uv[2 * (size_t) i0], t0v = uv[2 * (size_t) i0 + 1];
    const float t1u = uv[2 * (size_t) i1], t1v = uv[2 * (size_t) i1 + 1];
    const float t2u = uv[2 * (size_t) i2], t2v = uv[2 * (size_t) i2 + 1];
    const float tt = (float) (1 - hu - hv);
    tu = (float) (tt * t0u + hu * t1u + hv * t2u);
    tv = (float) (tt * t0v + hu * t1v + hv * t2v);
  }
  float dm[4] = {1.f, 1.f, 1.f, 1.f};
  if (map >= 0) tex_lookup(S.textures[map], tu, tv, dm);

  switch (type) {
  case FJ_SHADER_CONSTANT:                                         // constant_shader.cc:72-96
    if (map >= 0) { a[0] = dm[0] * d0; a[1] = dm[1] * d1; a[2] = dm[2] * d2; }
    else { a[0] = d0; a[1] = d1; a[2] = d2; }
    break;
  case FJ_SHADER_PLASTIC:                                          // plastic_shader.cc: diffuse * diffuse_map
    a[0] = d0 * dm[0]; a[1] = d1 * dm[1]; a[2] = d2 * dm[2];
    break;
  case FJ_SHADER_PATHTRACING: {                                    // pathtracing_shader.cc: (Cd * diffuse_map) * diffuse
    float Cdm[3] = {Cd[0], Cd[1], Cd[2]};
    if (map >= 0) { Cdm[0] *= dm[0]; Cdm[1] *= dm[1]; Cdm[2] *= dm[2]; }
    a[0] = Cdm[0] * d0; a[1] = Cdm[1] * d1; a[2] = Cdm[2] * d2;
    break;
  }
  case FJ_SHADER_HAIR:                                             // hair_shader.cc: Cd * diffuse
    a[0] = Cd[0] * d0; a[1] = Cd[1] * d1; a[2] = Cd[2] * d2;
    break;
  case FJ_SHADER_GLASS:
    a[0] = a[1] = a[2] = 1.f;
    break;
  default:                                                         // FJ_SHADER_NONE, unknown: NO_SHADER_COLOR
    break;
  }
}

// ---------------------------------------------------------------- k_aov_albedo
// The mean albedo of every pixel's own rate_x * rate_y samples (a miss counts 0), after k_aov_reduce on the same batch: the hit records are
// still there, and the barycentrics are in them -- no ray is read.  Unlike k_aov_reduce, whose attribute tail is one lane of 64, every lane
// does the dependent gathers of its samples.  G = ap.lanes lanes serve a pixel (a power of two, 1 .. 64: the smallest >= the sample count,
// so that 2 x 2 spp keeps all 64 lanes busy on 16 pixels instead of 4 lanes on one); a wave serves 64 / G consecutive pixels of the tile,
// a group's lanes stride over the pixel's samples.  Partial sums in f64 per lane, a butterfly over the offsets below G, one division in
// f64, one rounding to f32: a pixel whose samples share one albedo gets exactly that value (k a and (n a) / n are exact in f64), any other
// the f64 mean within an ulp of f32.  Lanes past the tile's last pixel stay in the butterfly (they add zeros) and write nothing.
// No atomics, no LDS, no scratch memory.
__global__ void __launch_bounds__(BLOCK) k_aov_albedo(DScene S, AlbedoParams ap, const TileDesc *tiles, const DHit *hits)
{
  const TileDesc T = tiles[blockIdx.y];
  const int tw = T.xmax - T.xmin, th = T.ymax - T.ymin;
  const int G = ap.lanes, shift = ap.lanes_log2;
  const int wave = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  if ((wave << (6 - shift)) >= tw * th) return;                    // uniform over the wave
  const unsigned lane = __lane_id();
  const int gl = (int) lane & (G - 1);                             // lane of its group
  const int pk = (wave << (6 - shift)) + ((int) lane >> shift);    // pixel of this group
  const bool live = pk < tw * th;
  const int px = live ? pk % tw : 0, py = live ? pk / tw : 0;      // (relative to the tile)
  const uint32_t k0 = (uint32_t) (ap.margin_y + py * ap.rate_y) * (uint32_t) T.nx + (uint32_t) (ap.margin_x + px * ap.rate_x);
  const int nown = live ? ap.rate_x * ap.rate_y : 0;
  const FJ_GLOBAL DHit *gh = FJ_G(DHit, hits) + T.sample_offset;

  double s0 = 0, s1 = 0, s2 = 0;
  for (int w = gl; w < nown; w += G) {
    const int sy = w / ap.rate_x, sx = w - sy * ap.rate_x;
    const FJ_GLOBAL DHit *hp = gh + (k0 + (uint32_t) sy * (uint32_t) T.nx + (uint32_t) sx);
    const int inst = hp->inst;
    if (inst < 0) continue;
    float a[3];
    aov_sample_albedo(S, inst, hp->prim, hp->u, hp->v, a);
    s0 += (double) a[0]; s1 += (double) a[1]; s2 += (double) a[2];
  }
  for (int off = G >> 1; off > 0; off >>= 1) {
    s0 += __shfl_xor(s0, off);
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
  }
  if (!live || gl != 0) return;
  const double n = (double) (ap.rate_x * ap.rate_y);
  FJ_GLOBAL float *out = (FJ_GLOBAL float *) ap.albedo + 3 * ((size_t) (T.ymin + py) * ap.xres + (size_t) (T.xmin + px));
  out[0] = (float) (s0 / n); out[1] = (float) (s1 / n); out[2] = (float) (s2 / n);
}

#endif
