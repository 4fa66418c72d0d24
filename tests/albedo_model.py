"""numpy restatement of the albedo AOV and of albedo-demodulated denoising (include/fjgpu.h: fjgpu_render_aov_albedo,
fjgpu_denoise_albedo), written from the header's text.

Per sample that hits, in f32, every product one multiply:
    no shader / unknown type   NO_SHADER_COLOR = (0.5, 1, 0)
    ConstantShader             diffuse * tex(texture) where it has one, else diffuse
    PlasticShader              diffuse * tex(diffuse_map), or diffuse
    PathtracingShader          (Cd * tex(diffuse_map)) * diffuse
    HairShader                 Cd * diffuse
    GlassShader                (1, 1, 1)
with the shader from the slot rule of ObjectInstance::GetShader, tex(i) the nearest tap of Texture::Lookup at the f32 texture
coordinates of Mesh::ray_intersect (0, 0 without uv), Cd = 1 on a mesh.  A pixel's albedo is the f64 mean over its OWN
rate_x * rate_y samples, a miss counting 0, rounded to f32 once.

The samples come from the oracle's `trace` of the device's own camera rays (Scene.camera_samples), the barycentrics are recomputed
with TriRayIntersect's statements and checked against the oracle's t, as tests/test_gpu_aov.py does for its buffers.  The oracle's
trace does not hand out a curve's parameter, so the albedo of a curve sample is not computed here: pixels holding one are flagged
(`on_curve`) and get a range check.
"""
import ctypes as C

import numpy as np

import denoise_model
from test_gpu_aov import _Scene, _Xf, _cross, _dot, _xpoint, _xvector, sampler_margin, shader_slot
from fujiyama_renderer_amd import gpu

NO_SHADER_COLOR = np.array([0.5, 1.0, 0.0], dtype=np.float32)
NO_TEXTURE_COLOR = np.array([1.0, 0.63, 0.63], dtype=np.float32)
SHADER_NONE, SHADER_PLASTIC, SHADER_CONSTANT, SHADER_GLASS, SHADER_HAIR, SHADER_PATHTRACING = range(6)
F32 = np.float32


class _Texture(C.Structure):       # fj_texture_desc
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("nchannels", C.c_int32), ("tilesize", C.c_int32), ("tiles", C.POINTER(C.c_float))]


class _Shader(C.Structure):        # fj_shader_desc
    _fields_ = [("type", C.c_int32), ("diffuse", C.c_float * 3), ("specular", C.c_float * 3), ("ambient", C.c_float * 3),
                ("reflect", C.c_float * 3), ("refract", C.c_float * 3), ("emission", C.c_float * 3), ("filter_color", C.c_float * 3),
                ("roughness", C.c_float), ("ior", C.c_float), ("opacity", C.c_float), ("bump_amplitude", C.c_float),
                ("do_reflect", C.c_int32), ("do_color_filter", C.c_int32), ("diffuse_map", C.c_int32), ("bump_map", C.c_int32),
                ("texture", C.c_int32)]


def make_texture(width, height, nchannels, tilesize, tiles):
    return dict(width=int(width), height=int(height), nchannels=int(nchannels), tilesize=int(tilesize),
                tiles=None if tiles is None else np.ascontiguousarray(tiles, dtype=np.float32).ravel())


class Tables(object):
    """copies of the shader and texture tables of a scene description, and the colours of its curve sets' control points"""

    def __init__(self, sp):
        d = C.cast(sp, C.POINTER(_Scene)).contents
        _, n_curves, n_tex, n_sh, _, _, _ = list(d.n)
        tex = C.cast(d.textures, C.POINTER(_Texture))
        self.textures = []
        for k in range(n_tex):
            t = tex[k]
            n = (t.width // t.tilesize) * (t.height // t.tilesize) * t.tilesize * t.tilesize * t.nchannels if t.width > 0 and t.tilesize > 0 else 0
            tiles = np.ctypeslib.as_array(t.tiles, shape=(n,)).copy() if n and bool(t.tiles) else None
            self.textures.append(make_texture(t.width, t.height, t.nchannels, t.tilesize, tiles))
        sh = C.cast(d.shaders, C.POINTER(_Shader))
        self.shaders = [dict(type=int(sh[k].type), diffuse=np.array(list(sh[k].diffuse), dtype=np.float32), diffuse_map=int(sh[k].diffuse_map),
                             texture=int(sh[k].texture)) for k in range(n_sh)]
        self.curve_cd = []
        for k in range(n_curves):
            c = d.curves[k]
            cd = C.cast(c.Cd, C.POINTER(C.c_float))
            self.curve_cd.append(np.ctypeslib.as_array(cd, shape=(c.n_points, 3)).copy() if bool(c.Cd) else np.zeros((1, 3), np.float32))

    def map_of(self, sid):
        """the texture a shader's colour looks up, or -1"""
        if sid < 0:
            return -1
        s = self.shaders[sid]
        if s["type"] == SHADER_CONSTANT:
            return s["texture"]
        if s["type"] in (SHADER_PLASTIC, SHADER_PATHTRACING):
            return s["diffuse_map"]
        return -1


def texel_index(tex, u, v):
    """Texture::Lookup's tap (src/fj_texture.cc:51-78, MipInput::ReadTile's clamp) for f32 arrays u, v -> the index of the texel's first
    channel in the tile-major array; -1 where the tap falls outside the tile's stored pixels (the lookup returns zeros there)"""
    u, v = np.asarray(u, dtype=F32), np.asarray(v, dtype=F32)
    ts = tex["tilesize"]
    xnt, ynt = tex["width"] // ts, tex["height"] // ts
    tu = u - np.floor(u)
    tv = v - np.floor(v)
    su = tu * F32(xnt)
    sv = (F32(1) - tv) * F32(ynt)
    xt = np.clip(np.floor(su).astype(np.int64), 0, xnt - 1)
    yt = np.clip(np.floor(sv).astype(np.int64), 0, ynt - 1)
    xp = ((su - np.floor(su)) * F32(64)).astype(np.int64)          # (C's conversion truncates; the values are >= 0)
    yp = ((sv - np.floor(sv)) * F32(64)).astype(np.int64)
    inside = (xp >= 0) & (xp < ts) & (yp >= 0) & (yp < ts)
    at = ((yt * xnt + xt) * ts * ts + (yp * ts + xp)) * tex["nchannels"]
    return np.where(inside, at, -1)


def tex_lookup(tex, u, v):
    """rgb [n, 3] f32 of the nearest tap; NO_TEXTURE_COLOR for a texture that is not open (width 0), zeros outside the tile"""
    u = np.atleast_1d(np.asarray(u, dtype=F32))
    v = np.atleast_1d(np.asarray(v, dtype=F32))
    if tex["width"] == 0 or tex["tiles"] is None:
        return np.tile(NO_TEXTURE_COLOR, (u.size, 1))
    at = texel_index(tex, u, v)
    ok = at >= 0
    a = np.where(ok, at, 0)
    t, nch = tex["tiles"], tex["nchannels"]
    if nch == 1:
        rgb = np.stack([t[a], t[a], t[a]], axis=1)
    elif nch in (3, 4):
        rgb = np.stack([t[a], t[a + 1], t[a + 2]], axis=1)
    else:
        rgb = np.zeros((u.size, 3), dtype=F32)
    return np.where(ok[:, None], rgb, F32(0)).astype(F32)


def shader_albedo(tab, sid, tu, tv, Cd=None):
    """the table of the module docstring for n samples of ONE shader (sid < 0: none): tu, tv f32 [n], Cd f32 [n, 3] or None = ones"""
    tu = np.atleast_1d(np.asarray(tu, dtype=F32))
    n = tu.size
    if sid < 0:
        return np.tile(NO_SHADER_COLOR, (n, 1))
    s = tab.shaders[sid]
    diffuse = s["diffuse"]
    Cd = np.ones((n, 3), dtype=F32) if Cd is None else np.asarray(Cd, dtype=F32)
    m = tab.map_of(sid)
    dm = tex_lookup(tab.textures[m], tu, tv) if m >= 0 else None
    if s["type"] == SHADER_CONSTANT:
        return (dm * diffuse[None, :]).astype(F32) if dm is not None else np.tile(diffuse, (n, 1))
    if s["type"] == SHADER_PLASTIC:
        return (diffuse[None, :] * dm).astype(F32) if dm is not None else np.tile(diffuse, (n, 1))
    if s["type"] == SHADER_PATHTRACING:
        cdm = (Cd * dm).astype(F32) if dm is not None else Cd
        return (cdm * diffuse[None, :]).astype(F32)
    if s["type"] == SHADER_HAIR:
        return (Cd * diffuse[None, :]).astype(F32)
    if s["type"] == SHADER_GLASS:
        return np.ones((n, 3), dtype=F32)
    return np.tile(NO_SHADER_COLOR, (n, 1))


def _ulp_neighbours_select_another_texel(tex, tu, tv):
    """a sample is fragile when (tu, tv) moved by one f32 ulp either way on either axis selects a different texel"""
    if tex["width"] == 0 or tex["tiles"] is None:
        return np.zeros(tu.shape, dtype=bool)
    here = texel_index(tex, tu, tv)
    frag = np.zeros(tu.shape, dtype=bool)
    for du, dv in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        uu = np.nextafter(tu, F32(np.inf * du)) if du else tu
        vv = np.nextafter(tv, F32(np.inf * dv)) if dv else tv
        frag |= texel_index(tex, uu, vv) != here
    return frag


def sample_albedo(view, tab, rays, t, ids):
    """per-sample albedo of traced camera rays: rays [n, 8], the oracle's t [n] and ids [n, 2] ->
    (albedo [n, 3] f32 (0 for a miss and for a curve hit), curve [n], fragile [n], textured [n])"""
    n = rays.shape[0]
    alb = np.zeros((n, 3), dtype=F32)
    curve = np.zeros(n, dtype=bool)
    fragile = np.zeros(n, dtype=bool)
    textured = np.zeros(n, dtype=bool)
    hit = ids[:, 0] >= 0
    for ii in np.unique(ids[hit, 0]):
        I = view.instances[int(ii)]
        sel = np.nonzero(hit & (ids[:, 0] == ii))[0]
        if I["curve"]:
            curve[sel] = True
            continue
        m = view.meshes[I["primset"]]
        f = ids[sel, 1]
        ix = m["ix"][f]
        sg = m["fg"][f] if m["fg"] is not None else np.zeros(f.size, dtype=np.int32)
        sid = np.array([shader_slot(I, int(g)) for g in sg])
        tu = np.zeros(sel.size, dtype=F32)
        tv = np.zeros(sel.size, dtype=F32)
        if m["uv"] is not None:
            o, dd = rays[sel, 0:3], rays[sel, 3:6]
            p0, p1, p2 = m["P"][ix[:, 0]], m["P"][ix[:, 1]], m["P"][ix[:, 2]]
            oo, od = _xpoint(I["Minv"], o), _xvector(I["Minv"], dd)
            e1, e2 = p1 - p0, p2 - p0
            pvec = _cross(od, e2)
            inv_det = 1.0 / _dot(e1, pvec)
            tvec = oo - p0
            u = _dot(tvec, pvec) * inv_det
            qvec = _cross(tvec, e1)
            v = _dot(od, qvec) * inv_det
            assert np.allclose(_dot(e2, qvec) * inv_det, t[sel], rtol=1e-12, atol=1e-12)      # (the test's own reference, checked first)
            t0, t1, t2 = m["uv"][ix[:, 0]], m["uv"][ix[:, 1]], m["uv"][ix[:, 2]]
            tb = (1 - u - v).astype(F32)                   # f32 barycentric, src/fj_mesh.cc:285
            uv = ((tb[:, None] * t0).astype(np.float64) + u[:, None] * t1.astype(np.float64) + v[:, None] * t2.astype(np.float64)).astype(F32)
            tu, tv = uv[:, 0], uv[:, 1]
        for s in np.unique(sid):
            w = sid == s
            alb[sel[w]] = shader_albedo(tab, int(s), tu[w], tv[w])
            mp = tab.map_of(int(s))
            if mp >= 0:
                textured[sel[w]] = True
                # (a mesh without uv: the coordinates are the constants 0, 0 on both sides, not a rounded sum -- nothing to be fragile about)
                if m["uv"] is not None:
                    fragile[sel[w]] = _ulp_neighbours_select_another_texel(tab.textures[mp], tu[w], tv[w])
    return alb, curve, fragile, textured


def own_sample_indices(rd, rect):
    """[h, w, ry * rx] indices k = y * nx + x of every pixel's own samples in its tile (FixedGridSampler's window without the margin)"""
    xmin, ymin, xmax, ymax = rect
    w, h = xmax - xmin, ymax - ymin
    mx, my = sampler_margin(rd)
    rx, ry = rd.rate_x, rd.rate_y
    nx, ny = rx * w + 2 * mx, ry * h + 2 * my
    kk = np.arange(nx * ny).reshape(ny, nx)[my:my + ry * h, mx:mx + rx * w].reshape(h, ry, w, rx).transpose(0, 2, 1, 3).reshape(h, w, ry * rx)
    return kk, nx * ny


def pixel_mean(alb, kk):
    """f64 mean over a pixel's own samples, rounded to f32 once: alb [n, 3] f32, kk [h, w, s] -> ([h, w, 3] f32, [h, w, 3] f64)"""
    mean = alb[kk].astype(np.float64).sum(axis=2) / np.float64(kk.shape[2])
    return mean.astype(F32), mean


class OracleSamples(object):
    """stands where the device scene is expected (camera_samples) when there is no device: the oracle's sampler and camera"""

    def __init__(self, sp):
        self.sp = sp

    def camera_samples(self, rd, tile):
        return oracle_camera_samples(self.sp, rd, gpu.tile_rect(rd, int(tile)))


def expected_albedo(gs, osc, view, tab, rd, tiles, prefill=0.0):
    """-> dict: albedo [H, W, 3] f32 (prefill outside the listed tiles), mean64, and the pixel masks uniform (every own sample hits a
    mesh with one albedo: EQUAL asked), mesh (own hits all on meshes, at least one), on_curve (holds a curve sample), fragile (holds a
    sample whose texel a one-ulp move of its uv changes), textured (holds a sample of a shader with a map), all_curve, touched (in a
    listed tile), coverage, amax; n_rays = rays traced"""
    H, W = rd.yres, rd.xres
    out = dict(albedo=np.full((H, W, 3), prefill, dtype=F32), mean64=np.zeros((H, W, 3)), coverage=np.zeros((H, W)),
               n_rays=0)
    out["amax"] = np.zeros((H, W, 3), dtype=F32)          # the largest albedo among a pixel's own samples (curve samples: 0)
    for name in ("uniform", "mesh", "on_curve", "all_curve", "fragile", "textured", "touched"):
        out[name] = np.zeros((H, W), dtype=bool)
    for tile in tiles:
        rect = gpu.tile_rect(rd, int(tile))
        kk, n = own_sample_indices(rd, rect)
        rays = gs.camera_samples(rd, int(tile))
        assert rays.shape == (n, 8)
        out["n_rays"] += n
        t, ids, _ = osc.trace(view.target_group, rays)
        alb, curve, fragile, textured = sample_albedo(view, tab, rays, t, ids)
        sl = (slice(rect[1], rect[3]), slice(rect[0], rect[2]))
        a32, a64 = pixel_mean(alb, kk)
        hit = ids[:, 0] >= 0
        out["albedo"][sl] = a32
        out["mean64"][sl] = a64
        out["coverage"][sl] = hit[kk].mean(axis=2)
        out["on_curve"][sl] = curve[kk].any(axis=2)
        out["fragile"][sl] = fragile[kk].any(axis=2)
        out["textured"][sl] = textured[kk].any(axis=2)
        out["mesh"][sl] = hit[kk].any(axis=2) & ~curve[kk].any(axis=2)
        out["uniform"][sl] = hit[kk].all(axis=2) & ~curve[kk].any(axis=2) & (alb[kk] == alb[kk][:, :, :1]).all(axis=(2, 3))
        out["all_curve"][sl] = curve[kk].all(axis=2)
        out["amax"][sl] = alb[kk].max(axis=2)
        out["touched"][sl] = True
    return out


class _Cam(C.Structure):           # fj_camera_desc
    _fields_ = [("xform", _Xf), ("fov", C.c_double), ("znear", C.c_double), ("zfar", C.c_double)]


class _SceneCam(C.Structure):      # fj_scene_desc, the camera included
    _fields_ = list(_Scene._fields_) + [("camera", _Cam)]


def oracle_camera_samples(sp, rd, rect):
    """a tile's camera rays [n, 8] without a device: the oracle's sampler and camera (fjo_tile_samples, fjo_camera_rays), static camera"""
    import oracle_ffi
    O = oracle_ffi.lib()
    cam = C.cast(sp, C.POINTER(_SceneCam)).contents.camera
    r4 = (C.c_int32 * 4)(*[int(v) for v in rect])
    nxy = (C.c_int32 * 2)()
    n = O.fjo_tile_samples(C.byref(rd), r4, None, 0, nxy)
    uvt = np.empty((n, 3))
    assert O.fjo_tile_samples(C.byref(rd), r4, uvt.ctypes.data_as(C.c_void_p), n, nxy) == n
    out = np.empty((n, 8))
    O.fjo_camera_rays(C.byref(cam), int(rd.xres), int(rd.yres), n, uvt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def demodulate(color, albedo, albedo_floor, region=None):
    """(D, a'): rgb of the region divided by the clamped albedo in f32, alpha and the pixels outside the region as they are"""
    color = np.ascontiguousarray(color, dtype=F32)
    H, W = color.shape[:2]
    x0, y0, x1, y1 = (0, 0, W, H) if region is None else region
    a = np.ones((H, W, 3), dtype=F32)
    al = np.asarray(albedo, dtype=F32)[y0:y1, x0:x1]
    with np.errstate(invalid="ignore"):
        a[y0:y1, x0:x1] = np.where(al > F32(albedo_floor), al, F32(albedo_floor))
    D = color.copy()
    D[y0:y1, x0:x1, :3] = color[y0:y1, x0:x1, :3] / a[y0:y1, x0:x1]
    return D, a


def demodulated_denoise(color, normal=None, position=None, ids=None, albedo=None, albedo_floor=1e-4, region=None, **kw):
    """clamp, divide, denoise_model.denoise, multiply"""
    if albedo is None:
        return denoise_model.denoise(color, normal, position, ids, region=region, **kw)
    D, a = demodulate(color, albedo, albedo_floor, region)
    F = denoise_model.denoise(D, normal, position, ids, region=region, **kw)
    H, W = F.shape[:2]
    x0, y0, x1, y1 = (0, 0, W, H) if region is None else region
    out = F.copy()
    out[y0:y1, x0:x1, :3] = F[y0:y1, x0:x1, :3] * a[y0:y1, x0:x1]
    return out
