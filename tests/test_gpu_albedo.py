"""GPU suite (-m gpu): the albedo AOV (include/fjgpu.h: fjgpu_render_aov_albedo) against tests/albedo_model.py over the CPU oracle's
trace of the device's own camera rays (Scene.camera_samples), as tests/test_gpu_aov.py does for the six geometry buffers.

Bounds.  A mesh-hit pixel whose own samples all hit and share one albedo must be EQUAL (k a and (n a) / n are exact in f64, whatever
the order of the sum).  Any other pixel without a curve sample must be within one f32 ulp of the expected f64 mean (the device adds the
same f32 values in f64 in another order: 1e-16 relative, which moves the f32 rounding by at most one ulp).  A pixel none of whose
samples hits is exactly 0.

Excluded pixels.  The texture coordinates are a rounded f64 sum of barycentrics the device and the test compute with the same
statements but not necessarily the same last bit (tests/test_gpu_aov.py gives uv one ulp), and a nearest-tap lookup turns such a bit
into another texel where the coordinate sits on a texel's edge.  A sample whose (tu, tv), moved by one f32 ulp either way on either
axis, selects another texel is fragile, a pixel holding one is left out, and at most 1 % of the textured pixels may be.  (On a mesh
WITHOUT uv the coordinates are the constants 0, 0 on both sides -- no sum, nothing to round -- so such a sample is never fragile:
the textured floor of the edge scenes has no uv and is compared in full.)  Counted on the CPU as well: tests/test_albedo_cpu.py.

Curve pixels.  The oracle's trace does not hand out the curve parameter, so a pixel holding a curve sample gets a range check per
channel: within [min, max] of Cd * diffuse over the curve sets where every sample is a curve hit, within [0, the largest of that and
the pixel's mesh samples] otherwise.  The lerp of two end colours and the product with diffuse are four f32 roundings: 4 ulp of slack.
"""
import numpy as np
import pytest

import albedo_model as am
import edge_scenes
import oracle_ffi
from fujiyama_renderer_amd import gpu, workloads
from test_gpu_aov import ALL, RAGGED, SENTINEL, SceneView, all_tiles, assert_aov, expected_aov, prepare, sampler_margin, shader_slot, ulp32

pytestmark = pytest.mark.gpu

EXCLUDED_CAP = 0.01
ALBEDO_SENTINEL = -7.5


def curve_range(view, tab):
    """[min, max] per channel of Cd * diffuse over the scene's curve instances, or None"""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for I in view.instances:
        if not I["curve"]:
            continue
        sid = shader_slot(I, 0)
        cd = tab.curve_cd[I["primset"]]
        a = am.shader_albedo(tab, sid, np.zeros(cd.shape[0], np.float32), np.zeros(cd.shape[0], np.float32), Cd=cd)
        lo, hi = np.minimum(lo, a.min(axis=0)), np.maximum(hi, a.max(axis=0))
    return None if not np.isfinite(lo).all() else (lo, hi)


def assert_albedo(got, e, view, tab, what=""):
    """got [H, W, 3] f32 against expected_albedo's dict over the touched pixels; returns the mask of compared mesh pixels"""
    assert got.dtype == np.float32 and got.shape == e["albedo"].shape
    T = e["touched"]
    left_out = T & e["fragile"]
    n_tex = int((T & e["textured"]).sum())
    print("albedo %s: %d pixels, %d uniform, %d textured, %d left out, %d with curve samples" % (
        what, int(T.sum()), int((T & e["uniform"]).sum()), n_tex, int(left_out.sum()), int((T & e["on_curve"]).sum())))
    assert int((left_out & e["textured"]).sum()) <= EXCLUDED_CAP * n_tex
    empty = T & (e["coverage"] == 0)
    assert not got[empty].any()
    equal = T & e["uniform"] & ~left_out
    assert np.array_equal(got[equal], e["albedo"][equal])
    near = T & ~e["on_curve"] & ~left_out & ~empty
    err = np.abs(got[near].astype(np.float64) - e["mean64"][near])
    bound = ulp32(e["mean64"][near])
    worst = float((err - bound).max()) if err.size else 0.0
    print("albedo %s: max |err| %.3e, max (err - one ulp) %.3e over %d pixels" % (what, float(err.max()) if err.size else 0.0, worst, int(near.sum())))
    assert worst <= 0
    on_curve = T & e["on_curve"]
    if on_curve.any():
        lo, hi = curve_range(view, tab)
        slack = 4 * ulp32(hi)
        g = got[on_curve].astype(np.float64)
        allc = e["all_curve"][on_curve]
        top = np.maximum(hi[None, :], e["amax"][on_curve].astype(np.float64)) + slack
        assert (g >= 0).all() and (g <= top).all()
        assert (g[allc] >= lo - slack).all() and (g[allc] <= hi + slack).all()
    return near


def run_case(text, tile_ids=None, want=gpu.AOV_ALL, prefill=None, options=()):
    """scene text -> dict(got buffers, stats, expected albedo, view, tables, rd, device scene closed)"""
    sp, rd = prepare(text)
    view, tab = SceneView(sp), am.Tables(sp)
    gs = gpu.Scene(sp)
    osc = oracle_ffi.OracleScene(sp)
    try:
        for name, value in options:
            gs.set_option(name, value)
        got, st = gs.render_aov_albedo(rd, tile_ids=tile_ids, want=want, prefill=prefill)
        tiles = all_tiles(rd) if tile_ids is None else tile_ids
        fill = prefill.get("albedo", 0) if isinstance(prefill, dict) else (prefill or 0)
        e = am.expected_albedo(gs, osc, view, tab, rd, tiles, prefill=fill)
        aov = expected_aov(gs, osc, view, rd, tiles, prefill if isinstance(prefill, dict) else None) if "ids" in want else None
    finally:
        osc.close()
        gs.close()
    return dict(got=got, st=st, e=e, view=view, tab=tab, rd=rd, aov=aov)


@pytest.fixture(scope="module")
def ragged(asset_dir):
    """the ragged frame of test_gpu_aov.py once, all seven buffers: the device scene stays open, the call and its expected values are shared"""
    sp, rd = prepare(workloads.buddhas(asset_dir, **RAGGED))
    view, tab = SceneView(sp), am.Tables(sp)
    gs = gpu.Scene(sp)
    osc = oracle_ffi.OracleScene(sp)
    got, st = gs.render_aov_albedo(rd, want=gpu.AOV_ALL)
    e = am.expected_albedo(gs, osc, view, tab, rd, all_tiles(rd))
    osc.close()
    yield dict(gs=gs, rd=rd, view=view, tab=tab, got=got, st=st, e=e)
    gs.close()


def test_ragged_frame(ragged):
    """several instances and shaders, ragged tiles, a filter margin, 3 x 2 = 6 samples on G = 8 lanes: the whole frame; silhouettes against
    the empty background hold coverage x surface, empty pixels 0"""
    rd, e, got = ragged["rd"], ragged["e"], ragged["got"]
    assert gpu.tile_count(rd) == 6 and sampler_margin(rd) != (0, 0) and rd.rate_x * rd.rate_y == 6
    assert sorted(got) == sorted(gpu.AOV_ALL)
    assert_albedo(got["albedo"], e, ragged["view"], ragged["tab"], "ragged")
    cov = got["coverage"][:, :, 0]
    assert np.array_equal(cov, e["coverage"].astype(np.float32))
    assert len(np.unique(got["albedo"][e["uniform"]], axis=0)) > 2                 # several shaders
    sil = (cov > 0) & (cov < 1)
    assert sil.sum() > 10 and (cov == 0).any()
    a, top = got["albedo"][sil], e["amax"][sil]
    lit = top > 0                                                                  # (a channel the surface has at all)
    assert (a[lit] > 0).all() and (a[lit] < top[lit]).all() and not a[~lit].any()
    assert not got["albedo"][cov == 0].any()
    assert ragged["st"].rays.camera == e["n_rays"] and ragged["st"].batches == 1


@pytest.mark.parametrize("res, spp, jitter, lanes", [((8, 6), (9, 8), 1, 64), ((24, 16), (1, 1), 0, 1), ((16, 12), (2, 2), 1, 4), ((8, 6), (8, 8), 1, 64),
                                                     ((12, 8), (4, 4), 1, 16), ((12, 8), (5, 1), 1, 8)])
def test_sample_counts(asset_dir, res, spp, jitter, lanes):
    """every lanes-per-pixel path: 72 samples (more than 64 lanes: the loop), 1 (no butterfly), 4, 64, and 16 and 5-on-8 in between"""
    r = run_case(workloads.buddhas(asset_dir, res=res, spp=spp, mesh="tiny", extra=(("sample_jitter", (jitter,)),)), want=("albedo", "coverage"))
    n = spp[0] * spp[1]
    assert lanes == min(64, 1 << (n - 1).bit_length())
    near = assert_albedo(r["got"]["albedo"], r["e"], r["view"], r["tab"], "%d x %d spp" % spp)
    assert near.sum() > 10 and r["st"].rays.camera == r["e"]["n_rays"]
    if n == 1:
        assert r["rd"].jitter == 0
        hit = r["e"]["coverage"] > 0
        assert np.array_equal(r["e"]["uniform"], hit) and np.array_equal(r["got"]["albedo"][hit], r["e"]["albedo"][hit])


def test_textured_scene(asset_dir):
    """a plastic floor with a diffuse map (a mesh without uv: one texel) and a dome whose constant shader looks up the sky map: textured
    pixels exist, their albedo varies, the exclusion cap holds"""
    r = run_case(edge_scenes.custom_scene(asset_dir, **edge_scenes.EDGE_CASES["textures_diffuse_and_bump"]))
    e, got = r["e"], r["got"]["albedo"]
    assert (r["rd"].xres, r["rd"].yres, r["rd"].rate_x, r["rd"].rate_y) == (64, 48, 2, 2)
    near = assert_albedo(got, e, r["view"], r["tab"], "textured")
    tex = e["textured"] & near
    assert tex.sum() > 1000
    assert len(np.unique(got[tex], axis=0)) > 50
    sid = r["got"]["ids"][:, :, 3]
    with_dmap = np.array([s["diffuse_map"] >= 0 for s in r["tab"].shaders] + [False])[sid]
    assert (with_dmap & near).sum() > 500                                           # the floor is among them
    assert int((e["textured"] & e["fragile"]).sum()) <= EXCLUDED_CAP * int(e["textured"].sum())


def test_face_groups_follow_the_slot_rule(asset_dir):
    """groups with an unassigned slot (B = 2) or an id past the shader list (D = 4) take slot 0's colour"""
    r = run_case(edge_scenes.custom_scene(asset_dir, **edge_scenes.EDGE_CASES["obj_face_groups"]))
    e, got, view, tab = r["e"], r["got"], r["view"], r["tab"]
    assert_albedo(got["albedo"], e, view, tab, "face groups")
    obj = [k for k, I in enumerate(view.instances) if not I["curve"] and view.meshes[I["primset"]]["fg"] is not None
           and view.meshes[I["primset"]]["fg"].max() > 0]
    assert len(obj) == 1
    I = view.instances[obj[0]]
    zero = np.zeros(1, np.float32)
    colour = lambda g: am.shader_albedo(tab, shader_slot(I, g), zero, zero)[0]
    slot0 = colour(0)
    assert np.array_equal(colour(2), slot0) and np.array_equal(colour(4), slot0) and not np.array_equal(colour(1), slot0)
    assert colour(3).tolist() == [1, 1, 1]                                          # C: the glass shader
    on_obj = e["uniform"] & (got["ids"][:, :, 0] == obj[0])
    # a uniform pixel's samples share one albedo, so the nearest sample's group names it
    seen = set()
    for g in (0, 1, 2, 3, 4):
        px = on_obj & (got["ids"][:, :, 2] == g)
        if px.any():
            seen.add(g)
            assert (got["albedo"][px] == colour(g)[None, :]).all(), g
    assert {1, 2, 4} <= seen


def test_glass_is_white(asset_dir):
    r = run_case(edge_scenes.custom_scene(asset_dir, **edge_scenes.EDGE_CASES["depth_limits"]))
    e, got, tab = r["e"], r["got"], r["tab"]
    assert_albedo(got["albedo"], e, r["view"], tab, "glass")
    glass = [k for k, s in enumerate(tab.shaders) if s["type"] == am.SHADER_GLASS]
    assert len(glass) == 1
    px = (got["ids"][:, :, 3] == glass[0]) & (got["coverage"][:, :, 0] == 1) & e["uniform"]
    assert px.sum() > 20 and (got["albedo"][px] == 1).all()


def test_cornell_pathtracing_walls(asset_dir):
    r = run_case(workloads.cornell(asset_dir, res=(32, 24), spp=(2, 2), mesh="tiny"))
    e, got, tab = r["e"], r["got"], r["tab"]
    near = assert_albedo(got["albedo"], e, r["view"], tab, "cornell")
    assert all(s["type"] == am.SHADER_PATHTRACING for s in tab.shaders)
    colours = {tuple(c) for c in got["albedo"][e["uniform"] & near].tolist()}
    d = float(np.float32(.8))
    assert (d, 0.0, 0.0) in colours and (0.0, d, 0.0) in colours and len(colours) >= 4          # the red and the green wall among them


def test_curves(asset_dir):
    r = run_case(workloads.furry(asset_dir, res=(32, 24), spp=(2, 2), mesh="furball", nlights=1))
    e, got = r["e"], r["got"]
    assert e["on_curve"].sum() > 10 and e["all_curve"].sum() > 0
    near = assert_albedo(got["albedo"], e, r["view"], r["tab"], "furry")
    assert (near & (e["coverage"] > 0)).sum() > 10                                  # mesh pixels, exact
    assert got["albedo"][e["all_curve"]].any()
    lo, hi = curve_range(r["view"], r["tab"])
    assert (hi > 0).any()


def test_region_and_tile_subset_leave_other_pixels_untouched(asset_dir):
    """a render region not aligned to the tiles, a subset of its tiles in reverse order, a sentinel in all seven buffers"""
    kw = dict(RAGGED)
    kw["extra"] = RAGGED["extra"] + (("render_region", (3, 2, 37, 23)),)
    text = workloads.buddhas(asset_dir, **kw)
    _, rd = prepare(text)
    n_tiles = gpu.tile_count(rd)
    subset = list(range(n_tiles))[::-1][::2]
    assert 1 < len(subset) < n_tiles
    fill = dict(SENTINEL, albedo=ALBEDO_SENTINEL)
    r = run_case(text, tile_ids=subset, prefill=fill)
    got, e = r["got"], r["e"]
    assert_albedo(got["albedo"], e, r["view"], r["tab"], "tile subset")
    exp, on_curve, n = r["aov"]
    assert_aov(got, exp, on_curve, r["view"])
    touched = e["touched"]
    assert touched.any() and not touched.all()
    for name in gpu.AOV_ALL:
        want = np.full((), fill[name], dtype=got[name].dtype)
        assert (got[name][~touched] == want).all(), name
    assert (got["albedo"][touched] != np.float32(ALBEDO_SENTINEL)).all()
    assert r["st"].rays.camera == n == e["n_rays"]


def test_batches_change_nothing(ragged):
    """one tile per batch: the albedo is the single batch's bit for bit, the six buffers are those of a call without albedo"""
    gs, rd = ragged["gs"], ragged["rd"]
    plain, _ = gs.render_aov(rd)
    gs.set_option("aov_batch_samples", 1)
    try:
        got, st = gs.render_aov_albedo(rd, want=gpu.AOV_ALL)
    finally:
        gs.set_option("aov_batch_samples", 0)
    assert st.batches == st.closest_launches == gpu.tile_count(rd) >= 3
    assert np.array_equal(got["albedo"], ragged["got"]["albedo"])
    for name in ALL:
        assert np.array_equal(got[name], plain[name]) and np.array_equal(ragged["got"][name], plain[name]), name
    assert st.rays.camera == ragged["st"].rays.camera


def test_albedo_alone(ragged):
    """want=("albedo",): the same bits, the beauty pass's camera rays, one walk"""
    gs, rd = ragged["gs"], ragged["rd"]
    got, st = gs.render_aov_albedo(rd, want=("albedo",))
    assert sorted(got) == ["albedo"] and np.array_equal(got["albedo"], ragged["got"]["albedo"])
    _, st_beauty = gs.render_frame(rd)
    assert st.rays.camera == st_beauty.rays.camera == ragged["st"].rays.camera
    assert st.closest_launches == st.batches == 1 and ragged["st"].closest_launches == ragged["st"].batches == 1
    assert st.resolve_ms > 0 and st.total_ms > 0


def test_refusals_name_the_entry_point(asset_dir):
    for text, why in ((workloads.buddhas(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny", extra=(("sampler_type", (1,)),)), "adaptive sampler"),
                      (workloads.motion(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny", kind="object"), "motion"),
                      (workloads.motion(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny", kind="camera"), "time-sampled camera")):
        sp, rd = prepare(text)
        gs = gpu.Scene(sp)
        try:
            with pytest.raises(gpu.GpuError, match="fjgpu_render_aov_albedo.*" + why):
                gs.render_aov_albedo(rd, want=gpu.AOV_ALL)
            with pytest.raises(gpu.GpuError, match="fjgpu_render_aov_albedo.*" + why):
                gs.render_aov_albedo(rd, want=("albedo",))
        finally:
            gs.close()


def test_does_not_disturb_rendering(asset_dir):
    """render_frame, render_aov_albedo(want=AOV_ALL), render_frame on the reproducible frame of test_gpu_aov.py: pixels, ray counts, work arena"""
    kw = dict(RAGGED, nlights=1)
    kw["extra"] = RAGGED["extra"] + (("max_reflect_depth", (0,)), ("max_refract_depth", (0,)))
    sp, rd = prepare(workloads.buddhas(asset_dir, **kw))
    gs = gpu.Scene(sp)
    try:
        fb0, st0 = gs.render_frame(rd)
        fb1, st1 = gs.render_frame(rd)
        work0 = gs.query("work_bytes")
        got, sta = gs.render_aov_albedo(rd, want=gpu.AOV_ALL)
        assert gs.query("work_bytes") == work0
        fb2, st2 = gs.render_frame(rd)
    finally:
        gs.close()
    assert fb1.any() and np.array_equal(fb0, fb1)          # (the premise: the frame is reproducible)
    assert np.array_equal(fb1, fb2)
    assert st0.rays.as_dict() == st1.rays.as_dict() == st2.rays.as_dict()
    assert sta.rays.camera == st1.rays.camera and sta.rays.total() == sta.rays.camera
    assert got["albedo"].any()
