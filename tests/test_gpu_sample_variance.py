"""GPU suite (-m gpu): fjgpu_render_tiles_variance (include/fjgpu.h), the beauty pass's sample variance.

1. Against the per-sample radiances.  The entry keeps no sample, so they are rendered: without jitter, sample (X, Y) of the coarse frame is
   pixel (X, Y) of the FINE frame -- rate times the resolution and the region, 1 x 1 sample per pixel, filter width 1 (a window of one
   sample of weight exp(0)) -- the same (u, v), the same camera ray, deterministic shading.  The premise is asserted first: the coarse
   beauty frame rebuilt from the fine frame with the filter's weights is the coarse beauty frame within 1e-5 (denoise_model.rel_err) on
   every pixel whose window lies inside the fine frame, i.e. at least ceil(margin / rate) from the border.  (With the oracle alone:
   3.2e-7 and 6.3e-7, no pixel over; the project's device-to-oracle figure for whole frames is 2.4e-6.)  Then the device's variance on
   those pixels is tests/sample_variance_model.py's on the device's fine frame and on the oracle's, within REL_TOL = 1e-4, the project's
   model tolerance with rel_err's floor.  Border pixels: filter width 1 on the coarse frame has no margin, every pixel is interior.  All
   of it again under the albedo of render_aov_albedo with albedo_floor 0.05.  A third scene has a window of 81 samples: the kernel's
   second path (the samples read twice).
2. It leaves rendering alone: on tests/test_gpu_aov.py's reproducible frame (one light, no bounces) the framebuffer and the ray counts
   are fjgpu_render_tiles's to the bit; pixels of tiles not listed keep what the variance buffer held; whole frame, tile by tile and
   batch_tiles 1 give the same variance to the bit.
3. A jittered frame of one constant-shader object before an empty background: V <= 1e-12 where every window sample hits it (coverage 1,
   eroded by the margin), V > 0 on the silhouette, finite everywhere.
4. The refusals on a live scene.
5. The pipeline: render_denoised(variance_guided=True, variance="samples") stage by stage against the numpy models on the buffers the
   device kept, its error against the spatial estimate's, "spatial" bit-identical to the call without the argument, and
   TemporalDenoiser(variance="samples") over the six-frame pan of tests/test_gpu_temporal.py.
"""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import denoise_variance_model as dvm
import oracle_ffi
import sample_variance_model as svm
from fujiyama_renderer_amd import ffi, gpu, host, synth, workloads
from fujiyama_renderer_amd.fujiyama import SceneInterface

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4
PREMISE_TOL = 1e-5
FLOOR = 0.05


@pytest.fixture(autouse=True)
def the_entry_point():
    """every test here is about fjgpu_render_tiles_variance: without it none has a subject"""
    return gpu.lib().fjgpu_render_tiles_variance


def prepare(text):
    host.run_scene_text(text, deferred=True)
    return host.get_desc()


def check(got, ref, what, tol=REL_TOL):
    err = dm.rel_err(got, ref)
    print("sample variance %-62s max rel err %.3e, %d of %d over" % (what, float(err.max()), int((err > tol).sum()), err.size))
    assert np.isfinite(got).all()
    assert float(err.max()) <= tol, (what, float(err.max()))


def fine_desc(rd):
    """the frame whose pixels are rd's unjittered samples"""
    f = rd.copy()
    f.xres, f.yres = rd.xres * rd.rate_x, rd.yres * rd.rate_y
    f.region[:] = (rd.region[0] * rd.rate_x, rd.region[1] * rd.rate_y, rd.region[2] * rd.rate_x, rd.region[3] * rd.rate_y)
    f.rate_x = f.rate_y = 1
    f.filter_w = f.filter_h = 1.0
    return f


# ---------------------------------------------------------------- 1. against the per-sample radiances
CASES = {
    "teapot_32x32_2x2": dict(res=(32, 32), spp=(2, 2)),                                          # window 4 x 4
    "teapot_40x24_3x3": dict(res=(40, 24), spp=(3, 3)),                                          # window 7 x 7: most of a wave
    "teapot_24x16_3x3_filter3": dict(res=(24, 16), spp=(3, 3), extra=(("filterwidth", (3, 3)),)),   # window 9 x 9 = 81 > 64: read twice
}


@pytest.fixture(scope="module", params=sorted(CASES))
def fine(request, asset_dir):
    """one scene: the coarse frame with its variance (plain and under the albedo), with filter width 1 likewise, and the fine frame from
    the device and from the oracle"""
    kw = CASES[request.param]
    sp, rd = prepare(workloads.teapot(asset_dir, mesh="tiny", **kw))
    rd.jitter = 0
    assert tuple(rd.region) == (0, 0) + kw["res"] and (rd.rate_x, rd.rate_y) == kw["spp"]
    gs = gpu.Scene(sp)
    osc = oracle_ffi.OracleScene(sp)
    try:
        albedo = gs.render_aov_albedo(rd, want=("albedo",))[0]["albedo"]
        out = dict(name=request.param, rd=rd, albedo=albedo)
        out["fb"], out["var"], out["st"] = gs.render_frame_variance(rd)
        out["fb_a"], out["var_a"], _ = gs.render_frame_variance(rd, albedo=albedo, albedo_floor=FLOOR)
        rd1 = rd.copy()
        rd1.filter_w = rd1.filter_h = 1.0
        out["fb1"], out["var1"], _ = gs.render_frame_variance(rd1)
        _, out["var1_a"], _ = gs.render_frame_variance(rd1, albedo=albedo, albedo_floor=FLOOR)
        fd = fine_desc(rd)
        out["fine_device"], _ = gs.render_frame(fd)
        out["fine_oracle"], _ = osc.render(fd)
    finally:
        osc.close()
        gs.close()
    return out


def _model(fine, which, filt=None, albedo=False):
    rd = fine["rd"]
    filt = (float(rd.filter_w), float(rd.filter_h)) if filt is None else filt
    return svm.from_fine_frame(fine["fine_" + which], (rd.xres, rd.yres), (rd.rate_x, rd.rate_y), filt,
                               fine["albedo"] if albedo else None, FLOOR)


@pytest.mark.parametrize("which", ["device", "oracle"])
def test_premise_the_fine_frame_holds_the_samples(fine, which):
    rd = fine["rd"]
    _, beauty, inside = _model(fine, which)
    mx, my = svm.sampler_margin(rd.rate_x, rd.filter_w), svm.sampler_margin(rd.rate_y, rd.filter_h)
    assert inside.sum() == (rd.xres - 2 * -(-mx // rd.rate_x)) * (rd.yres - 2 * -(-my // rd.rate_y)) > 0 and mx > 0
    check(fine["fb"][inside], beauty[inside], "%s: beauty rebuilt from the %s's fine frame" % (fine["name"], which), PREMISE_TOL)
    _, beauty1, inside1 = _model(fine, which, (1.0, 1.0))
    assert inside1.all()
    check(fine["fb1"], beauty1, "%s: the same at filter width 1, every pixel" % fine["name"], PREMISE_TOL)
    # an albedo changes the variance only (two renders of this frame, 32 lights, differ in last bits: tests/test_gpu_parity.py allows 1e-6)
    check(fine["fb_a"], fine["fb"], "%s: the frame of the albedo call" % fine["name"], 1e-6)


@pytest.mark.parametrize("albedo", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("which", ["device", "oracle"])
def test_variance_equals_the_model_on_the_samples(fine, which, albedo):
    V, _, inside = _model(fine, which, albedo=albedo)
    got = fine["var_a" if albedo else "var"]
    assert np.isfinite(got).all() and (got >= 0).all() and (got[inside] > 0).any()
    check(got[inside], V[inside], "%s %s: interior against the %s's samples" % (fine["name"], "albedo" if albedo else "plain", which))
    n = fine["rd"].rate_x * fine["rd"].rate_y
    print("    V in [%.3e, %.3e], %d of %d interior pixels above 1e-3 / %d" % (float(got.min()), float(got.max()), int((V[inside] > 1e-3 / n).sum()),
                                                                           int(inside.sum()), n))


@pytest.mark.parametrize("albedo", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("which", ["device", "oracle"])
def test_border_pixels_at_filter_width_one(fine, which, albedo):
    V, _, inside = _model(fine, which, (1.0, 1.0), albedo=albedo)
    assert inside.all()
    check(fine["var1_a" if albedo else "var1"], V, "%s %s: filter width 1, every pixel, the %s's samples" % (fine["name"], "albedo" if albedo else "plain", which))


def test_the_albedo_matters_and_the_stats_are_the_beauty_passs(fine):
    assert not np.array_equal(fine["var"], fine["var_a"])
    st = fine["st"]
    rd = fine["rd"]
    mx, my = svm.sampler_margin(rd.rate_x, rd.filter_w), svm.sampler_margin(rd.rate_y, rd.filter_h)
    assert st.batches >= 1 and st.resolve_ms > 0 and st.rays.camera >= (rd.xres * rd.rate_x + 2 * mx) * (rd.yres * rd.rate_y + 2 * my)


# ---------------------------------------------------------------- 2. it leaves rendering alone
RAGGED = dict(res=(40, 24), spp=(3, 2), mesh="tiny", nlights=1,
              extra=(("tilesize", (16, 16)), ("filterwidth", (2, 2)), ("sample_jitter", (1,)), ("max_reflect_depth", (0,)),
                     ("max_refract_depth", (0,))))
SENTINEL = -7.5


def device_call(gs, rd, tile_ids, prefill=SENTINEL, albedo=None, fb=None, var=None):
    """Scene.render_tiles(variance=...) into prefilled device tensors -> (framebuffer, variance, stats) as numpy"""
    import torch
    dev = torch.device("cuda", 0)
    fb = torch.full((rd.yres, rd.xres, 4), prefill, dtype=torch.float32, device=dev) if fb is None else fb
    var = torch.full((rd.yres, rd.xres), prefill, dtype=torch.float32, device=dev) if var is None else var
    a = None if albedo is None else torch.from_numpy(albedo).to(dev)
    torch.cuda.synchronize(dev)
    st = gs.render_tiles(rd, tile_ids, fb.data_ptr(), variance=var.data_ptr(), albedo=None if a is None else a.data_ptr(), albedo_floor=FLOOR)
    return fb.cpu().numpy(), var.cpu().numpy(), st


@pytest.fixture(scope="module")
def ragged(asset_dir):
    sp, rd = prepare(workloads.buddhas(asset_dir, **RAGGED))
    gs = gpu.Scene(sp)
    fb0, st0 = gs.render_frame(rd)
    fb, var, st = gs.render_frame_variance(rd)
    yield dict(gs=gs, rd=rd, fb0=fb0, st0=st0, fb=fb, var=var, st=st)
    gs.close()


def test_framebuffer_and_ray_counts_are_render_tiles(ragged):
    gs, rd = ragged["gs"], ragged["rd"]
    assert gpu.tile_count(rd) == 6 and svm.sampler_margin(rd.rate_x, rd.filter_w) > 0 and rd.jitter > 0
    fb1, st1 = gs.render_frame(rd)
    assert ragged["fb0"].any() and np.array_equal(ragged["fb0"], fb1)            # (the premise: the frame is reproducible)
    assert np.array_equal(ragged["fb"], ragged["fb0"])
    assert ragged["st"].rays.as_dict() == ragged["st0"].rays.as_dict() == st1.rays.as_dict() and ragged["st"].rays.shadow > 0
    assert ragged["st"].batches == ragged["st0"].batches and ragged["st"].trace_launches == ragged["st0"].trace_launches
    assert np.isfinite(ragged["var"]).all() and (ragged["var"] >= 0).all() and (ragged["var"] > 0).any()


def test_pixels_of_tiles_not_listed_are_untouched(ragged):
    gs, rd = ragged["gs"], ragged["rd"]
    subset = list(range(gpu.tile_count(rd)))[::-1][::2]
    assert 1 < len(subset) < gpu.tile_count(rd)
    fb, var, st = device_call(gs, rd, subset)
    touched = np.zeros((rd.yres, rd.xres), dtype=bool)
    for t in subset:
        x0, y0, x1, y1 = gpu.tile_rect(rd, t)
        touched[y0:y1, x0:x1] = True
    assert touched.any() and not touched.all()
    assert (var[~touched] == np.float32(SENTINEL)).all() and (fb[~touched] == np.float32(SENTINEL)).all()
    assert np.array_equal(var[touched], ragged["var"][touched]) and np.array_equal(fb[touched], ragged["fb"][touched])


def test_ragged_region(asset_dir):
    """a render region not aligned to the tiles: outside it nothing is written, inside it the whole-frame values of the same region"""
    kw = dict(RAGGED)
    kw["extra"] = RAGGED["extra"] + (("render_region", (3, 2, 37, 23)),)
    sp, rd = prepare(workloads.buddhas(asset_dir, **kw))
    gs = gpu.Scene(sp)
    try:
        fb, var, st = device_call(gs, rd, None)
        fb_t, var_t = None, None
        import torch
        dev = torch.device("cuda", 0)
        fbt = torch.full((rd.yres, rd.xres, 4), SENTINEL, dtype=torch.float32, device=dev)
        vt = torch.full((rd.yres, rd.xres), SENTINEL, dtype=torch.float32, device=dev)
        for t in range(gpu.tile_count(rd)):
            fb_t, var_t, _ = device_call(gs, rd, [t], fb=fbt, var=vt)
    finally:
        gs.close()
    inside = np.zeros((rd.yres, rd.xres), dtype=bool)
    inside[2:23, 3:37] = True
    assert (var[~inside] == np.float32(SENTINEL)).all() and (fb[~inside] == np.float32(SENTINEL)).all()
    assert np.isfinite(var[inside]).all() and (var[inside] >= 0).all() and (var[inside] > 0).any()
    assert np.array_equal(var, var_t) and np.array_equal(fb, fb_t)


def test_whole_frame_tile_by_tile_and_batches_of_one_tile_agree(ragged):
    import torch
    gs, rd = ragged["gs"], ragged["rd"]
    dev = torch.device("cuda", 0)
    fbt = torch.full((rd.yres, rd.xres, 4), SENTINEL, dtype=torch.float32, device=dev)
    vt = torch.full((rd.yres, rd.xres), SENTINEL, dtype=torch.float32, device=dev)
    for t in range(gpu.tile_count(rd)):
        fb, var, st = device_call(gs, rd, [t], fb=fbt, var=vt)
        assert st.batches == 1
    assert np.array_equal(var, ragged["var"]) and np.array_equal(fb, ragged["fb"])
    gs.set_option("batch_tiles", 1)
    try:
        fb, var, st = gs.render_frame_variance(rd)
    finally:
        gs.set_option("batch_tiles", 0)
    assert st.batches == gpu.tile_count(rd)
    assert np.array_equal(var, ragged["var"]) and np.array_equal(fb, ragged["fb"])
    # ... and the plain entry goes on as before
    fb2, st2 = gs.render_frame(rd)
    assert np.array_equal(fb2, ragged["fb0"]) and st2.rays.as_dict() == ragged["st0"].rays.as_dict()


# ---------------------------------------------------------------- 3. a jittered frame
def constant_object(asset_dir, res=(48, 40), spp=(3, 3)):
    """the tiny mesh with a constant shader and nothing else: no floor, no dome, no light"""
    a = synth.ensure_assets(asset_dir, ("tiny",))
    si = SceneInterface(parse_args=False)
    si.OpenPlugin("constant_shader", "ConstantShader")
    si.OpenPlugin("stanfordply_procedure", "StanfordPlyProcedure")
    si.NewCamera("cam1", "PerspectiveCamera")
    si.SetProperty3("cam1", "translate", 0, 1, 6)
    si.SetProperty1("cam1", "fov", 30)
    si.NewShader("obj_shader", "constant_shader")
    si.SetProperty3("obj_shader", "diffuse", .7, .4, .2)
    workloads._ply(si, "obj_mesh", a["tiny"])
    si.NewObjectInstance("obj1", "obj_mesh")
    si.SetProperty3("obj1", "rotate", 10, 25, -5)
    si.AssignShader("obj1", "DEFAULT_SHADING_GROUP", "obj_shader")
    workloads._renderer(si, res, spp, (("filterwidth", (2, 2)),))
    return si.text()


def test_constant_object_under_jitter(asset_dir):
    sp, rd = prepare(constant_object(asset_dir))
    assert rd.jitter > 0
    gs = gpu.Scene(sp)
    try:
        cov = gs.render_aov(rd, want=("coverage",))[0]["coverage"][..., 0]
        fb, var, _ = gs.render_frame_variance(rd)
    finally:
        gs.close()
    assert np.isfinite(var).all() and (var >= 0).all()
    # every window sample is an own sample of a pixel at most ceil(margin / rate) away
    e = max(-(-svm.sampler_margin(rd.rate_x, rd.filter_w) // rd.rate_x), -(-svm.sampler_margin(rd.rate_y, rd.filter_h) // rd.rate_y))
    assert e >= 1
    full = cov == 1
    solid = full.copy()
    H, W = full.shape
    for dy in range(-e, e + 1):
        for dx in range(-e, e + 1):
            shifted = np.zeros_like(full)
            shifted[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] = full[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
            solid &= shifted
    edge = (cov > 0) & (cov < 1)
    l = float(dvm.luminance(fb[solid][0:1, :3])[0])
    print("constant object: %d solid pixels (V max %.3e, luminance %.4f), %d silhouette pixels (V min %.3e)" % (
        int(solid.sum()), float(var[solid].max()), l, int(edge.sum()), float(var[edge].min())))
    assert solid.sum() > 50 and edge.sum() > 20 and l > 0.1
    assert (var[solid] <= 1e-12).all()
    assert (var[edge] > 0).all()


# ---------------------------------------------------------------- 4. refusals on a live scene
def test_refusals_on_a_live_scene(asset_dir):
    import torch
    dev = torch.device("cuda", 0)
    sp, rd = prepare(workloads.buddhas(asset_dir, res=(16, 12), spp=(2, 2), mesh="tiny", nlights=1))
    gs = gpu.Scene(sp)
    L = gpu.lib()
    fb = torch.zeros((12, 16, 4), dtype=torch.float32, device=dev)
    var = torch.zeros((12, 16), dtype=torch.float32, device=dev)
    alb = torch.full((12, 16, 3), 0.5, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    st = ffi.GpuStats()

    def call(render, d_fb, d_albedo, floor, d_var):
        rc = L.fjgpu_render_tiles_variance(gs._h, C.byref(render), None, 0, d_fb, d_albedo, floor, d_var, None, C.byref(st))
        return rc, L.fjgpu_last_error().decode()

    try:
        adaptive = rd.copy()
        adaptive.sampler_type = 1
        rc, msg = call(adaptive, fb.data_ptr(), None, 0.0, var.data_ptr())
        assert rc == -3 and msg.startswith("fjgpu_render_tiles_variance:") and "adaptive sampler" in msg, (rc, msg)
        for what, args in (("null", (fb.data_ptr(), None, 0.0, None)), ("null", (None, None, 0.0, var.data_ptr())),
                           ("overlap", (fb.data_ptr(), None, 0.0, fb.data_ptr())),
                           ("overlap", (fb.data_ptr(), None, 0.0, fb.data_ptr() + 16 * 12 * 4 * 4 - 4)),
                           ("overlap", (fb.data_ptr(), alb.data_ptr(), FLOOR, alb.data_ptr())),
                           ("albedo_floor", (fb.data_ptr(), alb.data_ptr(), 0.0, var.data_ptr())),
                           ("albedo_floor", (fb.data_ptr(), alb.data_ptr(), -1.0, var.data_ptr())),
                           ("albedo_floor", (fb.data_ptr(), alb.data_ptr(), float("nan"), var.data_ptr())),
                           ("albedo_floor", (fb.data_ptr(), alb.data_ptr(), float("inf"), var.data_ptr()))):
            rc, msg = call(rd, *args)
            assert rc == -2 and msg.startswith("fjgpu_render_tiles_variance:") and what in msg, (what, rc, msg)
        assert not fb.any() and not var.any()                        # (nothing was rendered)
        with pytest.raises(gpu.GpuError, match="fjgpu_render_tiles_variance: .*adaptive sampler"):
            gs.render_frame_variance(adaptive)
        # a floor without an albedo is not looked at, and the scene renders as ever
        rc, msg = call(rd, fb.data_ptr(), None, float("nan"), var.data_ptr())
        assert rc == 0, (rc, msg)
        ref, _ = gs.render_frame(rd)
        got, v, _ = gs.render_frame_variance(rd, albedo=alb, albedo_floor=FLOOR)
    finally:
        gs.close()
    check(fb.cpu().numpy(), ref, "after the refusals: the frame")
    check(got, ref, "after the refusals: the frame of the albedo call")
    assert np.isfinite(v).all() and (v > 0).any()
    check(v, var.cpu().numpy() / np.float32(0.25), "a uniform albedo of 0.5: four times the plain variance")


# ---------------------------------------------------------------- 5. the pipeline
CORNELL = dict(res=(64, 48), mesh="tiny")


@pytest.fixture(scope="module")
def cornell(asset_dir):
    """the Cornell box at 4 x 4 spp through Scene.render_denoised: plain filter, variance-guided with the spatial estimate and with the
    sample variance (inputs kept; also demodulated), and the device's 12 x 12 spp frame as truth"""
    sp, rd = prepare(workloads.cornell(asset_dir, spp=(12, 12), **CORNELL))
    gs = gpu.Scene(sp)
    truth, _ = gs.render_frame(rd)
    gs.close()
    sp, rd = prepare(workloads.cornell(asset_dir, spp=(4, 4), **CORNELL))
    gs = gpu.Scene(sp)
    try:
        out = dict(truth=truth, rd=rd)
        out["plain"], _ = gs.render_denoised(rd)
        out["spatial"], _ = gs.render_denoised(rd, variance_guided=True, variance="spatial")
        out["samples"], out["info"] = gs.render_denoised(rd, variance_guided=True, keep_inputs=True, variance="samples")
        out["dem"], out["info_dem"] = gs.render_denoised(rd, variance_guided=True, keep_inputs=True, variance="samples", demodulate=True)
        _, out["var"], _ = gs.render_frame_variance(rd)
        _, out["var_dem"], _ = gs.render_frame_variance(rd, albedo=out["info_dem"]["aov"]["albedo"])
        with pytest.raises(ValueError):
            gs.render_denoised(rd, variance="samples")
        with pytest.raises(ValueError):
            gs.render_denoised(rd, variance_guided=True, variance="temporal")
    finally:
        gs.close()
    return out


@pytest.mark.parametrize("demodulate", [False, True], ids=["plain", "demodulated"])
def test_render_denoised_samples_equals_the_models_on_its_own_inputs(cornell, demodulate):
    info = cornell["info_dem" if demodulate else "info"]
    aov = info["aov"]
    assert sorted(aov) == (["albedo"] if demodulate else []) + ["ids", "normal", "position"]
    assert info["beauty_stats"].rays.camera == info["aov_stats"].rays.camera > 0 and info["sigma_luminance"] == gpu.SIGMA_LUMINANCE
    vin = info["variance_in"]
    assert vin.shape == (48, 64) and np.isfinite(vin).all() and (vin >= 0).all() and (vin > 0).mean() > 0.5
    # the stage in front: the pass by itself gives this variance (two renders of the frame differ in the last bits of a sample)
    check(vin, cornell["var_dem" if demodulate else "var"], "render_denoised(samples%s): variance_in against the call by itself" % (", demodulate" if demodulate else ""))
    kw = dict(albedo=aov["albedo"], albedo_floor=info["albedo_floor"]) if demodulate else {}
    ref, ref_var = dvm.denoise_variance(info["beauty"], aov["normal"], aov["position"], aov["ids"], variance=vin,
                                        iterations=gpu.DENOISE_ITERATIONS, sigma_luminance=gpu.SIGMA_LUMINANCE, sigma_normal=gpu.SIGMA_NORMAL,
                                        sigma_position=info["sigma_position"], stop_at_ids=True, **kw)
    check(cornell["dem" if demodulate else "samples"], ref, "render_denoised(samples%s): colour" % (", demodulate" if demodulate else ""))
    check(info["variance"], ref_var, "render_denoised(samples%s): variance of the last iteration" % (", demodulate" if demodulate else ""))
    assert info["denoise_stats"].batches == gpu.DENOISE_ITERATIONS


def test_sample_variance_beats_the_spatial_estimate(cornell):
    """mean squared error against the 12 x 12 spp frame at the shipped sigmas.  CPU figures (oracle and numpy models, jitter 0, the
    uncorrected V): 0.0152 with the sample variance against 0.0216 with the spatial estimate, plain filter 0.0110, noisy 0.0324.
    Measured on an MI355X (profiles/sample_variance.txt): 0.015983 against 0.024018, plain filter 0.011183, noisy 0.029860"""
    truth = cornell["truth"].astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))
    noisy, plain, spatial, samples = mse(cornell["info"]["beauty"]), mse(cornell["plain"]), mse(cornell["spatial"]), mse(cornell["samples"])
    print("Cornell 64x48 at 4x4 spp, MSE against 12x12 spp: noisy %.6f, plain filter %.6f, variance-guided with the spatial estimate %.6f, "
          "with the sample variance %.6f" % (noisy, plain, spatial, samples))
    assert samples < spatial


def test_spatial_is_the_call_without_the_argument(ragged):
    """bit for bit, on the frame whose beauty render is reproducible to the bit (the path-traced Cornell box is not: the atomic adds of a
    sample's terms arrive in any order, tests/test_gpu_temporal.py) -- that premise is checked first"""
    gs, rd = ragged["gs"], ragged["rd"]
    for demodulate in (False, True):
        a, ia = gs.render_denoised(rd, variance_guided=True, keep_inputs=True, demodulate=demodulate)
        b, ib = gs.render_denoised(rd, variance_guided=True, keep_inputs=True, demodulate=demodulate, variance="spatial")
        assert np.array_equal(ia["beauty"], ragged["fb0"]) and np.array_equal(ib["beauty"], ragged["fb0"])          # (the premise)
        assert "variance_in" not in ia and "variance_in" not in ib and sorted(ia["aov"]) == sorted(ib["aov"])
        for name in ia["aov"]:
            assert np.array_equal(ia["aov"][name], ib["aov"][name], equal_nan=True), name
        assert np.array_equal(a, b) and np.array_equal(ia["variance"], ib["variance"]) and not np.array_equal(a, ragged["fb0"])
        # ... and the other source is another filter input on the same frame
        c, ic = gs.render_denoised(rd, variance_guided=True, keep_inputs=True, demodulate=demodulate, variance="samples")
        assert np.array_equal(ic["beauty"], ragged["fb0"]) and not np.array_equal(c, a)
        if not demodulate:
            assert np.array_equal(ic["variance_in"], ragged["var"])


PAN_STEP = 0.012                   # tests/test_gpu_temporal.py's pan
CORNELL_CAM = "SetSampleProperty3 cam1 translate 0 0.5 1.85 0"


def test_temporal_denoiser_with_the_sample_variance(asset_dir):
    text = workloads.cornell(asset_dir, spp=(2, 2), **CORNELL)
    assert text.count(CORNELL_CAM) == 1
    sp, rd = prepare(text)
    gs = gpu.Scene(sp)
    try:
        runs = {}
        for mode in ("spatial", "samples"):
            td = gpu.TemporalDenoiser(gs, rd, variance=mode) if mode == "samples" else gpu.TemporalDenoiser(gs, rd)
            runs[mode] = [td.render(camera=dict(translate=(k * PAN_STEP, 0.5, 1.85)), keep_inputs=True) for k in range(6)]
        with pytest.raises(ValueError):
            gpu.TemporalDenoiser(gs, rd, variance="none")
    finally:
        gs.close()
    for k in range(6):
        (out0, info0), (out1, info1) = runs["spatial"][k], runs["samples"][k]
        assert np.array_equal(info0["history_length"], info1["history_length"]) and info1["frame"] == k
        assert info0["estimate_stats"] is not None and info1["estimate_stats"] is None
        vs = info1["variance_spatial"]
        assert np.isfinite(vs).all() and (vs >= 0).all() and (vs > 0).any() and not np.array_equal(vs, info0["variance_spatial"])
        assert np.isfinite(out1).all() and np.isfinite(info1["variance"]).all() and (info1["variance"] >= 0).all()
        for name in ("position", "normal", "ids", "albedo"):
            assert np.array_equal(info0["aov"][name], info1["aov"][name])
    fg = runs["samples"][-1][1]["aov"]["ids"][..., 0] >= 0
    share = float((runs["samples"][-1][1]["history_length"][fg] >= 2).mean())
    print("Cornell 64x48 pan with the sample variance: history >= 2 on %.3f of the foreground" % share)
    assert share >= 0.9
