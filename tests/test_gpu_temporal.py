"""GPU suite (-m gpu): fjgpu_denoise_temporal, fjgpu_denoise_estimate_variance_albedo, the camera of a resident scene and the view of a
frame (include/fjgpu.h) on the device.

The accumulation runs against the numpy restatement tests/temporal_model.py on the analytic scene of tests/temporal_scene.py (37 x 29 with
region (3, 2, 34, 27): more than one 16 x 16 block each way, both ragged), the cases and the tolerance of tests/test_temporal_cpu.py:
REL_TOL = 1e-4 with denoise_model.rel_err, the history length exact.  set_camera is held against a scene freshly created with that camera,
bit for bit wherever two renders of one scene are.  The pipeline test is the feature's claim: on a six-frame sub-pixel pan of the Cornell box the temporally accumulated and
filtered frame is nearer a 12 x 12 spp frame than the last frame filtered alone.
"""
import re

import numpy as np
import pytest

import albedo_model as am
import denoise_model as dm
import denoise_variance_model as dvm
import temporal_model as tm
import temporal_scene as ts
from fujiyama_renderer_amd import ffi, gpu, host, workloads

pytestmark = pytest.mark.gpu

W, H, REGION = ts.W, ts.H, ts.REGION


def c_view(v):
    out = ffi.View()
    out.world_to_camera[:] = list(v.world_to_camera)
    out.uv_size[:] = list(v.uv_size)
    out.xres, out.yres = v.xres, v.yres
    return out


def run_device(cur, prev, prev_hist, albedo, vs, out=None, var_out=None, **params):
    import torch
    nxt = None if out is None else {k: torch.from_numpy(v).to("cuda:0") for k, v in out.items()}
    vout = None if var_out is None else torch.from_numpy(var_out).to("cuda:0")
    hist, var, st = gpu.temporal_accumulate(
        cur["color"], cur["position"], cur["normal"], cur["ids"], albedo=cur["albedo"] if albedo else None, variance_spatial=vs,
        prev_view=c_view(prev["view"]) if prev else None, prev_position=prev["position"] if prev else None,
        prev_normal=prev["normal"] if prev else None, prev_ids=prev["ids"] if prev else None, prev=prev_hist, next=nxt, variance_out=vout,
        region=REGION, **params)
    assert st.batches == 1 and st.total_ms > 0 and st.resolve_ms == st.total_ms
    return hist, var


@pytest.mark.parametrize("albedo", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("spatial", [False, True], ids=["moments", "spatial"])
def test_device_equals_model(albedo, spatial):
    ts.check_equal_to_model(run_device, albedo, spatial, "device %s %s" % ("albedo" if albedo else "plain", "spatial" if spatial else "moments"))


def test_pixels_outside_the_region_are_untouched():
    ts.check_untouched_and_unread(run_device)


def test_large_move_resets():
    """a move of eight pixels at the sphere's distance, where disoccluded, background and surviving pixels all occur (the resets of
    tests/test_temporal_cpu.py), against the model: pixels without history carry length 1 and the current colour bit for bit"""
    f0 = ts.frame(noise=0.1, seed=1)
    f1 = ts.frame(dx=8 * ts.PIXEL_AT_SPHERE, noise=0.1, seed=2)
    h0, _ = run_device(f0, None, None, True, None, **ts.PARAMS)
    got, var = run_device(f1, f0, h0, True, None, **ts.PARAMS)
    ref, rvar = ts.model_run(f1, f0, h0, True, None, **ts.PARAMS)
    assert np.array_equal(got["length"], ref["length"])
    assert float(tm.rel_err(got["color"], ref["color"]).max()) <= ts.REL_TOL and float(tm.rel_err(var, rvar).max()) <= ts.REL_TOL
    m = ts.inside()
    reset = m & (got["length"] == 1)
    assert (m & (f1["ids"][..., 0] == 0) & reset).sum() >= 5 and (m & (got["length"] > 1)).sum() > 300
    assert np.array_equal(got["color"][reset], f1["color"][reset])


def test_device_tensors_stay_on_the_device_and_ping_pong():
    """to_host=False returns the tensors the call wrote; feeding them back as prev and the older pair as next gives the bits of separate buffers"""
    import torch
    frames = ts.pan_sequence(3)
    kw = dict(region=REGION, **ts.PARAMS)
    host_hist = None
    dev_hist, spare = None, None
    for k, f in enumerate(frames):
        p = frames[k - 1] if k else None
        args = dict(prev_view=c_view(p["view"]) if p else None, prev_position=p["position"] if p else None, prev_normal=p["normal"] if p else None,
                    prev_ids=p["ids"] if p else None)
        host_hist, host_var, _ = gpu.temporal_accumulate(f["color"], f["position"], f["normal"], f["ids"], prev=host_hist, **args, **kw)
        new, var, _ = gpu.temporal_accumulate(f["color"], f["position"], f["normal"], f["ids"], prev=dev_hist, next=spare, to_host=False, **args, **kw)
        assert all(torch.is_tensor(t) and t.is_cuda for t in new.values()) and var.is_cuda
        dev_hist, spare = new, dev_hist
        for name in gpu.HISTORY_NAMES:
            assert np.array_equal(new[name].cpu().numpy()[ts.inside()], host_hist[name][ts.inside()])
        assert np.array_equal(var.cpu().numpy(), host_var)
    with pytest.raises(gpu.GpuError, match="fjgpu_denoise_temporal: an output buffer"):
        f, p = frames[2], frames[1]
        gpu.temporal_accumulate(f["color"], f["position"], f["normal"], f["ids"], prev=dev_hist, next=dev_hist, prev_view=c_view(p["view"]),
                                prev_position=p["position"], prev_normal=p["normal"], prev_ids=p["ids"], **kw)


def test_estimate_variance_albedo_equals_model():
    f = ts.pan_sequence(1)[0]
    kw = dict(sigma_normal=0.8, sigma_position=1.2)
    got, st = gpu.estimate_variance_albedo(f["color"], f["albedo"], f["normal"], f["position"], f["ids"], albedo_floor=0.05, region=REGION, **kw)
    D, _ = am.demodulate(f["color"], f["albedo"], 0.05, REGION)
    ref = dvm.estimate_variance(D, f["normal"], f["position"], f["ids"], region=REGION, **kw)
    err = float(dm.rel_err(got, ref).max())
    print("estimate_variance_albedo: max rel err %.3e" % err)
    assert err <= 1e-4 and st.gen_ms > 0 and (got[~ts.inside()] == 0).all() and got[ts.inside()].max() > 0
    plain, _ = gpu.estimate_variance(f["color"], f["normal"], f["position"], f["ids"], region=REGION, **kw)
    assert not np.array_equal(plain, got)


# ---- the camera of a resident scene

TEAPOT_CAM = "SetProperty3 cam1 translate 0 1 7"
CORNELL_CAM = "SetSampleProperty3 cam1 translate 0 0.5 1.85 0"


REPRODUCIBLE = (("max_reflect_depth", (0,)), ("max_refract_depth", (0,)))


def _teapot(asset_dir, translate=None, rotate=None, one_light=False):
    kw = dict(nlights=1, extra=REPRODUCIBLE) if one_light else {}
    text = workloads.teapot(asset_dir, res=(32, 32), spp=(1, 1), mesh="tiny", **kw)
    assert text.count(TEAPOT_CAM) == 1
    if translate is not None:
        text = text.replace(TEAPOT_CAM, "SetProperty3 cam1 translate %r %r %r" % tuple(translate))
    if rotate is not None:
        text, n = re.subn(r"SetProperty3 cam1 rotate \S+ 0 0", "SetProperty3 cam1 rotate %r %r %r" % tuple(rotate), text)
        assert n == 1
    return text


def _cornell(asset_dir, spp=(2, 2), translate=None):
    text = workloads.cornell(asset_dir, res=(64, 48), spp=spp, mesh="tiny")
    assert text.count(CORNELL_CAM) == 1
    if translate is not None:
        text = text.replace(CORNELL_CAM, "SetSampleProperty3 cam1 translate %r %r %r 0" % tuple(translate))
    return text


def _everything(gs, rd):
    fb, st = gs.render_frame(rd)
    aov, st_aov = gs.render_aov(rd)
    rays = gs.camera_samples(rd, 0)
    return fb, st.rays.as_dict(), aov, st_aov.rays.as_dict(), rays


def _same(a, b, reproducible, what):
    """ray counts, AOVs and camera samples bit for bit; the beauty frame bit for bit where two renders of ONE scene are, else as near as those"""
    assert a[1] == b[1] and a[3] == b[3] and np.array_equal(a[4], b[4])
    for name in a[2]:
        assert np.array_equal(a[2][name], b[2][name], equal_nan=True), name
    err = float(dm.rel_err(a[0], b[0]).max())
    print("set_camera %-28s %d of %d beauty values differ, max rel err %.3e (reproducible frame: %s)"
          % (what, int((a[0] != b[0]).sum()), a[0].size, err, reproducible))
    assert np.array_equal(a[0], b[0]) if reproducible else err <= 1e-6


@pytest.mark.parametrize("scene", ["teapot", "teapot_one_light", "cornell"])
def test_set_camera_is_a_fresh_scene_with_that_camera(scene, asset_dir):
    """scene X created with camera A and moved to B gives the bits and the ray counts of scene Y created with B -- beauty frame, AOVs, camera
    samples --, and moved back to A its own first frame.
    The beauty frames of the teapot with its 32 lights and of the path-traced Cornell box are not reproducible to the bit even between two
    renders of one untouched scene: the atomic adds of a pixel's terms arrive in any order (tests/test_gpu_aov.py:
    test_does_not_disturb_rendering; tests/test_gpu_parity.py: render_both allows 1e-6 relative for it).  Measured on an MI355X: 160 to 213
    of the teapot's 4096 values and 0 to 4 of the Cornell box's 12288 differ between two such renders, by at most 2.3e-7 relative.  So
    bit identity of the beauty frame is asked where it exists -- "teapot_one_light", the reproducible recipe of tests/test_gpu_aov.py (one
    light, no bounces: at most two terms per sample), whose premise is checked first -- and render_both's 1e-6 for the two others.  Ray
    counts, AOVs and camera samples are bit-identical in every case."""
    if scene.startswith("teapot"):
        make = lambda d, **kw: _teapot(d, one_light=scene == "teapot_one_light", **kw)
        move = dict(translate=(0.75, 1.25, 6.5), rotate=(-8.0, 6.0, 0.0))
    else:
        make, move = _cornell, dict(translate=(0.0625, 0.5, 1.85))
    host.run_scene_text(make(asset_dir), deferred=True)
    sp, rd = host.get_desc()
    X = gpu.Scene(sp)
    try:
        cam_a = X.get_camera()
        a = _everything(X, rd)
        cam_b = X.set_camera(**move)
        assert tuple(X.get_camera().xform.translate[0].v) == tuple(float(v) for v in move["translate"])
        moved = _everything(X, rd)
        reproducible = scene == "teapot_one_light"
        if reproducible:
            assert np.array_equal(X.render_frame(rd)[0], moved[0])          # (the premise)
        host.run_scene_text(make(asset_dir, **move), deferred=True)
        sp_b, rd_b = host.get_desc()
        Y = gpu.Scene(sp_b)
        try:
            fresh = _everything(Y, rd_b)
            cam_y = Y.get_camera()
            view_y = Y.view(rd_b)
        finally:
            Y.close()
        assert bytes(cam_y) == bytes(cam_b) and bytes(view_y) == bytes(X.view(rd))
        _same(moved, fresh, reproducible, scene + ", moved against fresh")
        assert float(dm.rel_err(moved[0], a[0]).max()) > 1e-2
        X.set_camera(cam_a)
        _same(_everything(X, rd), a, reproducible, scene + ", moved back")
    finally:
        X.close()


def test_set_camera_refuses_time_sampled_cameras(asset_dir):
    host.run_scene_text(_teapot(asset_dir), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    try:
        cam = gs.get_camera()
        cam.xform.n_translate = 2
        cam.xform.translate[1].v[:] = (1.0, 1.0, 7.0)
        cam.xform.translate[1].time = 1.0
        with pytest.raises(gpu.GpuError, match=r"error -3: fjgpu_scene_set_camera: a time-sampled camera"):
            gs.set_camera(cam)
        cam.xform.n_translate = 9
        with pytest.raises(gpu.GpuError, match=r"error -2: fjgpu_scene_set_camera: camera transform sample count out of range"):
            gs.set_camera(cam)
        fb, _ = gs.render_frame(rd)
        assert fb.any()
    finally:
        gs.close()
    host.run_scene_text(workloads.motion(asset_dir, res=(32, 24), spp=(1, 1), mesh="tiny", kind="camera"), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    try:
        static = gs.get_camera()
        assert static.xform.n_translate == 2
        static.xform.n_translate = static.xform.n_rotate = 1
        with pytest.raises(gpu.GpuError, match=r"error -3: fjgpu_scene_set_camera: the scene was created with a time-sampled camera"):
            gs.set_camera(static)
        with pytest.raises(gpu.GpuError, match=r"error -3: fjgpu_scene_view: a time-sampled camera"):
            gs.view(rd)
    finally:
        gs.close()


@pytest.mark.parametrize("scene", ["teapot", "cornell"])
def test_view_projects_positions_onto_their_own_pixels(scene, asset_dir):
    """a jitter-0, 1 x 1 spp AOV pass: every foreground pixel's position, projected through Scene.view, lands on the pixel's own centre
    within 1e-3 pixel.  The bound is f32's: a position of magnitude up to ~10 carries 2^-24 * 10 = 6e-7 of rounding, a pixel of these
    frames is about 0.03 to 0.1 world units wide at the nearest surfaces: 2e-5 pixel, grazing surfaces a few times more.  Measured
    on an MI355X: 1.2e-6 pixel on the teapot, 1.5e-6 on the Cornell box."""
    text = _teapot(asset_dir) if scene == "teapot" else _cornell(asset_dir, spp=(1, 1))
    text = text.replace("RenderScene ren1", "SetProperty1 ren1 sample_jitter 0\nRenderScene ren1")
    host.run_scene_text(text, deferred=True)
    sp, rd = host.get_desc()
    assert rd.jitter == 0 and (rd.rate_x, rd.rate_y) == (1, 1)
    gs = gpu.Scene(sp)
    try:
        gs.set_camera(translate=(0.125, float(gs.get_camera().xform.translate[0].v[1]), float(gs.get_camera().xform.translate[0].v[2])))
        aov, _ = gs.render_aov(rd)
        view = gs.view(rd)
    finally:
        gs.close()
    fg = aov["ids"][..., 0] >= 0
    assert fg.sum() > 100
    fx, fy, ok = tm.project(view, aov["position"])
    y, x = np.nonzero(fg)
    assert ok[fg].all()
    err = max(float(np.abs(fx[fg] - x).max()), float(np.abs(fy[fg] - y).max()))
    print("view, %s: %d foreground pixels, max projection error %.3e pixel" % (scene, fg.sum(), err))
    assert err <= 1e-3


# ---- the pipeline

PAN_STEP = 0.012                   # world units per frame: about 0.4 pixel at the box's back wall (scripts/temporal_grid.py)


@pytest.fixture(scope="module")
def pan(asset_dir):
    """six frames of TemporalDenoiser over a sideways pan of the Cornell box at 2 x 2 spp (inputs kept), the last frame alone through
    render_denoised(variance_guided, demodulate) and a 12 x 12 spp frame of the last camera"""
    last = (5 * PAN_STEP, 0.5, 1.85)
    host.run_scene_text(_cornell(asset_dir, spp=(12, 12), translate=last), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    truth, _ = gs.render_frame(rd)
    gs.close()
    host.run_scene_text(_cornell(asset_dir), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    try:
        td = gpu.TemporalDenoiser(gs, rd)
        results = [td.render(camera=dict(translate=(k * PAN_STEP, 0.5, 1.85)), keep_inputs=True) for k in range(6)]
        views = []
        for k in range(6):
            gs.set_camera(translate=(k * PAN_STEP, 0.5, 1.85))
            views.append(gs.view(rd))
        single, _ = gs.render_denoised(rd, variance_guided=True, demodulate=True)
        td.reset()
        again, info_again = td.render(keep_inputs=True)
    finally:
        gs.close()
    return dict(truth=truth, results=results, views=views, single=single, again=again, info_again=info_again, td=td)


def test_pipeline_equals_the_models_on_its_own_inputs(pan):
    """every stage of every frame against the numpy models on the buffers the device kept: the spatial estimate, the accumulation (history
    length exact), the variance-guided filter of the accumulated frame with the temporal variance"""
    hist, prev = None, None
    for k, (out, info) in enumerate(pan["results"]):
        aov = info["aov"]
        assert sorted(aov) == ["albedo", "ids", "normal", "position"] and info["frame"] == k
        assert info["beauty_stats"].rays.camera == info["aov_stats"].rays.camera > 0 and info["temporal_stats"].batches == 1
        D, _ = am.demodulate(info["beauty"], aov["albedo"], gpu.ALBEDO_FLOOR)
        vs = dvm.estimate_variance(D, aov["normal"], aov["position"], aov["ids"], sigma_normal=gpu.SIGMA_NORMAL, sigma_position=info["sigma_position"])
        hist, var = tm.accumulate(info["beauty"], aov["position"], aov["normal"], aov["ids"], albedo=aov["albedo"], variance_spatial=vs,
                                  prev_view=pan["views"][k - 1] if k else None, prev_position=prev["position"] if prev else None,
                                  prev_normal=prev["normal"] if prev else None, prev_ids=prev["ids"] if prev else None, prev=hist,
                                  alpha_min=gpu.ALPHA_MIN, max_history=gpu.MAX_HISTORY, tol_position=info["tol_position"],
                                  cos_normal=gpu.COS_NORMAL, min_history_variance=gpu.MIN_HISTORY_VARIANCE, albedo_floor=gpu.ALBEDO_FLOOR)
        # (the spatial estimate differs by expf's few ulp, and so may the variance where it is taken; which taps were valid does not)
        assert np.array_equal(info["history_length"], hist["length"])
        for name, a, b in (("accumulated", info["accumulated"], hist["color"]), ("variance", info["variance"], var)):
            err = float(dm.rel_err(a, b).max())
            print("pipeline frame %d %-12s max rel err %.3e" % (k, name, err))
            assert err <= 1e-4
        ref, _ = dvm.denoise_variance(info["accumulated"], aov["normal"], aov["position"], aov["ids"], albedo=aov["albedo"],
                                      albedo_floor=gpu.ALBEDO_FLOOR, variance=info["variance"], iterations=gpu.DENOISE_ITERATIONS,
                                      sigma_luminance=gpu.SIGMA_LUMINANCE, sigma_normal=gpu.SIGMA_NORMAL, sigma_position=info["sigma_position"],
                                      stop_at_ids=True)
        err = float(dm.rel_err(out, ref).max())
        print("pipeline frame %d %-12s max rel err %.3e" % (k, "result", err))
        assert err <= 1e-4
        # the history the next frame reads is the device's own
        hist = dict(color=info["accumulated"], moments=hist["moments"], length=info["history_length"])
        prev = aov
    p = pan["results"][0][1]["aov"]["position"][pan["results"][0][1]["aov"]["ids"][..., 0] >= 0].astype(np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    assert pan["results"][-1][1]["tol_position"] == pytest.approx(gpu.TOL_POSITION_FRACTION * diag, rel=1e-6)


def test_pipeline_history_and_error(pan):
    """at the last frame the history is at least 2 frames long on 90 % of the foreground (the numpy model gives the same lengths on the
    same AOVs: test_pipeline_equals_the_models_on_its_own_inputs), and the result is nearer the 12 x 12 spp frame than the last frame
    filtered alone.  Measured on an MI355X (profiles/temporal_pass.txt, section 2): history on 0.992 of the foreground; mean squared error
    196365.97 against 241753.47 -- both figures are the blow-up of the variance-guided filter on this frame's demodulated emitter
    (profiles/denoise_variance.txt), which the comparison the feature was asked to pass inherits; the noisy frame measures 0.128."""
    out, info = pan["results"][-1]
    fg = info["aov"]["ids"][..., 0] >= 0
    share = float((info["history_length"][fg] >= 2).mean())
    truth = pan["truth"].astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))
    temporal, single, noisy = mse(out), mse(pan["single"]), mse(info["beauty"])
    print("Cornell 64x48 pan: history >= 2 on %.3f of %d foreground pixels, longest %.2f" % (share, fg.sum(), float(info["history_length"].max())))
    print("Cornell 64x48 pan: MSE against 12x12 spp: noisy 2x2 %.6f, last frame alone filtered %.6f, temporal + filtered %.6f" % (noisy, single, temporal))
    assert share >= 0.9
    assert temporal < single


def test_reset_drops_the_history(pan):
    """after reset() a frame is the first of a sequence: length 1 everywhere, and -- the camera being the last frame's -- the accumulated
    colour is that frame's beauty pass"""
    info = pan["info_again"]
    assert info["frame"] == 0 and (info["history_length"] == 1).all()
    assert np.array_equal(info["accumulated"], info["beauty"]) and np.array_equal(info["beauty"], pan["results"][-1][1]["beauty"])
    assert pan["td"].frames == 1
