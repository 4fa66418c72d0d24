"""GPU suite (-m gpu): fjgpu_accumulate, fjgpu_accumulate_tile_error (include/fjgpu.h), Scene.render_progressive and
TemporalDenoiser(reseed=True).

1. The kernels against tests/accumulate_model.py on the frames and rectangle lists of tests/test_accumulate_cpu.py: state and variance
   bit for bit, tile errors within 1 f32 ulp (the model sums serially); a NaN pixel is skipped, pixels outside the rectangles keep a
   sentinel, reset ignores what is stored.
2. The variance of the mean is what gpu.denoise_variance takes.
3. render_progressive is the loop it stands for (set_option, render_tiles, accumulate), bit for bit, and leaves the scene's seed alone.
4. Convergence: tiles that show only background leave the active list after the second pass and are not rendered again; the camera
   rays traced are those of the active tiles.
5. TemporalDenoiser(reseed=True): a standing camera accumulates independent frames.
"""
import numpy as np
import pytest

import accumulate_cases as ac
import accumulate_model as am
import sample_variance_model as svm
from fujiyama_renderer_amd import gpu, host, workloads
from test_gpu_sample_variance import RAGGED, constant_object

pytestmark = pytest.mark.gpu

W, H = ac.W, ac.H


@pytest.fixture(autouse=True)
def the_entry_points():
    return gpu.lib().fjgpu_accumulate, gpu.lib().fjgpu_accumulate_tile_error


def prepare(text):
    host.run_scene_text(text, deferred=True)
    return host.get_desc()


def device_state(fill):
    s = gpu.new_accum_state((H, W))
    for t in s.values():
        t.fill_(float(fill))
    return s


def to_host(state):
    return {k: t.cpu().numpy() for k, t in state.items()}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


FRAMES = ac.frames(5)


# ---------------------------------------------------------------- 1. against the model
@pytest.mark.parametrize("name", sorted(ac.RECTS))
def test_device_equals_model(name):
    import torch
    rects = ac.RECTS[name]
    st_d, st_m = device_state(ac.SENTINEL), am.new_state(H, W, ac.SENTINEL)
    var_d = torch.full((H, W), float(ac.SENTINEL), dtype=torch.float32, device="cuda:0")
    var_m = np.full((H, W), ac.SENTINEL, np.float32)
    for i, f in enumerate(FRAMES):
        fr = f
        if i == 3:                               # a firefly: skipped, its neighbours advance
            fr = f.copy()
            fr[9, 20, 1] = np.nan
            fr[10, 3, 3] = np.inf
        _, _, st = gpu.accumulate(torch.from_numpy(np.ascontiguousarray(fr)).cuda(), st_d, rects=rects, reset=(i == 0), variance_out=var_d)
        am.accumulate(fr, st_m, rects, reset=(i == 0), variance_out=var_m)
        got = to_host(st_d)
        for k in ("mean", "m2", "count"):
            assert same_bits(got[k], st_m[k]), (name, i, k)
        assert same_bits(var_d.cpu().numpy(), var_m), (name, i)
        assert st.batches == 1 and st.total_ms >= 0
    inside = ac.inside(rects)
    got = to_host(st_d)
    for a in (got["mean"], got["m2"], got["count"], var_d.cpu().numpy()):
        assert np.all(a[~inside] == ac.SENTINEL)
    assert np.isfinite(got["mean"][inside]).all()
    if inside[9, 20]:
        assert got["count"][9, 20] == len(FRAMES) - 1 and got["count"][9, 21] == len(FRAMES)
    e_d, _ = gpu.tile_errors(st_d, rects=rects, lum_floor=ac.LUM_FLOOR)
    e_m = am.tile_errors(st_m, rects, ac.LUM_FLOOR)
    print("tile errors %s: device %s model %s" % (name, e_d, e_m))
    assert e_d.shape == e_m.shape and np.isfinite(e_d).all() and (e_d > 0).all()
    assert (ac.ulp_distance(e_d, e_m) <= 1).all()


def test_short_histories_and_reset():
    import torch
    st = device_state(np.nan)                    # stale NaN everywhere: reset must not look at it
    f = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in FRAMES[:2]]
    gpu.accumulate(f[0], st, reset=True)
    got = to_host(st)
    assert same_bits(got["mean"], FRAMES[0]) and np.all(got["m2"] == 0) and np.all(got["count"] == 1)
    e, _ = gpu.tile_errors(st, rects=ac.RECTS["ragged_split"])
    assert np.all(np.isposinf(e))
    gpu.accumulate(f[0], st)
    got = to_host(st)
    assert np.all(got["m2"] == 0) and np.all(got["count"] == 2) and same_bits(got["mean"], FRAMES[0])
    e, _ = gpu.tile_errors(st, rects=ac.RECTS["ragged_split"])
    assert np.all(e == 0)
    e, _ = gpu.tile_errors(st)
    assert e.shape == (1,) and e[0] == 0


# ---------------------------------------------------------------- 2. the denoiser takes the variance
def test_variance_feeds_the_variance_guided_denoiser():
    import torch
    st = gpu.new_accum_state((H, W))
    var = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    for f in FRAMES:
        gpu.accumulate(torch.from_numpy(np.ascontiguousarray(f)).cuda(), st, variance_out=var)
    v = var.cpu().numpy()
    assert np.isfinite(v).all() and (v >= 0).all() and (v > 0).any()
    out, vout, _ = gpu.denoise_variance(st["mean"], variance=var, iterations=2, return_variance=True)
    assert out.shape == (H, W, 4) and np.isfinite(out).all() and np.isfinite(vout).all() and (vout >= 0).all()
    assert not np.array_equal(out, st["mean"].cpu().numpy())


# ---------------------------------------------------------------- 3. render_progressive is its loop
@pytest.fixture(scope="module")
def ragged(asset_dir):
    sp, rd = prepare(workloads.buddhas(asset_dir, **RAGGED))
    gs = gpu.Scene(sp)
    yield dict(gs=gs, rd=rd)
    gs.close()


def test_render_progressive_is_the_manual_loop(ragged):
    import torch
    gs, rd = ragged["gs"], ragged["rd"]
    gs.set_option("sampler_seed", 11)
    try:
        mean, info = gs.render_progressive(rd, 4, first_seed=3)
        assert gs.query("sampler_seed") == 11
    finally:
        gs.set_option("sampler_seed", 0)
    dev = torch.device("cuda", 0)
    fb = torch.zeros((rd.yres, rd.xres, 4), dtype=torch.float32, device=dev)
    st = gpu.new_accum_state((rd.yres, rd.xres))
    var = torch.zeros((rd.yres, rd.xres), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    cam = 0
    for i in range(4):
        gs.set_option("sampler_seed", 3 + i)
        cam += gs.render_tiles(rd, None, fb.data_ptr()).rays.camera
        gpu.accumulate(fb, st, variance_out=var)
    gs.set_option("sampler_seed", 0)
    assert same_bits(mean, st["mean"].cpu().numpy()) and same_bits(info["variance"], var.cpu().numpy())
    assert np.all(info["count"] == 4) and info["rays"].camera == cam and info["rays"].shadow > 0
    assert info["active"] == [list(range(gpu.tile_count(rd)))] * 4 and info["errors"] == [None] * 4
    assert (info["variance"] > 0).any() and np.isfinite(mean).all()
    # the seed comes back on an exception too: seed 65535 + 1 is refused in the second pass
    gs.set_option("sampler_seed", 5)
    try:
        with pytest.raises(gpu.GpuError):
            gs.render_progressive(rd, 2, first_seed=65535)
        assert gs.query("sampler_seed") == 5
    finally:
        gs.set_option("sampler_seed", 0)


# ---------------------------------------------------------------- 4. convergence
def test_background_tiles_converge_after_two_passes(asset_dir):
    sp, rd = prepare(constant_object(asset_dir))
    rd.tile_w = rd.tile_h = 8                                  # 6 x 5 tiles of the 48 x 40 frame
    assert gpu.tile_count(rd) == 30 and rd.jitter > 0
    mx, my = svm.sampler_margin(rd.rate_x, rd.filter_w), svm.sampler_margin(rd.rate_y, rd.filter_h)
    samples = lambda t: ((gpu.tile_rect(rd, t)[2] - gpu.tile_rect(rd, t)[0]) * rd.rate_x + 2 * mx) * \
        ((gpu.tile_rect(rd, t)[3] - gpu.tile_rect(rd, t)[1]) * rd.rate_y + 2 * my)
    gs = gpu.Scene(sp)
    try:
        # measured first: the errors of every tile after two passes
        _, probe = gs.render_progressive(rd, 2, target_error=-1.0)
        e2 = probe["errors"][1]
        assert np.all(np.isposinf(probe["errors"][0])) and len(e2) == 30 and np.isfinite(e2).all()
        background = [t for t in range(30) if e2[t] == 0]       # (every sample of both passes missed -- or, inside the object, hit)
        silhouette = [t for t in range(30) if e2[t] > 0]
        print("errors after pass 2: tiles %s: 0 (background); silhouette tiles %s: %s" % (background, silhouette, e2[silhouette]))
        assert len(background) >= 4 and len(silhouette) >= 4 and 0 in background
        target = float(e2[silhouette].min()) * 1e-3            # between the background's 0 and every silhouette tile, which only shrink as 1 / sqrt(n)
        _, two = gs.render_progressive(rd, 2, target_error=target, keep_state=True)
        snapshot = two["state"]["mean"].cpu().numpy()
        mean, info = gs.render_progressive(rd, 6, target_error=target)
        scratch = _scratch(rd)
        frame_st = gs.render_tiles(rd, None, scratch.data_ptr())
    finally:
        gs.close()
    assert info["active"][0] == info["active"][1] == list(range(30))
    for p in range(2, 6):
        assert info["active"][p] == silhouette, (p, info["active"][p])
    for t in background:
        x0, y0, x1, y1 = gpu.tile_rect(rd, t)
        assert np.all(info["count"][y0:y1, x0:x1] == 2)
        assert same_bits(mean[y0:y1, x0:x1], snapshot[y0:y1, x0:x1])
    assert np.all(mean[0:8, 0:8] == 0)                          # tile 0 is a corner of the empty background
    for t in silhouette:
        x0, y0, x1, y1 = gpu.tile_rect(rd, t)
        assert np.all(info["count"][y0:y1, x0:x1] == 6)
    want = sum(sum(samples(t) for t in active) for active in info["active"])
    print("camera rays: %d over 6 passes, a frame's %d" % (info["rays"].camera, frame_st.rays.camera))
    assert info["rays"].camera == want < 6 * frame_st.rays.camera
    assert all(np.all(info["errors"][p][np.isfinite(info["errors"][p])] >= 0) for p in range(6))


def _scratch(rd):
    import torch
    t = torch.zeros((rd.yres, rd.xres, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------- 5. a standing camera
@pytest.fixture(scope="module")
def standing(asset_dir):
    """the Cornell box from one camera, 8 frames through TemporalDenoiser with and without reseed, against a 12 x 12 spp frame"""
    sp_ref, rd_ref = prepare(workloads.cornell(asset_dir, res=(64, 48), spp=(12, 12), mesh="tiny"))
    gs_ref = gpu.Scene(sp_ref)
    try:
        ref, _ = gs_ref.render_frame(rd_ref)
    finally:
        gs_ref.close()
    sp, rd = prepare(workloads.cornell(asset_dir, res=(64, 48), spp=(2, 2), mesh="tiny"))
    gs = gpu.Scene(sp)
    mse = lambda a: float(np.mean((a[..., :3].astype(np.float64) - ref[..., :3]) ** 2))
    out = dict(curves={}, acc={}, beauty={}, seed_after={})
    try:
        gs.set_option("sampler_seed", 9)                       # the scene's own seed, which a reseeding sequence must put back
        for reseed in (True, False):
            td = gpu.TemporalDenoiser(gs, rd, reseed=reseed)
            infos = [td.render(keep_inputs=True)[1] for _ in range(8)]
            out["acc"][reseed] = [i["accumulated"] for i in infos]
            out["beauty"][reseed] = [i["beauty"] for i in infos]
            out["curves"][reseed] = [mse(a) for a in out["acc"][reseed]]
            out["seed_after"][reseed] = gs.query("sampler_seed")
        gs.set_option("sampler_seed", 1)
        out["seed_1"] = gs.render_frame(rd)[0]
    finally:
        gs.close()
    print("accumulated colour against 12 x 12 spp, frames 1..8:    reseed %s" % " ".join("%.3e" % v for v in out["curves"][True]))
    print("                                                  no reseed %s" % " ".join("%.3e" % v for v in out["curves"][False]))
    return out


def _rel(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-3)).max())


def test_temporal_denoiser_reseed_renders_frame_k_under_seed_1_plus_k(standing):
    """the mechanics: frame k under seed 1 + k and the scene's seed back afterwards; without reseed the scene's seed for every frame"""
    assert standing["seed_after"] == {True: 9, False: 9}
    b = standing["beauty"]
    assert _rel(b[True][0], standing["seed_1"]) <= 1e-6                  # (frame 0: seed 1; the frames are not bit-reproducible)
    assert all(_rel(b[False][k], b[False][0]) <= 1e-6 for k in range(8))
    assert all(_rel(b[True][k], b[True][0]) > 1e-2 for k in range(1, 8))
    c = standing["curves"]
    assert all(c[True][k] < c[False][k] for k in range(1, 8)), c


def test_temporal_denoiser_reseed_lowers_the_error_of_a_standing_camera(standing):
    """the mse of the accumulated colour against a 12 x 12 spp frame is strictly lower at frame 8 than at frame 1.  Measured on an MI355X,
    frames 1..8: 1.770e-01 9.440e-02 6.555e-02 6.695e-02 4.699e-02 4.540e-02 4.042e-02 3.331e-02.  It holds because TemporalDenoiser
    reprojects a point on the ray through the pixel's CENTRE where it reseeds or the camera stands (_centre_position).  With the AOV
    pass's own position -- the hit of the pixel's nearest own sample, 0.28 pixels from the centre on average (|dx| 0.285, |dy| 0.281 over
    the foreground of this frame) -- the history of a standing camera is resampled bilinearly once per frame, and the same eight seeded
    frames gave 1.770e-01 1.086e-01 1.288e-01 1.235e-01 1.855e-01 1.699e-01 2.369e-01 2.735e-01."""
    c = standing["curves"][True]
    assert c[7] < c[0], c
    assert c[7] < c[0] / 4, c                  # (eight independent frames under alpha = max(1 / n, 0.1): 1 / 8 of the noise, plus what never averages out)


def test_temporal_denoiser_without_reseed_repeats_itself(standing):
    """with reseed=False frames 1 and 8 of the accumulated colour agree to 1e-4 (denoise_model.rel_err's measure): a camera that stands
    fetches every pixel's history from that pixel.  Measured on an MI355X: 1.1e-7, and the mse against the 12 x 12 spp frame stays at
    1.805e-01 over the eight frames.  Two things make it so, both in TemporalDenoiser.render for a camera that has not moved since the
    frame before: the point that is projected is slid onto the ray through the pixel's centre, and the fetch is keyed by the pixel's
    index, so that the neighbour tap of weight 2e-6 that f32's rounding of the point leaves does not count.  Without the first the
    accumulated colour of frame 2 differed from frame 1's on 3775 of 12288 values, by up to 4.05 (4.74 at frame 8, the mse rising to
    3.704e-01); with the first alone dark pixels beside bright ones still moved by 2e-3 per frame (1.7e-2 at frame 8)."""
    a = standing["acc"][False]
    c = standing["curves"][False]
    print("no reseed: frames 1 and 8 of the accumulated colour differ by %.3e" % _rel(a[0], a[7]))
    assert _rel(a[0], a[7]) <= 1e-4, _rel(a[0], a[7])
    assert max(c) - min(c) <= 1e-3 * c[0], c                  # (colours that agree to 1e-4 give mean squared errors that agree to a few 1e-4)
