"""GPU suite (-m gpu): option "sampler_seed" (include/fjgpu.h; DESIGN.md 4, "Random streams").

1. Seed 0 is the renderer as it was: on tests/test_gpu_sample_variance.py's reproducible jittered frame the framebuffer, the sample
   variance, the six AOVs, the albedo, the camera rays of a tile and the ray counts are the same bits with the option set to 0 and with it
   never set.
2. The seeded camera samples are the reference's sampler fed with the seeded table: (u, v) computed here in numpy from
   fjgpu_host_xorshift_f01_seeded and FixedGridSampler::generate_samples' statements (src/fj_fixed_grid_sampler.cc:33-84), through the
   oracle's camera (fjo_camera_rays), bit for bit.
3. A seeded beauty frame against the oracle, which has no seed: a constant shader's sample is the constant on a hit and 0 on a miss, so
   the frame is the Gaussian resolve of the oracle's trace of the device's seeded rays.  The resolve used here is first held against the
   UNSEEDED frame, where the oracle's own render is the reference.
4. Determinism and batching under a seed; a scene that draws nothing does not change; frames of different seeds are independent draws of
   the estimator whose unseeded draw the oracle renders; the adaptive sampler; the option's range.
"""
import ctypes as C

import numpy as np
import pytest

import denoise_model as dm
import oracle_ffi
import sample_variance_model as svm
from fujiyama_renderer_amd import gpu, host, workloads
from test_gpu_aov import SceneView
from test_gpu_sample_variance import RAGGED, constant_object

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4          # tests/test_gpu_parity.py's


def prepare(text):
    host.run_scene_text(text, deferred=True)
    return host.get_desc()


def margins(rd):
    return svm.sampler_margin(rd.rate_x, rd.filter_w), svm.sampler_margin(rd.rate_y, rd.filter_h)


def seeded_uv(rd, rect, seed):
    """(u, v) [n, 2] of a tile's samples, k = y * nx + x, margin samples included: generate_samples' statements with the seeded table"""
    mx, my = margins(rd)
    nx, ny = rd.rate_x * (rect[2] - rect[0]) + 2 * mx, rd.rate_y * (rect[3] - rect[1]) + 2 * my
    tab = gpu.host_xorshift_f01_seeded(seed, 2 * nx * ny)
    udelta, vdelta = 1. / (rd.rate_x * rd.xres), 1. / (rd.rate_y * rd.yres)
    xoffset, yoffset = rect[0] * rd.rate_x - mx, rect[1] * rd.rate_y - my
    y, x = np.mgrid[0:ny, 0:nx]
    u = ((.5 + x + xoffset) * udelta).reshape(-1)
    v = (1 - (.5 + y + yoffset) * vdelta).reshape(-1)
    if rd.jitter > 0:
        jitter = float(rd.jitter)
        u = u + udelta * (tab[0::2] * jitter - .5)
        v = v + vdelta * (tab[1::2] * jitter - .5)
    return np.stack([u, v], axis=1), nx, ny


def oracle_rays(gs, rd, uv):
    """the oracle's camera rays [n, 8] of film positions uv through the camera the device scene renders with (static camera, time 0)"""
    O = oracle_ffi.lib()
    cam = gs.get_camera()
    uvt = np.ascontiguousarray(np.concatenate([uv, np.zeros((len(uv), 1))], axis=1), dtype=np.float64)
    out = np.empty((len(uv), 8))
    O.fjo_camera_rays(C.byref(cam), int(rd.xres), int(rd.yres), len(uv), uvt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def resolve_tile(rd, rect, uv, nx, radiance):
    """the Gaussian resolve of a tile: radiance [n, 4] f64 of its samples -> [h, w, 4] f32 (f64 sums, rounded once)"""
    mx, my = margins(rd)
    npx_x, npx_y = rd.rate_x + 2 * mx, rd.rate_y + 2 * my
    sy, sx = np.mgrid[0:npx_y, 0:npx_x]
    h, w = rect[3] - rect[1], rect[2] - rect[0]
    out = np.zeros((h, w, 4), dtype=np.float32)
    for py in range(h):
        for px in range(w):
            s = (py * rd.rate_y * nx + px * rd.rate_x + sy * nx + sx).reshape(-1)
            wt = svm.weight(rd.xres, rd.yres, rd.filter_w, rd.filter_h, rect[0] + px, rect[1] + py, uv[s, 0], uv[s, 1])
            out[py, px] = ((wt[:, None] * radiance[s]).sum(axis=0) / wt.sum()).astype(np.float32)
    return out


def with_seed(gs, seed, fn):
    before = gs.query("sampler_seed")
    gs.set_option("sampler_seed", seed)
    try:
        return fn()
    finally:
        gs.set_option("sampler_seed", int(before))


def check(got, ref, what, tol=REL_TOL):
    err = dm.rel_err(got, ref)
    print("sampler seed %-70s max rel err %.3e, %d of %d over" % (what, float(err.max()), int((err > tol).sum()), err.size))
    assert np.isfinite(got).all() and float(err.max()) <= tol, (what, float(err.max()))


@pytest.fixture(scope="module")
def ragged(asset_dir):
    sp, rd = prepare(workloads.buddhas(asset_dir, **RAGGED))
    gs = gpu.Scene(sp)
    yield dict(sp=sp, gs=gs, rd=rd)
    gs.close()


def everything(gs, rd):
    """every output the seed could reach, and the ray counts"""
    fb, st = gs.render_frame(rd)
    fb_v, var, st_v = gs.render_frame_variance(rd)
    aov, st_a = gs.render_aov_albedo(rd)
    return dict(fb=fb, fb_v=fb_v, var=var, rays=gs.camera_samples(rd, 0), counts=(st.rays.as_dict(), st_v.rays.as_dict(), st_a.rays.as_dict()),
                **{"aov_" + k: v for k, v in aov.items()})


# ---------------------------------------------------------------- 1. seed 0 is today
def test_seed_0_is_the_option_never_set(ragged, asset_dir):
    rd = ragged["rd"]
    assert rd.jitter > 0 and margins(rd)[0] > 0 and gpu.tile_count(rd) == 6
    unset = everything(ragged["gs"], rd)                       # (the module's scene has not seen the option yet: this test runs first)
    assert ragged["gs"].query("sampler_seed") == 0
    sp2, rd2 = prepare(workloads.buddhas(asset_dir, **RAGGED))
    g2 = gpu.Scene(sp2)
    try:
        g2.set_option("sampler_seed", 0)
        zero = everything(g2, rd2)
        g2.set_option("sampler_seed", 5)
        five = everything(g2, rd2)
        g2.set_option("sampler_seed", 0)
        back = everything(g2, rd2)
    finally:
        g2.close()
    assert set(unset) >= {"fb", "var", "aov_depth", "aov_position", "aov_normal", "aov_uv", "aov_ids", "aov_coverage", "aov_albedo", "rays"}
    for k in unset:
        if k == "counts":
            assert unset[k] == zero[k] == back[k] and unset[k][0]["shadow"] > 0
        else:
            assert np.array_equal(unset[k], zero[k]) and np.array_equal(unset[k], back[k]), k
    assert not np.array_equal(unset["fb"], five["fb"]) and not np.array_equal(unset["rays"], five["rays"])
    assert not np.array_equal(unset["aov_coverage"], five["aov_coverage"])


# ---------------------------------------------------------------- 2. the seeded samples
@pytest.mark.parametrize("seed", [1, 65535])
def test_camera_samples_are_the_references_sampler_on_the_seeded_table(ragged, seed):
    gs = ragged["gs"]
    rd = ragged["rd"].copy()
    rd.tile_w = rd.tile_h = 8                                   # 5 x 3 tiles of the 40 x 24 frame: tile 6 is interior, tile 14 the last corner
    assert gpu.tile_count(rd) == 15
    for tile in (6, 14, 0):
        rect = gpu.tile_rect(rd, tile)
        uv, nx, ny = seeded_uv(rd, rect, seed)
        want = oracle_rays(gs, rd, uv)
        got = with_seed(gs, seed, lambda: gs.camera_samples(rd, tile))
        assert got.shape == want.shape == (nx * ny, 8)
        assert np.array_equal(got, want), (seed, tile, float(np.abs(got - want).max()))
        uv0, _, _ = seeded_uv(rd, rect, 0)
        assert np.array_equal(gs.camera_samples(rd, tile), oracle_rays(gs, rd, uv0)) and not np.array_equal(uv, uv0)


# ---------------------------------------------------------------- 3. a seeded beauty frame against the oracle
def test_seeded_constant_object_is_the_resolve_of_the_oracles_trace(asset_dir):
    sp, rd = prepare(constant_object(asset_dir))
    assert (rd.xres, rd.yres) == (48, 40) and (rd.rate_x, rd.rate_y) == (3, 3) and rd.filter_w == 2 and rd.jitter > 0
    const = np.array([.7, .4, .2, 1.])
    gs = gpu.Scene(sp)
    osc = oracle_ffi.OracleScene(sp)
    group = SceneView(sp).target_group
    try:
        frames, covs, expect, share = {}, {}, {}, {}
        for seed in (0, 7):
            frames[seed] = with_seed(gs, seed, lambda: gs.render_frame(rd)[0])
            covs[seed] = with_seed(gs, seed, lambda: gs.render_aov(rd, want=("coverage",))[0]["coverage"][..., 0])
            expect[seed] = np.zeros((rd.yres, rd.xres, 4), np.float32)
            share[seed] = np.zeros((rd.yres, rd.xres), np.float32)
            mx, my = margins(rd)
            for tile in range(gpu.tile_count(rd)):
                rect = gpu.tile_rect(rd, tile)
                rays = with_seed(gs, seed, lambda: gs.camera_samples(rd, tile))
                uv, nx, ny = seeded_uv(rd, rect, seed)
                assert np.array_equal(rays, oracle_rays(gs, rd, uv))
                hit = osc.trace(group, rays)[1][:, 0] >= 0
                expect[seed][rect[1]:rect[3], rect[0]:rect[2]] = resolve_tile(rd, rect, uv, nx, hit[:, None] * const[None, :])
                h, w = rect[3] - rect[1], rect[2] - rect[0]
                kk = np.arange(nx * ny).reshape(ny, nx)[my:my + rd.rate_y * h, mx:mx + rd.rate_x * w].reshape(h, rd.rate_y, w, rd.rate_x)
                kk = kk.transpose(0, 2, 1, 3).reshape(h, w, -1)
                share[seed][rect[1]:rect[3], rect[0]:rect[2]] = hit[kk].sum(axis=2).astype(np.float32) / np.float32(rd.rate_x * rd.rate_y)
        ref, _ = osc.render(rd)
    finally:
        osc.close()
        gs.close()
    check(expect[0], ref, "premise: the resolve of the unseeded rays is the oracle's frame")
    check(frames[0], ref, "premise: the unseeded frame is the oracle's")
    check(frames[7], expect[7], "seed 7: the frame against the resolve of the oracle's trace of its rays")
    assert np.array_equal(covs[7], share[7]) and np.array_equal(covs[0], share[0])
    edge = (covs[0] > 0) & (covs[0] < 1)
    moved = (frames[7] != frames[0]).any(axis=2)
    print("constant object: %d silhouette pixels, %d of them differ under seed 7; %d pixels differ in all" % (edge.sum(), (moved & edge).sum(), moved.sum()))
    assert edge.sum() > 20 and (moved & edge).sum() > edge.sum() // 2


# ---------------------------------------------------------------- 4. determinism and batching
def test_seeded_frames_are_deterministic_and_batch_alike(ragged):
    import torch
    gs, rd = ragged["gs"], ragged["rd"]
    dev = torch.device("cuda", 0)

    def body():
        a, st_a = gs.render_frame(rd)
        b, st_b = gs.render_frame(rd)
        assert np.array_equal(a, b) and st_a.rays.as_dict() == st_b.rays.as_dict()
        fbt = torch.full((rd.yres, rd.xres, 4), -7.5, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        for t in range(gpu.tile_count(rd)):
            assert gs.render_tiles(rd, [t], fbt.data_ptr()).batches == 1
        assert np.array_equal(fbt.cpu().numpy(), a)
        gs.set_option("batch_tiles", 1)
        try:
            c, st_c = gs.render_frame(rd)
        finally:
            gs.set_option("batch_tiles", 0)
        assert st_c.batches == gpu.tile_count(rd) and np.array_equal(c, a)
        fb_v, var, st_v = gs.render_frame_variance(rd)
        assert np.array_equal(fb_v, a) and st_v.rays.as_dict() == st_a.rays.as_dict() and (var > 0).any()
        return a

    seeded = with_seed(gs, 3, body)
    unseeded, _ = gs.render_frame(rd)
    assert gs.query("sampler_seed") == 0 and not np.array_equal(seeded, unseeded)


def test_a_scene_that_draws_nothing_does_not_change(asset_dir):
    kw = dict(RAGGED)
    kw["extra"] = tuple(e for e in RAGGED["extra"] if e[0] != "sample_jitter") + (("sample_jitter", (0,)),)
    sp, rd = prepare(workloads.buddhas(asset_dir, **kw))
    assert rd.jitter == 0
    gs = gpu.Scene(sp)
    try:
        a, st_a = gs.render_frame(rd)
        b, st_b = with_seed(gs, 9, lambda: gs.render_frame(rd))
        rays = [with_seed(gs, s, lambda: gs.camera_samples(rd, 1)) for s in (0, 9)]
    finally:
        gs.close()
    assert a.any() and np.array_equal(a, b) and st_a.rays.as_dict() == st_b.rays.as_dict() and np.array_equal(rays[0], rays[1])


# ---------------------------------------------------------------- 5. independent draws of the oracle's estimator
def mse(a, b):
    return float(np.mean((np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]) ** 2))


@pytest.fixture(scope="module")
def cornell_frames(asset_dir):
    sp, rd = prepare(workloads.cornell(asset_dir, res=(64, 48), spp=(2, 2), mesh="tiny"))
    gs = gpu.Scene(sp)
    osc = oracle_ffi.OracleScene(sp)
    try:
        frames = [with_seed(gs, s, lambda: gs.render_frame(rd)[0]) for s in range(1, 33)]
        oracle, _ = osc.render(rd)
    finally:
        osc.close()
        gs.close()
    return dict(frames=frames, oracle=oracle)


def test_frames_of_different_seeds_are_independent(cornell_frames):
    f = [x.astype(np.float64) for x in cornell_frames["frames"]]
    assert len(f) == 32 and all(np.isfinite(x).all() for x in f)
    A, B = np.mean(f[:16], axis=0), np.mean(f[16:], axis=0)
    pair = float(np.mean([mse(f[i], f[16 + i]) for i in range(16)]))
    R = mse(A, B) / pair if pair > 0 else float("nan")
    print("independence: mean pair mse %.4e, mse of the two means of 16 %.4e, R = %.4f (independent: 1 / 16 = 0.0625)" % (pair, mse(A, B), R))
    assert pair > 0
    assert 1 / 32 <= R <= 1 / 8


def test_seeded_frames_estimate_what_the_oracle_estimates(cornell_frames):
    f = [x.astype(np.float64) for x in cornell_frames["frames"]]
    O = cornell_frames["oracle"].astype(np.float64)
    single = float(np.mean([mse(x, O) for x in f]))
    ratio = mse(np.mean(f, axis=0), O) / single
    print("estimator: mean mse of a seeded frame against the oracle's %.4e, of the mean of 32 %.4e, ratio %.4f (unbiased: 0.516)" % (
        single, mse(np.mean(f, axis=0), O), ratio))
    assert 0.40 <= ratio <= 0.65


# ---------------------------------------------------------------- 6. the adaptive sampler, the option's range
def test_adaptive_sampler_takes_the_seed(asset_dir):
    adaptive = (("sampler_type", (1,)), ("adaptive_max_subdivision", (2,)), ("adaptive_subdivision_threshold", (.03,)))
    text = workloads.cornell(asset_dir, res=(48, 32), spp=(2, 2), mesh="tiny", extra=adaptive)
    sp, rd = prepare(text)
    assert rd.sampler_type == 1
    gs = gpu.Scene(sp)
    try:
        unset, st_u = gs.render_frame(rd)
        zero, st_0 = with_seed(gs, 0, lambda: gs.render_frame(rd))
        one, st_1 = with_seed(gs, 1, lambda: gs.render_frame(rd))
        two, st_2 = with_seed(gs, 2, lambda: gs.render_frame(rd))
    finally:
        gs.close()
    assert np.array_equal(unset, zero) and st_u.rays.as_dict() == st_0.rays.as_dict()
    assert not np.array_equal(one, two) and not np.array_equal(one, unset)
    assert np.isfinite(one).all() and np.isfinite(two).all()


def test_option_range_and_query(ragged):
    gs = ragged["gs"]
    for bad in (-1, 65536):
        with pytest.raises(gpu.GpuError) as e:
            gs.set_option("sampler_seed", bad)
        assert "sampler_seed" in str(e.value) and "0..65535" in str(e.value)
    assert gs.query("sampler_seed") == 0
    for s in (1, 65535, 0):
        gs.set_option("sampler_seed", s)
        assert gs.query("sampler_seed") == s
