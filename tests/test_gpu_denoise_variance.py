"""GPU suite (-m gpu): fjgpu_denoise_estimate_variance and fjgpu_denoise_variance (include/fjgpu.h) on the device against the numpy
restatement, tests/denoise_variance_model.py.

Tolerance: REL_TOL = 1e-4 with denoise_model.rel_err (denominator floored at 1e-3), the project's pixel tolerance, for colours and
variances alike.  The device and numpy differ in expf (a few ulp) and its propagation through the luminance term and the variance of
later iterations; every comparison prints the largest error it saw.  Where two device results are compared with each other they are
bit-identical: the kernels have no atomics and a fixed order of taps.  The shapes are those at which the tiling can go wrong: a region
of a small frame, exactly one block of 64 x 4 and one lane and one row more, single pixels, rows and columns, and a frame of many
blocks ragged both ways (the estimate's LDS footprint is 70 x 10 around each block).
"""
import numpy as np
import pytest

import denoise_model as dm
import denoise_variance_model as dvm
from fujiyama_renderer_amd import gpu, host, workloads
from test_albedo_cpu import FLOOR, random_albedo
from test_denoise_cpu import REGION, random_inputs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4
GUIDES = dict(sigma_normal=0.8, sigma_position=1.2)
SIGMA_L = 2.5


def check(got, ref, what):
    err = float(dm.rel_err(got, ref).max())
    print("denoise_variance %-50s max rel err %.3e" % (what, err))
    assert np.isfinite(got).all()
    assert err <= REL_TOL, (what, err)


@pytest.fixture(scope="module")
def small():
    return random_inputs()


@pytest.fixture(scope="module")
def big():
    """200 x 150: four blocks of 64 pixels across (the last one ragged), 38 blocks of 4 rows down (the last one ragged)"""
    return random_inputs(W=200, H=150, seed=7)


@pytest.fixture(scope="module")
def albedo_small(small):
    """the inputs of tests/test_gpu_denoise_albedo.py: the same frames with test_albedo_cpu's random albedo"""
    return small + (random_albedo(),)


@pytest.fixture(scope="module")
def albedo_big(big):
    return big + (random_albedo(W=200, H=150, seed=11),)


def supplied(shape):
    return (np.random.default_rng(5).random(shape[:2]) * 0.5).astype(np.float32)


def both(color, normal, position, ids, what, **kw):
    """filter on the device and in the model with the same parameters; colour and variance checked"""
    got, var, st = gpu.denoise_variance(color, normal, position, ids, sigma_luminance=SIGMA_L, return_variance=True, **kw)
    ref, ref_var = dvm.denoise_variance(color, normal, position, ids, sigma_luminance=SIGMA_L, **kw)
    check(got, ref, what + ", colour")
    check(var, ref_var, what + ", variance")
    return got, var, st


REGIONS = [REGION, (0, 0, 64, 4), (0, 0, 65, 5), (66, 20, 67, 21), (0, 0, 1, 1), (0, 7, 67, 8), (5, 0, 6, 21)]


@pytest.mark.parametrize("region", REGIONS)
def test_estimate_on_regions(small, region):
    color, normal, position, ids = small
    got, st = gpu.estimate_variance(color, normal, position, ids, region=region, **GUIDES)
    check(got, dvm.estimate_variance(color, normal, position, ids, region=region, **GUIDES), "estimate, region %s" % (region,))
    assert got.shape == color.shape[:2] and got.dtype == np.float32 and st.gen_ms > 0 and st.batches == 0
    inside = np.zeros(color.shape[:2], dtype=bool)
    inside[region[1]:region[3], region[0]:region[2]] = True
    assert (got[~inside] == 0).all()


@pytest.mark.parametrize("stop", [0, 1])
def test_estimate_full_frame_of_many_blocks(big, stop):
    color, normal, position, ids = big
    got, _ = gpu.estimate_variance(color, normal, position, ids, stop_at_ids=bool(stop), **GUIDES)
    check(got, dvm.estimate_variance(color, normal, position, ids, stop_at_ids=bool(stop), **GUIDES), "estimate 200x150, stop %d" % stop)
    # (with the stop a pixel whose 48 neighbours all carry other ids keeps its centre tap alone: variance exactly 0)
    assert got.min() > 0 if not stop else got.min() >= 0 and (got > 0).mean() > 0.99


@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("given", [False, True], ids=["estimated", "supplied"])
def test_region_of_a_small_frame(small, iterations, given):
    color, normal, position, ids = small
    v = supplied(color.shape) if given else None
    got, var, st = both(color, normal, position, ids, "67x21 region, %d iterations, %s" % (iterations, "supplied" if given else "estimated"),
                        variance=v, iterations=iterations, region=REGION, **GUIDES)
    inside = np.zeros(color.shape[:2], dtype=bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    assert np.array_equal(got[~inside], color[~inside]) and not np.array_equal(got[inside], color[inside])
    assert (var[~inside] == 0).all() and (var[inside] > 0).all()
    assert st.batches == iterations and st.total_ms > 0 and st.resolve_ms > 0 and st.gen_ms > 0


@pytest.mark.parametrize("region", REGIONS[1:])
@pytest.mark.parametrize("given", [False, True], ids=["estimated", "supplied"])
def test_block_edges_and_degenerate_regions(small, region, given):
    """exactly one block, one lane and one row more, one pixel (both corners of the frame), one row, one column"""
    color, normal, position, ids = small
    both(color, normal, position, ids, "region %s" % (region,), variance=supplied(color.shape) if given else None, iterations=3,
         region=region, **GUIDES)


@pytest.mark.parametrize("given", [False, True], ids=["estimated", "supplied"])
def test_full_frame_of_many_blocks(big, given):
    color, normal, position, ids = big
    both(color, normal, position, ids, "200x150 full frame", variance=supplied(color.shape) if given else None, iterations=5, **GUIDES)


@pytest.mark.parametrize("missing", ["normal", "position", "ids"])
def test_a_missing_guide_switches_its_term_off(small, missing):
    color, normal, position, ids = small
    g = dict(normal=normal, position=position, ids=ids)
    g[missing] = None
    got, _, _ = both(color, g["normal"], g["position"], g["ids"], "without %s" % missing, iterations=3, **GUIDES)
    full, _ = gpu.denoise_variance(color, normal, position, ids, sigma_luminance=SIGMA_L, iterations=3, **GUIDES)
    assert not np.array_equal(got, full)
    est, _ = gpu.estimate_variance(color, g["normal"], g["position"], g["ids"], **GUIDES)
    check(est, dvm.estimate_variance(color, g["normal"], g["position"], g["ids"], **GUIDES), "estimate without %s" % missing)


@pytest.mark.parametrize("stop", [0, 1])
def test_id_stop(small, stop):
    color, normal, position, ids = small
    assert (ids[:, :, 0] == -1).any()
    both(color, normal, position, ids, "stop %d" % stop, iterations=3, stop_at_ids=bool(stop), **GUIDES)


@pytest.mark.parametrize("frame", ["albedo_small", "albedo_big"])
@pytest.mark.parametrize("given", [False, True], ids=["estimated", "supplied"])
def test_with_albedo(request, frame, given):
    color, normal, position, ids, albedo = request.getfixturevalue(frame)
    H, W = color.shape[:2]
    reg = REGION if frame == "albedo_small" else (1, 2, W - 1, H - 1)
    got, _, _ = both(color, normal, position, ids, "%s with albedo" % frame, albedo=albedo, albedo_floor=FLOOR,
                     variance=supplied(color.shape) if given else None, iterations=4, region=reg, **GUIDES)
    plain, _ = gpu.denoise_variance(color, normal, position, ids, sigma_luminance=SIGMA_L, variance=supplied(color.shape) if given else None,
                                    iterations=4, region=reg, **GUIDES)
    assert not np.array_equal(got, plain)


@pytest.mark.parametrize("iterations,region", [(1, None), (5, (1, 2, 199, 149)), (3, (0, 0, 65, 5))])
@pytest.mark.parametrize("stop", [0, 1])
def test_sigma_luminance_0_is_the_plain_filter_bit_for_bit(big, iterations, region, stop):
    color, normal, position, ids = big
    kw = dict(iterations=iterations, region=region, stop_at_ids=bool(stop), **GUIDES)
    got, _ = gpu.denoise_variance(color, normal, position, ids, sigma_luminance=0.0, **kw)
    ref, _ = gpu.denoise(color, normal, position, ids, sigma_color=0.0, **kw)
    assert np.array_equal(got, ref) and not np.array_equal(got, color)
    got, _ = gpu.denoise_variance(color, sigma_luminance=0.0, **kw)
    ref, _ = gpu.denoise(color, sigma_color=0.0, **kw)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("iterations", [1, 4])
@pytest.mark.parametrize("given", [False, True], ids=["estimated", "supplied"])
def test_in_place_equals_separate_buffers(big, iterations, given):
    import torch
    color, normal, position, ids = big
    kw = dict(sigma_luminance=SIGMA_L, variance=supplied(color.shape) if given else None, iterations=iterations, region=(1, 2, 199, 149),
              return_variance=True, **GUIDES)
    apart, var, _ = gpu.denoise_variance(color, normal, position, ids, **kw)
    t = torch.from_numpy(color).to("cuda:0")
    same, var_same, _ = gpu.denoise_variance(t, normal, position, ids, out=t, **kw)
    assert np.array_equal(same, apart) and np.array_equal(var_same, var)
    assert np.array_equal(t.cpu().numpy(), apart)
    # ... and a second call on the same inputs gives the same bits
    again, var_again, _ = gpu.denoise_variance(color, normal, position, ids, **kw)
    assert np.array_equal(again, apart) and np.array_equal(var_again, var)


def test_sentinels_outside_the_region_survive(small):
    import torch
    color, normal, position, ids = small
    out = torch.full(color.shape, -7.5, dtype=torch.float32, device="cuda:0")
    vout = torch.full(color.shape[:2], -7.5, dtype=torch.float32, device="cuda:0")
    got, var, _ = gpu.denoise_variance(color, normal, position, ids, sigma_luminance=SIGMA_L, iterations=5, region=REGION, out=out,
                                       variance_out=vout, **GUIDES)
    inside = np.zeros(color.shape[:2], dtype=bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    assert (got[~inside] == np.float32(-7.5)).all() and (var[~inside] == np.float32(-7.5)).all()
    ref, ref_var = dvm.denoise_variance(color, normal, position, ids, sigma_luminance=SIGMA_L, iterations=5, region=REGION, **GUIDES)
    check(got[inside], ref[inside], "sentinel frame, colour")
    check(var[inside], ref_var[inside], "sentinel frame, variance")
    # garbage outside the region of every input changes nothing inside
    junk = [a.copy() for a in (color, normal, position)]
    for a in junk:
        a[~inside] = np.float32(1e30)
    jids = ids.copy()
    jids[~inside] = 12345
    again, var_again, _ = gpu.denoise_variance(junk[0], junk[1], junk[2], jids, sigma_luminance=SIGMA_L, iterations=5, region=REGION,
                                               return_variance=True, **GUIDES)
    assert np.array_equal(again[inside], got[inside]) and np.array_equal(var_again[inside], var[inside])


def test_refusals_reach_python(small):
    import torch
    color, normal, position, ids = small
    with pytest.raises(gpu.GpuError, match="fjgpu_denoise_variance: sigma_luminance is NaN"):
        gpu.denoise_variance(color, normal, position, ids, sigma_luminance=float("nan"))
    v = torch.zeros(color.shape[:2], dtype=torch.float32, device="cuda:0")
    with pytest.raises(gpu.GpuError, match="variance_out"):
        gpu.denoise_variance(color, normal, position, ids, variance=v, variance_out=v)
    with pytest.raises(ValueError, match="variance"):
        gpu.denoise_variance(color, normal, position, ids, variance=np.zeros((3, 3), dtype=np.float32))


CORNELL = dict(res=(64, 48), mesh="tiny")


@pytest.fixture(scope="module")
def cornell(asset_dir):
    """the Cornell box at 2 x 2 spp through Scene.render_denoised plain, variance-guided and variance-guided with demodulation (inputs
    kept), and the device's 12 x 12 spp beauty frame as truth"""
    host.run_scene_text(workloads.cornell(asset_dir, spp=(12, 12), **CORNELL), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    truth, _ = gs.render_frame(rd)
    gs.close()
    host.run_scene_text(workloads.cornell(asset_dir, spp=(2, 2), **CORNELL), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    plain, _ = gs.render_denoised(rd)
    out, info = gs.render_denoised(rd, variance_guided=True, keep_inputs=True)
    dem, info_dem = gs.render_denoised(rd, variance_guided=True, keep_inputs=True, demodulate=True)
    gs.close()
    return dict(truth=truth, plain=plain, out=out, info=info, dem=dem, info_dem=info_dem)


def test_render_denoised_variance_guided_equals_model_on_its_own_inputs(cornell):
    info = cornell["info"]
    aov = info["aov"]
    assert sorted(aov) == ["ids", "normal", "position"]
    fg = aov["ids"][:, :, 0] >= 0
    p = aov["position"][fg].astype(np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    assert info["sigma_position"] == pytest.approx(gpu.SIGMA_POSITION_FRACTION_VARIANCE * diag, rel=1e-6)
    assert info["sigma_luminance"] == gpu.SIGMA_LUMINANCE
    ref, ref_var = dvm.denoise_variance(info["beauty"], aov["normal"], aov["position"], aov["ids"], iterations=gpu.DENOISE_ITERATIONS,
                                        sigma_luminance=gpu.SIGMA_LUMINANCE, sigma_normal=gpu.SIGMA_NORMAL,
                                        sigma_position=info["sigma_position"], stop_at_ids=True)
    check(cornell["out"], ref, "render_denoised(variance_guided), Cornell 64x48 at 2x2, colour")
    check(info["variance"], ref_var, "render_denoised(variance_guided), Cornell 64x48 at 2x2, variance")
    assert info["beauty_stats"].rays.camera == info["aov_stats"].rays.camera > 0
    assert info["denoise_stats"].batches == gpu.DENOISE_ITERATIONS


def test_render_denoised_variance_guided_and_demodulated_equals_model(cornell):
    info = cornell["info_dem"]
    aov = info["aov"]
    assert sorted(aov) == ["albedo", "ids", "normal", "position"] and info["albedo_floor"] == gpu.ALBEDO_FLOOR
    ref, ref_var = dvm.denoise_variance(info["beauty"], aov["normal"], aov["position"], aov["ids"], albedo=aov["albedo"],
                                        albedo_floor=info["albedo_floor"], iterations=gpu.DENOISE_ITERATIONS,
                                        sigma_luminance=info["sigma_luminance"], sigma_normal=gpu.SIGMA_NORMAL,
                                        sigma_position=info["sigma_position"], stop_at_ids=True)
    check(cornell["dem"], ref, "render_denoised(variance_guided, demodulate), Cornell, colour")
    check(info["variance"], ref_var, "render_denoised(variance_guided, demodulate), Cornell, variance")


def test_variance_guided_frame_is_nearer_the_truth_than_the_noisy_one(cornell):
    truth = cornell["truth"].astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))
    noisy, guided, plain = mse(cornell["info"]["beauty"]), mse(cornell["out"]), mse(cornell["plain"])
    print("Cornell 64x48: MSE against 12x12 spp: noisy 2x2 %.6f, variance-guided %.6f, plain filter %.6f" % (noisy, guided, plain))
    assert guided < noisy


def test_render_denoised_passes_on_the_aov_refusals(asset_dir):
    host.run_scene_text(workloads.buddhas(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny", extra=(("sampler_type", (1,)),)), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    try:
        with pytest.raises(gpu.GpuError, match="adaptive sampler"):
            gs.render_denoised(rd, variance_guided=True)
    finally:
        gs.close()


def test_does_not_disturb_rendering(asset_dir):
    """render_frame, fjgpu_denoise_variance, render_frame on a frame whose beauty render is reproducible to the bit (one light, no
    bounces: tests/test_gpu_aov.py): the same pixels and ray counts.  The call has no scene handle to touch."""
    text = workloads.buddhas(asset_dir, res=(40, 24), spp=(3, 2), mesh="tiny", nlights=1,
                             extra=(("tilesize", (16, 16)), ("filterwidth", (2, 2)), ("sample_jitter", (1,)),
                                    ("max_reflect_depth", (0,)), ("max_refract_depth", (0,))))
    host.run_scene_text(text, deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    try:
        fb0, st0 = gs.render_frame(rd)
        fb1, st1 = gs.render_frame(rd)
        work0 = gs.query("work_bytes")
        out, var, _ = gpu.denoise_variance(fb1, iterations=5, return_variance=True)
        est, _ = gpu.estimate_variance(fb1)
        assert gs.query("work_bytes") == work0
        fb2, st2 = gs.render_frame(rd)
    finally:
        gs.close()
    assert fb1.any() and np.array_equal(fb0, fb1)          # (the premise: the frame is reproducible)
    assert np.array_equal(fb1, fb2)
    assert st0.rays.as_dict() == st1.rays.as_dict() == st2.rays.as_dict()
    assert not np.array_equal(out, fb1) and est.any() and var.any()
