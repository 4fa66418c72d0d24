"""GPU suite (-m gpu): fjgpu_denoise (include/fjgpu.h) on the device against the numpy restatement, tests/denoise_model.py.

Tolerance: REL_TOL = 1e-4 with the error measure of tests/test_gpu_parity.py (denominator floored at 1e-3), the project's pixel
tolerance.  The device and numpy differ in expf (a few ulp) and its propagation through the colour term of later iterations, and in
nothing else; every comparison prints the largest error it saw.  Where two device results are compared with each other they are
bit-identical: the kernel has no atomics and a fixed order of taps.
"""
import numpy as np
import pytest

import denoise_model as dm
from fujiyama_renderer_amd import gpu, host, workloads
from test_denoise_cpu import REGION, SIGMAS, random_inputs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4


def check(got, ref, what):
    err = float(dm.rel_err(got, ref).max())
    print("denoise %-40s max rel err %.3e" % (what, err))
    assert np.isfinite(got).all()
    assert err <= REL_TOL, (what, err)


@pytest.fixture(scope="module")
def small():
    return random_inputs()


@pytest.fixture(scope="module")
def big():
    """200 x 150: four blocks of 64 pixels across (the last one ragged), 38 blocks of 4 rows down (the last one ragged)"""
    return random_inputs(W=200, H=150, seed=7)


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_region_of_a_small_frame(small, iterations):
    """67 x 21, region (3, 2, 61, 19): at spacing 16 most taps fall outside the region; pixels outside it are the input's"""
    color, normal, position, ids = small
    got, st = gpu.denoise(color, normal, position, ids, iterations=iterations, region=REGION, **SIGMAS)
    ref = dm.denoise(color, normal, position, ids, iterations=iterations, region=REGION, **SIGMAS)
    check(got, ref, "67x21 region, %d iterations" % iterations)
    inside = np.zeros(color.shape[:2], dtype=bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    assert np.array_equal(got[~inside], color[~inside]) and not np.array_equal(got[inside], color[inside])
    assert st.batches == iterations and st.total_ms > 0 and st.resolve_ms > 0 and st.gen_ms > 0


def test_sentinel_outside_the_region_survives(small):
    import torch
    color, normal, position, ids = small
    out = torch.full(color.shape, -7.5, dtype=torch.float32, device="cuda:0")
    got, _ = gpu.denoise(color, normal, position, ids, iterations=5, region=REGION, out=out, **SIGMAS)
    inside = np.zeros(color.shape[:2], dtype=bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    assert (got[~inside] == np.float32(-7.5)).all()
    check(got[REGION[1]:REGION[3], REGION[0]:REGION[2]],
          dm.denoise(color, normal, position, ids, iterations=5, region=REGION, **SIGMAS)[REGION[1]:REGION[3], REGION[0]:REGION[2]], "sentinel frame")


def test_full_frame_of_many_blocks(big):
    color, normal, position, ids = big
    got, _ = gpu.denoise(color, normal, position, ids, iterations=5, **SIGMAS)
    check(got, dm.denoise(color, normal, position, ids, iterations=5, **SIGMAS), "200x150 full frame")


@pytest.mark.parametrize("region", [(66, 20, 67, 21), (0, 0, 1, 1), (0, 7, 67, 8), (5, 0, 6, 21)])
def test_degenerate_regions(small, region):
    """one pixel (both corners of the frame), one row, one column"""
    color, normal, position, ids = small
    got, _ = gpu.denoise(color, normal, position, ids, iterations=3, region=region, **SIGMAS)
    check(got, dm.denoise(color, normal, position, ids, iterations=3, region=region, **SIGMAS), "region %s" % (region,))


TERMS = [dict(sigma_color=0.7, sigma_normal=0.0, sigma_position=0.0), dict(sigma_color=0.0, sigma_normal=0.8, sigma_position=0.0),
         dict(sigma_color=0.0, sigma_normal=0.0, sigma_position=1.2), SIGMAS, dict(sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0)]


@pytest.mark.parametrize("sig", TERMS, ids=["colour", "normal", "position", "all", "none"])
@pytest.mark.parametrize("stop", [0, 1])
def test_terms_and_id_stop(small, sig, stop):
    """each term on alone, all together, none; with and without the stop at instance ids (ids -1 .. 2)"""
    color, normal, position, ids = small
    assert (ids[:, :, 0] == -1).any()
    got, _ = gpu.denoise(color, normal, position, ids, iterations=3, stop_at_ids=bool(stop), **sig)
    check(got, dm.denoise(color, normal, position, ids, iterations=3, stop_at_ids=bool(stop), **sig), "terms %s stop %d" % (sig, stop))


@pytest.mark.parametrize("missing", ["normal", "position", "ids"])
def test_a_missing_guide_switches_its_term_off(small, missing):
    color, normal, position, ids = small
    g = dict(normal=normal, position=position, ids=ids)
    g[missing] = None
    got, _ = gpu.denoise(color, iterations=3, **g, **SIGMAS)
    check(got, dm.denoise(color, iterations=3, **g, **SIGMAS), "without %s" % missing)
    full, _ = gpu.denoise(color, normal, position, ids, iterations=3, **SIGMAS)
    assert not np.array_equal(got, full)


@pytest.mark.parametrize("iterations", [1, 4])
def test_in_place_equals_separate_buffers(big, iterations):
    import torch
    color, normal, position, ids = big
    apart, _ = gpu.denoise(color, normal, position, ids, iterations=iterations, region=(1, 2, 199, 149), **SIGMAS)
    t = torch.from_numpy(color).to("cuda:0")
    same, _ = gpu.denoise(t, normal, position, ids, iterations=iterations, region=(1, 2, 199, 149), out=t, **SIGMAS)
    assert np.array_equal(same, apart)
    assert np.array_equal(t.cpu().numpy(), apart)
    # ... and a second call on the same inputs gives the same bits
    again, _ = gpu.denoise(color, normal, position, ids, iterations=iterations, region=(1, 2, 199, 149), **SIGMAS)
    assert np.array_equal(again, apart)


CORNELL = dict(res=(64, 48), mesh="tiny")


@pytest.fixture(scope="module")
def cornell(asset_dir):
    """the Cornell box at 2 x 2 spp through Scene.render_denoised (inputs kept), and the device's 12 x 12 spp beauty frame as truth"""
    host.run_scene_text(workloads.cornell(asset_dir, spp=(12, 12), **CORNELL), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    truth, _ = gs.render_frame(rd)
    gs.close()
    host.run_scene_text(workloads.cornell(asset_dir, spp=(2, 2), **CORNELL), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    out, info = gs.render_denoised(rd, keep_inputs=True)
    gs.close()
    return dict(truth=truth, out=out, info=info)


def test_render_denoised_equals_model_on_its_own_inputs(cornell):
    info = cornell["info"]
    aov = info["aov"]
    assert sorted(aov) == ["ids", "normal", "position"]
    fg = aov["ids"][:, :, 0] >= 0
    p = aov["position"][fg].astype(np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    assert info["sigma_position"] == pytest.approx(gpu.SIGMA_POSITION_FRACTION * diag, rel=1e-6)
    ref = dm.denoise(info["beauty"], aov["normal"], aov["position"], aov["ids"], iterations=gpu.DENOISE_ITERATIONS,
                     sigma_color=gpu.SIGMA_COLOR, sigma_normal=gpu.SIGMA_NORMAL, sigma_position=info["sigma_position"], stop_at_ids=True)
    check(cornell["out"], ref, "render_denoised, Cornell 64x48 at 2x2")
    assert info["beauty_stats"].rays.camera == info["aov_stats"].rays.camera > 0
    assert info["denoise_stats"].batches == gpu.DENOISE_ITERATIONS


def test_denoised_frame_is_nearer_the_truth_than_the_noisy_one(cornell):
    truth = cornell["truth"].astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))
    noisy, clean = mse(cornell["info"]["beauty"]), mse(cornell["out"])
    print("Cornell 64x48: MSE against 12x12 spp: noisy 2x2 %.6f, denoised %.6f" % (noisy, clean))
    assert clean < noisy


def test_render_denoised_passes_on_the_aov_refusals(asset_dir):
    host.run_scene_text(workloads.buddhas(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny", extra=(("sampler_type", (1,)),)), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    try:
        with pytest.raises(gpu.GpuError, match="adaptive sampler"):
            gs.render_denoised(rd)
    finally:
        gs.close()


def test_does_not_disturb_rendering(asset_dir):
    """render_frame, fjgpu_denoise, render_frame on a frame whose beauty render is reproducible to the bit (one light, no bounces:
    tests/test_gpu_aov.py): the same pixels and ray counts.  The call has no scene handle to touch."""
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
        out, _ = gpu.denoise(fb1, iterations=5)
        assert gs.query("work_bytes") == work0
        fb2, st2 = gs.render_frame(rd)
    finally:
        gs.close()
    assert fb1.any() and np.array_equal(fb0, fb1)          # (the premise: the frame is reproducible)
    assert np.array_equal(fb1, fb2)
    assert st0.rays.as_dict() == st1.rays.as_dict() == st2.rays.as_dict()
    assert not np.array_equal(out, fb1)
