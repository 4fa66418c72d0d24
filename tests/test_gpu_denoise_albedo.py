"""GPU suite (-m gpu): fjgpu_denoise_albedo (include/fjgpu.h) -- the denoiser between a division by the albedo and a multiplication.

Bit tests.  Demodulation and remodulation are one correctly rounded f32 operation per value, which torch's f32 division and
multiplication on the device are as well, and the filter in between has no atomics and a fixed order of taps: gpu.denoise(C, albedo=A,
albedo_floor=f) must be BIT-IDENTICAL to gpu.denoise(C / a') * a' with a' = max-like clamp of A at f done in torch.  Against the numpy
model (tests/albedo_model.py: demodulated_denoise) the bound is the project's REL_TOL (expf differs by a few ulp).
"""
import numpy as np
import pytest

import albedo_model as am
import denoise_model as dm
import edge_scenes
from fujiyama_renderer_amd import gpu, host
from test_albedo_cpu import FLOOR, random_albedo
from test_denoise_cpu import REGION, SIGMAS, random_inputs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4


def check(got, ref, what):
    err = float(dm.rel_err(got, ref).max())
    print("denoise_albedo %-40s max rel err %.3e" % (what, err))
    assert np.isfinite(got).all()
    assert err <= REL_TOL, (what, err)


@pytest.fixture(scope="module")
def small():
    return random_inputs() + (random_albedo(),)


@pytest.fixture(scope="module")
def big():
    return random_inputs(W=200, H=150, seed=7) + (random_albedo(W=200, H=150, seed=11),)


def torch_demodulated(color, normal, position, ids, albedo, floor, region=None, in_place=False, **kw):
    """gpu.denoise(C / a') * a' with the division and the multiplication in torch f32 on the device, alpha and the pixels outside the
    region left alone"""
    import torch
    c = torch.from_numpy(color).to("cuda:0")
    a = torch.from_numpy(albedo).to("cuda:0")
    f = torch.tensor(floor, dtype=torch.float32, device="cuda:0")
    H, W = color.shape[:2]
    x0, y0, x1, y1 = (0, 0, W, H) if region is None else region
    ac = torch.where(a > f, a, f)[y0:y1, x0:x1]
    d = c.clone()
    d[y0:y1, x0:x1, :3] = c[y0:y1, x0:x1, :3] / ac
    out = d if in_place else None
    F, _ = gpu.denoise(d, normal, position, ids, region=region, out=out, **kw)
    F = torch.from_numpy(F).to("cuda:0")
    res = c.clone()
    res[y0:y1, x0:x1, :3] = F[y0:y1, x0:x1, :3] * ac
    res[y0:y1, x0:x1, 3] = F[y0:y1, x0:x1, 3]
    return res.cpu().numpy()


@pytest.mark.parametrize("frame", ["small", "big"])
@pytest.mark.parametrize("region", [None, "inner"])
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("in_place", [False, True])
def test_bit_identical_to_torch_demodulation(request, frame, region, iterations, in_place):
    import torch
    color, normal, position, ids, albedo = request.getfixturevalue(frame)
    H, W = color.shape[:2]
    reg = None if region is None else (REGION if frame == "small" else (1, 2, W - 1, H - 1))
    kw = dict(iterations=iterations, **SIGMAS)
    ref = torch_demodulated(color, normal, position, ids, albedo, FLOOR, region=reg, in_place=in_place, **kw)
    if in_place:
        t = torch.from_numpy(color).to("cuda:0")
        got, st = gpu.denoise(t, normal, position, ids, region=reg, out=t, albedo=albedo, albedo_floor=FLOOR, **kw)
        assert np.array_equal(t.cpu().numpy(), got)
    else:
        got, st = gpu.denoise(color, normal, position, ids, region=reg, albedo=albedo, albedo_floor=FLOOR, **kw)
    assert np.array_equal(got, ref)
    assert st.batches == iterations and st.gen_ms > 0 and st.resolve_ms > 0
    if not in_place:
        model = am.demodulated_denoise(color, normal, position, ids, albedo=albedo, albedo_floor=FLOOR, region=reg, **kw)
        check(got, model, "%s %s %d iterations" % (frame, reg, iterations))
        # albedo=None is the call without the parameter
        none, _ = gpu.denoise(color, normal, position, ids, region=reg, albedo=None, albedo_floor=FLOOR, **kw)
        plain, _ = gpu.denoise(color, normal, position, ids, region=reg, **kw)
        assert np.array_equal(none, plain) and not np.array_equal(got, plain)


def test_only_region_pixels_are_read_and_written(small):
    import torch
    color, normal, position, ids, albedo = small
    inside = np.zeros(color.shape[:2], dtype=bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    kw = dict(iterations=5, region=REGION, albedo_floor=FLOOR, **SIGMAS)
    clean, _ = gpu.denoise(color, normal, position, ids, albedo=albedo, **kw)
    junk = albedo.copy()
    junk[~inside] = np.nan
    out = torch.full(color.shape, -7.5, dtype=torch.float32, device="cuda:0")
    got, _ = gpu.denoise(color, normal, position, ids, albedo=junk, out=out, **kw)
    assert (got[~inside] == np.float32(-7.5)).all()
    assert np.array_equal(got[inside], clean[inside]) and np.isfinite(got[inside]).all()


def test_a_bad_floor_is_refused(small):
    color, normal, position, ids, albedo = small
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(gpu.GpuError, match="albedo_floor"):
            gpu.denoise(color, normal, position, ids, albedo=albedo, albedo_floor=floor)
    with pytest.raises(ValueError, match="albedo"):
        gpu.denoise(color, normal, position, ids, albedo=albedo[:, :, :2])


TEXTURED = edge_scenes.EDGE_CASES["textures_diffuse_and_bump"]


@pytest.fixture(scope="module")
def textured(asset_dir):
    """the textured scene at 2 x 2 spp through Scene.render_denoised, plain and demodulated (inputs kept), and the device's 12 x 12 spp frame"""
    host.run_scene_text(edge_scenes.custom_scene(asset_dir, **dict(TEXTURED, spp=(12, 12))), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    truth, _ = gs.render_frame(rd)
    gs.close()
    host.run_scene_text(edge_scenes.custom_scene(asset_dir, **TEXTURED), deferred=True)
    sp, rd = host.get_desc()
    tab = am.Tables(sp)
    gs = gpu.Scene(sp)
    plain, info_plain = gs.render_denoised(rd, keep_inputs=True)
    out, info = gs.render_denoised(rd, keep_inputs=True, demodulate=True)
    gs.close()
    return dict(truth=truth, plain=plain, info_plain=info_plain, out=out, info=info, tab=tab)


def test_render_denoised_demodulated_equals_model_on_its_own_inputs(textured):
    info = textured["info"]
    aov = info["aov"]
    assert sorted(aov) == ["albedo", "ids", "normal", "position"]
    assert aov["albedo"].shape == (48, 64, 3) and aov["albedo"].dtype == np.float32 and aov["albedo"].any()
    assert info["albedo_floor"] == gpu.ALBEDO_FLOOR
    ref = am.demodulated_denoise(info["beauty"], aov["normal"], aov["position"], aov["ids"], albedo=aov["albedo"], albedo_floor=info["albedo_floor"],
                                 iterations=gpu.DENOISE_ITERATIONS, sigma_color=gpu.SIGMA_COLOR, sigma_normal=gpu.SIGMA_NORMAL,
                                 sigma_position=info["sigma_position"], stop_at_ids=True)
    check(textured["out"], ref, "render_denoised(demodulate=True), textured 64x48 at 2x2")
    assert info["beauty_stats"].rays.camera == info["aov_stats"].rays.camera > 0
    assert info["aov_stats"].closest_launches == info["aov_stats"].batches
    assert info["denoise_stats"].batches == gpu.DENOISE_ITERATIONS


def test_demodulate_false_keeps_the_three_inputs(textured):
    info = textured["info_plain"]
    assert sorted(info["aov"]) == ["ids", "normal", "position"] and "albedo_floor" not in info
    ref = dm.denoise(info["beauty"], info["aov"]["normal"], info["aov"]["position"], info["aov"]["ids"], iterations=gpu.DENOISE_ITERATIONS,
                     sigma_color=gpu.SIGMA_COLOR, sigma_normal=gpu.SIGMA_NORMAL, sigma_position=info["sigma_position"], stop_at_ids=True)
    check(textured["plain"], ref, "render_denoised(), textured 64x48 at 2x2")
    assert np.array_equal(info["beauty"], textured["info"]["beauty"]) or info["beauty_stats"].rays.as_dict() == textured["info"]["beauty_stats"].rays.as_dict()


def test_demodulation_keeps_textures_nearer_the_truth(textured):
    """on the textured pixels (ids[3] a shader with a diffuse_map) against the device's 12 x 12 spp frame: the demodulated frame's error is
    smaller than the plain filter's.  CPU experiment (profiles/albedo_pass.txt): 0.001330 against 0.002695; the unfiltered 2 x 2 frame,
    which direct light from point lights leaves nearly noise-free, is at 0.000053 -- nearer than either."""
    truth = textured["truth"].astype(np.float64)
    sid = textured["info"]["aov"]["ids"][:, :, 3]
    m = np.array([s["diffuse_map"] >= 0 for s in textured["tab"].shaders] + [False])[sid]
    assert m.sum() > 1000
    mse = lambda a: float(np.mean((a.astype(np.float64)[m] - truth[m]) ** 2))
    noisy, plain, demod = mse(textured["info"]["beauty"]), mse(textured["plain"]), mse(textured["out"])
    print("textured 64x48, %d textured pixels: MSE against 12x12 spp: noisy 2x2 %.6f, plain denoise %.6f, demodulated %.6f" % (int(m.sum()), noisy, plain, demod))
    assert demod < plain
