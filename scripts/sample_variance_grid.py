#!/usr/bin/env python3
"""The experiment behind fjgpu_render_tiles_variance (profiles/sample_variance.txt, section 1), CPU only: what the variance-guided filter
gains when its input variance comes from the samples instead of the spatial estimate.  Cornell box 64 x 48 (tiny meshes), jitter 0.

The per-sample radiances are the oracle's frame at rate times the resolution, 1 x 1 spp, filter width 1: pixel (X, Y) of that frame is
sample (X, Y) of the coarse frame (tests/sample_variance_model.py: from_fine_frame).  The coarse frame is REBUILT from those samples with
the filter's weights -- the path tracer's random streams are keyed by the sample, so the oracle's own coarse frame is another draw -- and so
is the sample variance V (the corrected form of include/fjgpu.h).  Truth is the oracle at 12 x 12 spp.  AOVs and albedo come from the
oracle's trace of the tiles' camera rays (tests/albedo_model.py).  The filter is tests/denoise_variance_model.py at the shipped sigmas but
for sigma_luminance, which runs over 1 .. 16, over the INTERIOR -- the pixels whose filter window lies inside the fine frame -- and the
mean squared error over all four channels is taken there.  With an albedo both variances are those of the demodulated luminance.

    python scripts/sample_variance_grid.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import albedo_model as am                   # noqa: E402
import denoise_model as dm                  # noqa: E402
import denoise_variance_model as dvm        # noqa: E402
import oracle_ffi                           # noqa: E402
import sample_variance_model as svm         # noqa: E402
from test_gpu_aov import SceneView, all_tiles, expected_aov, prepare          # noqa: E402
from fujiyama_renderer_amd import gpu, workloads                              # noqa: E402

SIGMA_L = (1.0, 2.0, 4.0, 8.0, 16.0)


def experiment(asset, spp, truth):
    sp, rd = prepare(workloads.cornell(asset, res=(64, 48), spp=spp, mesh="tiny"))
    rd.jitter = 0
    view, tab = SceneView(sp), am.Tables(sp)
    osc = oracle_ffi.OracleScene(sp)
    fd = rd.copy()
    fd.xres, fd.yres = rd.xres * rd.rate_x, rd.yres * rd.rate_y
    fd.region[:] = (0, 0, fd.xres, fd.yres)
    fd.rate_x = fd.rate_y = 1
    fd.filter_w = fd.filter_h = 1.0
    fine, _ = osc.render(fd)
    src = am.OracleSamples(sp)
    aov, _, _ = expected_aov(src, osc, view, rd, all_tiles(rd))
    alb = am.expected_albedo(src, osc, view, tab, rd, all_tiles(rd))["albedo"]
    osc.close()
    normal, position, ids = aov["normal"].astype(np.float32), aov["position"].astype(np.float32), aov["ids"]
    fg = ids[:, :, 0] >= 0
    p = position[fg].astype(np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    geo = ((rd.xres, rd.yres), (rd.rate_x, rd.rate_y), (rd.filter_w, rd.filter_h))
    V, noisy, inside = svm.from_fine_frame(fine, *geo)
    Va, _, _ = svm.from_fine_frame(fine, *geo, albedo=alb, albedo_floor=gpu.ALBEDO_FLOOR)
    ys, xs = np.nonzero(inside)
    region = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
    truth64 = truth.astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64)[inside] - truth64[inside]) ** 2))
    print("%d x %d spp: window %d x %d samples, interior %s, %d foreground pixels, diagonal %.4f" % (
        spp + (rd.rate_x + 2 * svm.sampler_margin(rd.rate_x, rd.filter_w), rd.rate_y + 2 * svm.sampler_margin(rd.rate_y, rd.filter_h), region,
               int(fg.sum()), diag)))
    print("    noisy (rebuilt from the samples)          %.6f" % mse(noisy))
    guides = dict(sigma_normal=gpu.SIGMA_NORMAL, stop_at_ids=True, region=region)
    print("    plain filter, shipped sigmas              %.6f" % mse(dm.denoise(noisy, normal, position, ids, iterations=gpu.DENOISE_ITERATIONS,
                                                                                sigma_color=gpu.SIGMA_COLOR, sigma_position=gpu.SIGMA_POSITION_FRACTION * diag, **guides)))
    Vs = dvm.estimate_variance(noisy, normal, position, ids, sigma_position=gpu.SIGMA_POSITION_FRACTION_VARIANCE * diag, **guides)
    for name, v in (("spatial estimate", Vs), ("sample variance", V)):
        print("    %-18s of the luminance over the interior: mean %.6f, median %.6f, max %.4f" % (name, float(v[inside].mean()), float(np.median(v[inside])), float(v[inside].max())))
    for demodulate in (False, True):
        kw = dict(albedo=alb, albedo_floor=gpu.ALBEDO_FLOOR) if demodulate else {}
        print("    variance-guided, %d iterations, %s" % (gpu.DENOISE_ITERATIONS, "demodulated (floor %g)" % gpu.ALBEDO_FLOOR if demodulate else "not demodulated"))
        print("        sigma_luminance   spatial estimate   sample variance")
        for sl in SIGMA_L:
            row = []
            for vin in (None, Va if demodulate else V):
                out, _ = dvm.denoise_variance(noisy, normal, position, ids, variance=vin, iterations=gpu.DENOISE_ITERATIONS, sigma_luminance=sl,
                                              sigma_position=gpu.SIGMA_POSITION_FRACTION_VARIANCE * diag, **dict(guides, **kw))
                row.append(mse(out))
            print("        %-6g %s           %-12.6f       %-12.6f" % (sl, "(shipped)" if sl == gpu.SIGMA_LUMINANCE else "         ", row[0], row[1]))
    sys.stdout.flush()


if __name__ == "__main__":
    asset = workloads.default_asset_dir()
    sp, rd = prepare(workloads.cornell(asset, res=(64, 48), spp=(12, 12), mesh="tiny"))
    rd.jitter = 0
    osc = oracle_ffi.OracleScene(sp)
    truth, _ = osc.render(rd)
    osc.close()
    for spp in ((2, 2), (4, 4)):
        experiment(asset, spp, truth)
