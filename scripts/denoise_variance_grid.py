#!/usr/bin/env python3
"""The experiment behind gpu.SIGMA_LUMINANCE (profiles/denoise_variance.txt, section 2), CPU only: oracle frames at 2 x 2 spp (noisy) and
12 x 12 spp (truth), the AOVs and the albedo from the oracle's trace of the tiles' camera rays (tests/albedo_model.py, the reduction of
tests/test_gpu_aov.py), the filter of tests/denoise_variance_model.py with the variance estimated from the noisy frame.  The grid is
sigma_luminance in {1, 2, 4, 8, 16} times the sigma_normal / sigma_position grid of profiles/denoise_pass.txt at 5 iterations, with and
without albedo demodulation; the plain filter (tests/denoise_model.py at the shipped sigmas) is printed beside it.  Mean squared errors
over all four channels against the truth.

    python scripts/denoise_variance_grid.py [cornell] [textured]
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
import edge_scenes                          # noqa: E402
import oracle_ffi                           # noqa: E402
from test_gpu_aov import SceneView, all_tiles, expected_aov, prepare          # noqa: E402
from fujiyama_renderer_amd import gpu, workloads                              # noqa: E402

SIGMA_L = (1.0, 2.0, 4.0, 8.0, 16.0)
SIGMA_N = (0.1, 0.3, 1.0)
SIGMA_X = (0.01, 0.03, 0.1)          # fractions of the diagonal of the foreground's bounding box
ITERATIONS = 5


def experiment(name, make):
    sp, rd = prepare(make((12, 12)))
    osc = oracle_ffi.OracleScene(sp)
    truth, _ = osc.render(rd)
    osc.close()
    sp, rd = prepare(make((2, 2)))
    view, tab = SceneView(sp), am.Tables(sp)
    osc = oracle_ffi.OracleScene(sp)
    noisy, _ = osc.render(rd)
    src = am.OracleSamples(sp)
    aov, _, _ = expected_aov(src, osc, view, rd, all_tiles(rd))
    alb = am.expected_albedo(src, osc, view, tab, rd, all_tiles(rd))["albedo"]
    osc.close()
    normal, position, ids = aov["normal"].astype(np.float32), aov["position"].astype(np.float32), aov["ids"]
    fg = ids[:, :, 0] >= 0
    p = position[fg].astype(np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    truth64 = truth.astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth64) ** 2))
    print("%s: %d x %d, %d foreground pixels, diagonal %.4f" % (name, rd.xres, rd.yres, int(fg.sum()), diag))
    print("    noisy 2 x 2                               %.6f" % mse(noisy))
    plain = dict(iterations=gpu.DENOISE_ITERATIONS, sigma_color=gpu.SIGMA_COLOR, sigma_normal=gpu.SIGMA_NORMAL,
                 sigma_position=gpu.SIGMA_POSITION_FRACTION * diag, stop_at_ids=True)
    print("    plain filter, shipped sigmas              %.6f" % mse(dm.denoise(noisy, normal, position, ids, **plain)))
    print("    plain filter, demodulated                 %.6f" % mse(am.demodulated_denoise(noisy, normal, position, ids, albedo=alb,
                                                                                            albedo_floor=gpu.ALBEDO_FLOOR, **plain)))
    V = dvm.estimate_variance(noisy, normal, position, ids, sigma_normal=gpu.SIGMA_NORMAL, sigma_position=gpu.SIGMA_POSITION_FRACTION * diag)
    print("    estimated variance of the noisy frame's luminance (shipped guide sigmas): mean %.6f, median %.6f, max %.4f"
          % (float(V.mean()), float(np.median(V)), float(V.max())))
    best = {}
    for demodulate in (False, True):
        print("    variance-guided, stop_at_ids = 1, %d iterations, %s" % (ITERATIONS, "demodulated (floor %g)" % gpu.ALBEDO_FLOOR if demodulate else "not demodulated"))
        print("        sigma_luminance  sigma_normal   sigma_position = " + "   ".join("%g d" % f for f in SIGMA_X))
        for sl in SIGMA_L:
            for sn in SIGMA_N:
                row = []
                for fx in SIGMA_X:
                    out, _ = dvm.denoise_variance(noisy, normal, position, ids, albedo=alb if demodulate else None,
                                                  albedo_floor=gpu.ALBEDO_FLOOR, iterations=ITERATIONS, sigma_luminance=sl, sigma_normal=sn,
                                                  sigma_position=fx * diag, stop_at_ids=True)
                    row.append(mse(out))
                    if demodulate not in best or row[-1] < best[demodulate][0]:
                        best[demodulate] = (row[-1], sl, sn, fx)
                print("        %-6g %-6g  %s" % (sl, sn, "  ".join("%.6f" % v for v in row)))
        print("        best: %.6f at sigma_luminance %g, sigma_normal %g, sigma_position %g d" % best[demodulate])
    sys.stdout.flush()


if __name__ == "__main__":
    asset = workloads.default_asset_dir()
    which = sys.argv[1:] or ["cornell", "textured"]
    if "cornell" in which:
        experiment("cornell", lambda spp: workloads.cornell(asset, res=(64, 48), spp=spp, mesh="tiny"))
    if "textured" in which:
        experiment("textures_diffuse_and_bump",
                   lambda spp: edge_scenes.custom_scene(asset, **dict(edge_scenes.EDGE_CASES["textures_diffuse_and_bump"], spp=spp)))
