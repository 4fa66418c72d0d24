#!/usr/bin/env python3
"""The experiment behind gpu.ALBEDO_FLOOR (profiles/albedo_pass.txt, section 2), CPU only: oracle frames at 2 x 2 spp (noisy) and
12 x 12 spp (truth), the AOVs and the albedo from the oracle's trace of the tiles' camera rays (tests/albedo_model.py, the reduction
of tests/test_gpu_aov.py), the filter of tests/denoise_model.py at the shipped sigmas, plain and between a numpy demodulation and
remodulation at each floor of the grid.  Prints mean squared errors against the truth.

    python scripts/albedo_floor_grid.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import albedo_model as am          # noqa: E402
import denoise_model as dm         # noqa: E402
import edge_scenes                 # noqa: E402
import oracle_ffi                  # noqa: E402
from test_gpu_aov import SceneView, all_tiles, expected_aov, prepare          # noqa: E402
from fujiyama_renderer_amd import gpu, workloads                              # noqa: E402

FLOORS = (1e-4, 1e-3, 1e-2, 1e-1)


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
    kw = dict(iterations=gpu.DENOISE_ITERATIONS, sigma_color=gpu.SIGMA_COLOR, sigma_normal=gpu.SIGMA_NORMAL,
              sigma_position=gpu.SIGMA_POSITION_FRACTION * diag, stop_at_ids=True)
    sid = ids[:, :, 3]
    has_dmap = np.array([s["diffuse_map"] >= 0 for s in tab.shaders] + [False])
    has_map = np.array([tab.map_of(k) >= 0 for k in range(len(tab.shaders))] + [False])
    masks = [("all pixels", np.ones(fg.shape, dtype=bool)), ("diffuse_map >= 0", has_dmap[sid]), ("any texture", has_map[sid])]
    truth64 = truth.astype(np.float64)
    mse = lambda a, m: float(np.mean((a.astype(np.float64)[m] - truth64[m]) ** 2)) if m.any() else float("nan")
    print("%s: %d x %d, %d foreground pixels, diagonal %.4f; pixels: %s" % (name, rd.xres, rd.yres, int(fg.sum()), diag,
          ", ".join("%s %d" % (n, int(m.sum())) for n, m in masks)))
    print("    %-26s %s" % ("", "  ".join("%-18s" % n for n, _ in masks)))
    rows = [("noisy 2 x 2", noisy), ("plain denoise", dm.denoise(noisy, normal, position, ids, **kw))]
    for f in FLOORS:
        rows.append(("demodulated, floor %g" % f, am.demodulated_denoise(noisy, normal, position, ids, albedo=alb, albedo_floor=f, **kw)))
    for label, frame in rows:
        print("    %-26s %s" % (label, "  ".join("%-18.9f" % mse(frame, m) for _, m in masks)))


if __name__ == "__main__":
    asset = workloads.default_asset_dir()
    experiment("textures_diffuse_and_bump", lambda spp: edge_scenes.custom_scene(asset, **dict(edge_scenes.EDGE_CASES["textures_diffuse_and_bump"], spp=spp)))
    experiment("cornell", lambda spp: workloads.cornell(asset, res=(64, 48), spp=spp, mesh="tiny"))
