#!/usr/bin/env python3
"""The experiment behind gpu.CLAMP_RADIUS, gpu.CLAMP_GAMMA and gpu.CLAMP_STOP_AT_IDS (profiles/temporal_clamp.txt), CPU only, run the way
scripts/temporal_grid.py is and on its frames: the oracle's 64 x 48 Cornell box at 2 x 2 spp from six cameras of the sideways sub-pixel
pan, a 12 x 12 spp frame of the last camera as the truth, the shipped temporal settings (gpu.ALPHA_MIN, gpu.COS_NORMAL,
gpu.TOL_POSITION_FRACTION).  Every frame goes through tests/temporal_clamp_model.py against the frame before, the last accumulated frame
through the variance-guided filter with the temporal variance.  Printed per cell of radius x gamma x stop_at_ids, demodulated and not: the
mean squared error of the accumulated frame and of the filtered result, beside the unclamped chain and the last frame filtered alone.  The
constants are the cell with the smallest filtered error of the chain that is NOT demodulated.

    python scripts/temporal_clamp_grid.py [step in world units, default 0.012]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import albedo_model as am                   # noqa: E402
import denoise_variance_model as dvm        # noqa: E402
import temporal_clamp_model as tcm          # noqa: E402
from temporal_grid import frames_of_the_pan                    # noqa: E402
from fujiyama_renderer_amd import gpu, workloads                # noqa: E402

RADIUS = (1, 2, 3)
GAMMA = (0.75, 1.0, 1.5, 2.0)
STOP = (0, 1)


def pipeline(frames, diag, clamp, demodulate):
    """-> (the last frame's filtered result, the accumulated frame the filter read, the share of its foreground the clamp moved)"""
    sx = gpu.SIGMA_POSITION_FRACTION_VARIANCE * diag
    hist, prev = None, None
    for f in frames:
        alb = f["albedo"] if demodulate else None
        D = am.demodulate(f["color"], alb, gpu.ALBEDO_FLOOR)[0] if demodulate else f["color"]
        vs = dvm.estimate_variance(D, f["normal"], f["position"], f["ids"], sigma_normal=gpu.SIGMA_NORMAL, sigma_position=sx)
        hist, var, amount = tcm.accumulate(f["color"], f["position"], f["normal"], f["ids"], albedo=alb, variance_spatial=vs,
                                           prev_view=prev["view"] if prev else None, prev_position=prev["position"] if prev else None,
                                           prev_normal=prev["normal"] if prev else None, prev_ids=prev["ids"] if prev else None, prev=hist,
                                           alpha_min=gpu.ALPHA_MIN, max_history=gpu.MAX_HISTORY, tol_position=gpu.TOL_POSITION_FRACTION * diag,
                                           cos_normal=gpu.COS_NORMAL, min_history_variance=gpu.MIN_HISTORY_VARIANCE,
                                           albedo_floor=gpu.ALBEDO_FLOOR, clamp=clamp)
        prev = f
    f = frames[-1]
    out, _ = dvm.denoise_variance(hist["color"], f["normal"], f["position"], f["ids"], albedo=alb, albedo_floor=gpu.ALBEDO_FLOOR,
                                  variance=var, iterations=gpu.DENOISE_ITERATIONS, sigma_luminance=gpu.SIGMA_LUMINANCE,
                                  sigma_normal=gpu.SIGMA_NORMAL, sigma_position=sx, stop_at_ids=True)
    fg = f["ids"][:, :, 0] >= 0
    return out, hist["color"], float((amount[fg] > 0).mean())


if __name__ == "__main__":
    step = float(sys.argv[1]) if len(sys.argv) > 1 else 0.012
    frames, truth = frames_of_the_pan(workloads.default_asset_dir(), step)
    last = frames[-1]
    p = frames[0]["position"][frames[0]["ids"][:, :, 0] >= 0].astype(np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    truth64 = truth.astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth64) ** 2))
    print("cornell 64 x 48, %d frames, camera x += %g per frame; alpha_min %g, cos_normal %g, tol_position %g d, max_history %g"
          % (len(frames), step, gpu.ALPHA_MIN, gpu.COS_NORMAL, gpu.TOL_POSITION_FRACTION, gpu.MAX_HISTORY))
    print("    noisy 2 x 2, last frame                                  %.6f" % mse(last["color"]))
    for demodulate in (False, True):
        alb = last["albedo"] if demodulate else None
        single, _ = dvm.denoise_variance(last["color"], last["normal"], last["position"], last["ids"], albedo=alb,
                                         albedo_floor=gpu.ALBEDO_FLOOR, iterations=gpu.DENOISE_ITERATIONS, sigma_luminance=gpu.SIGMA_LUMINANCE,
                                         sigma_normal=gpu.SIGMA_NORMAL, sigma_position=gpu.SIGMA_POSITION_FRACTION_VARIANCE * diag, stop_at_ids=True)
        print("  %s" % ("demodulated (floor %g)" % gpu.ALBEDO_FLOOR if demodulate else "not demodulated"))
        print("    last frame alone, variance-guided (shipped sigmas)       %.6f" % mse(single))
        out, acc, _ = pipeline(frames, diag, None, demodulate)
        print("    unclamped chain: accumulated %.6f, filtered %.6f" % (mse(acc), mse(out)))
        print("    clamped chain: accumulated / filtered MSE (share of the last frame's foreground the clamp moved)")
        print("        radius  stop_at_ids   gamma = " + "                        ".join("%g" % g for g in GAMMA))
        best = None
        for radius in RADIUS:
            for stop in STOP:
                row = []
                for gamma in GAMMA:
                    out, acc, share = pipeline(frames, diag, (radius, gamma, stop), demodulate)
                    row.append((mse(acc), mse(out), share))
                    if best is None or row[-1][1] < best[0]:
                        best = (row[-1][1], radius, gamma, stop, row[-1][0])
                print("        %-6d  %-11d  %s" % (radius, stop, "  ".join("%.6f / %.6f (%.3f)" % r for r in row)))
                sys.stdout.flush()
        print("        smallest filtered error: %.6f at radius %d, gamma %g, stop_at_ids %d (accumulated %.6f); the last frame alone: %.6f -- %s"
              % (best + (mse(single), "the chain is BELOW the single frame" if best[0] < mse(single) else "NO cell brings the chain below the single frame")))
        if not demodulate:
            print("        -> gpu.CLAMP_RADIUS = %d, gpu.CLAMP_GAMMA = %g, gpu.CLAMP_STOP_AT_IDS = %s" % (best[1], best[2], bool(best[3])))
