#!/usr/bin/env python3
"""The experiment behind gpu.ALPHA_MIN, gpu.COS_NORMAL and gpu.TOL_POSITION_FRACTION (profiles/temporal_pass.txt, section 1), CPU only, run
the way scripts/denoise_variance_grid.py is: oracle frames of the 64 x 48 Cornell box at 2 x 2 spp from six cameras of a sideways
sub-pixel pan, their AOVs and albedo from the oracle's trace of the tiles' camera rays, a 12 x 12 spp frame of the LAST camera as the
truth.  Every frame goes through tests/temporal_model.py against the frame before (the spatial fallback: tests/denoise_variance_model.py's
estimate of the demodulated frame), the last accumulated frame through denoise_variance_model.denoise_variance with the temporal variance
at the shipped sigmas.  Printed: the mean squared error over all four channels of that against the truth, beside the last frame alone
through the variance-guided filter (what Scene.render_denoised(variance_guided=True, demodulate=True) computes), and the share of
foreground pixels whose history is at least 2 frames long.

    python scripts/temporal_grid.py [step in world units, default 0.012]
"""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import albedo_model as am                   # noqa: E402
import denoise_variance_model as dvm        # noqa: E402
import oracle_ffi                           # noqa: E402
import temporal_model as tm                 # noqa: E402
from test_gpu_aov import SceneView, all_tiles, expected_aov, prepare          # noqa: E402
from fujiyama_renderer_amd import ffi, gpu, workloads                         # noqa: E402

FRAMES = 6
ALPHA_MIN = (0.05, 0.1, 0.2, 0.4)
COS_NORMAL = (0.8, 0.9, 0.97)
TOL_X = (0.005, 0.01, 0.02, 0.05)      # fractions of the diagonal of the foreground's bounding box
CAMERA_LINE = re.compile(r"^SetSampleProperty3 cam1 translate 0 0\.5 1\.85 0$", re.M)


class SceneDescHead(C.Structure):       # fj_scene_desc, include/fj_scene_desc.h
    _fields_ = [("n", C.c_int32 * 7), ("target_group", C.c_int32), ("arrays", C.c_void_p * 7), ("camera", ffi.CameraDesc)]


def host_view(sp, rd):
    """fjgpu_scene_view without a device: the same host functions (include/fjgpu.h: diagnostics)"""
    L = gpu.lib()
    L.fjgpu_host_make_transform.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fjgpu_host_make_transform.restype = None
    L.fjgpu_host_camera_uv_size_y.argtypes = [C.c_double]
    L.fjgpu_host_camera_uv_size_y.restype = C.c_double
    cam = C.cast(sp, C.POINTER(SceneDescHead)).contents.camera
    x = cam.xform
    assert x.n_translate == x.n_rotate == x.n_scale == 1
    trs = np.array(list(x.translate[0].v) + list(x.rotate[0].v) + list(x.scale[0].v), dtype=np.float64)
    M, Minv = np.zeros(16), np.zeros(16)
    L.fjgpu_host_make_transform(x.transform_order, x.rotate_order, trs.ctypes.data, M.ctypes.data, Minv.ctypes.data)
    uvy = L.fjgpu_host_camera_uv_size_y(cam.fov)
    return tm.View(Minv[:12], (uvy * (rd.xres / float(rd.yres)), uvy), rd.xres, rd.yres)


def cornell(asset, spp, dx):
    text = workloads.cornell(asset, res=(64, 48), spp=spp, mesh="tiny")
    assert len(CAMERA_LINE.findall(text)) == 1
    return CAMERA_LINE.sub("SetSampleProperty3 cam1 translate %.17g 0.5 1.85 0" % dx, text)


def frames_of_the_pan(asset, step):
    out = []
    for k in range(FRAMES):
        sp, rd = prepare(cornell(asset, (2, 2), k * step))
        view, tab = SceneView(sp), am.Tables(sp)
        osc = oracle_ffi.OracleScene(sp)
        noisy, _ = osc.render(rd)
        src = am.OracleSamples(sp)
        aov, _, _ = expected_aov(src, osc, view, rd, all_tiles(rd))
        alb = am.expected_albedo(src, osc, view, tab, rd, all_tiles(rd))["albedo"]
        osc.close()
        out.append(dict(color=noisy, normal=aov["normal"].astype(np.float32), position=aov["position"].astype(np.float32), ids=aov["ids"],
                        albedo=alb.astype(np.float32), view=host_view(sp, rd)))
    sp, rd = prepare(cornell(asset, (12, 12), (FRAMES - 1) * step))
    osc = oracle_ffi.OracleScene(sp)
    truth, _ = osc.render(rd)
    osc.close()
    return out, truth


def pipeline(frames, diag, alpha_min, cos_normal, tol_fraction, max_history=gpu.MAX_HISTORY, demodulate=True):
    """-> (the last frame's result, its history length, the accumulated frame the filter read)"""
    sx = gpu.SIGMA_POSITION_FRACTION_VARIANCE * diag
    hist, prev = None, None
    for f in frames:
        alb = f["albedo"] if demodulate else None
        D = am.demodulate(f["color"], alb, gpu.ALBEDO_FLOOR)[0] if demodulate else f["color"]
        vs = dvm.estimate_variance(D, f["normal"], f["position"], f["ids"], sigma_normal=gpu.SIGMA_NORMAL, sigma_position=sx)
        hist, var = tm.accumulate(f["color"], f["position"], f["normal"], f["ids"], albedo=alb, variance_spatial=vs,
                                  prev_view=prev["view"] if prev else None, prev_position=prev["position"] if prev else None,
                                  prev_normal=prev["normal"] if prev else None, prev_ids=prev["ids"] if prev else None, prev=hist,
                                  alpha_min=alpha_min, max_history=max_history, tol_position=tol_fraction * diag, cos_normal=cos_normal,
                                  min_history_variance=gpu.MIN_HISTORY_VARIANCE, albedo_floor=gpu.ALBEDO_FLOOR)
        prev = f
    f = frames[-1]
    out, _ = dvm.denoise_variance(hist["color"], f["normal"], f["position"], f["ids"], albedo=alb, albedo_floor=gpu.ALBEDO_FLOOR,
                                  variance=var, iterations=gpu.DENOISE_ITERATIONS, sigma_luminance=gpu.SIGMA_LUMINANCE,
                                  sigma_normal=gpu.SIGMA_NORMAL, sigma_position=sx, stop_at_ids=True)
    return out, hist["length"], hist["color"]


if __name__ == "__main__":
    step = float(sys.argv[1]) if len(sys.argv) > 1 else 0.012
    frames, truth = frames_of_the_pan(workloads.default_asset_dir(), step)
    last = frames[-1]
    fg = last["ids"][:, :, 0] >= 0
    p = frames[0]["position"][frames[0]["ids"][:, :, 0] >= 0].astype(np.float64)
    diag = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    truth64 = truth.astype(np.float64)
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth64) ** 2))
    print("cornell 64 x 48, %d frames, camera x += %g per frame, %d foreground pixels in the last frame, diagonal %.4f (of the first)"
          % (FRAMES, step, int(fg.sum()), diag))
    print("    noisy 2 x 2, last frame                                  %.6f" % mse(last["color"]))
    for demodulate in (True, False):
        alb = last["albedo"] if demodulate else None
        single, _ = dvm.denoise_variance(last["color"], last["normal"], last["position"], last["ids"], albedo=alb,
                                         albedo_floor=gpu.ALBEDO_FLOOR, iterations=gpu.DENOISE_ITERATIONS, sigma_luminance=gpu.SIGMA_LUMINANCE,
                                         sigma_normal=gpu.SIGMA_NORMAL, sigma_position=gpu.SIGMA_POSITION_FRACTION_VARIANCE * diag, stop_at_ids=True)
        print("  %s" % ("demodulated (floor %g)" % gpu.ALBEDO_FLOOR if demodulate else "not demodulated"))
        print("    last frame alone, variance-guided (shipped sigmas)       %.6f" % mse(single))
        best = None
        print("    temporal + variance-guided, max_history %g, min_history_variance %g: MSE (share of foreground with history >= 2)"
              % (gpu.MAX_HISTORY, gpu.MIN_HISTORY_VARIANCE))
        print("        alpha_min  cos_normal   tol_position = " + "            ".join("%g d" % f for f in TOL_X))
        for am_ in ALPHA_MIN:
            for cn in COS_NORMAL:
                row = []
                for tx in TOL_X:
                    out, length, acc = pipeline(frames, diag, am_, cn, tx, demodulate=demodulate)
                    share = float((length[fg] >= 2).mean())
                    row.append((mse(out), share, mse(acc)))
                    if share >= 0.9 and (best is None or row[-1][0] < best[0]):
                        best = (row[-1][0], am_, cn, tx, share, row[-1][2])
                print("        %-9g  %-9g  %s" % (am_, cn, "  ".join("%.6f (%.3f)" % (a, b) for a, b, _ in row)))
        print("        best with history >= 2 on 90 %% of the foreground: %.6f at alpha_min %g, cos_normal %g, tol_position %g d (share %.3f; "
              "the accumulated frame before the filter: %.6f)" % best)
        out, length, acc = pipeline(frames, diag, gpu.ALPHA_MIN, gpu.COS_NORMAL, gpu.TOL_POSITION_FRACTION, demodulate=demodulate)
        print("        shipped (alpha_min %g, cos_normal %g, tol_position %g d): %.6f, history >= 2 on %.3f of the foreground, accumulated frame %.6f"
              % (gpu.ALPHA_MIN, gpu.COS_NORMAL, gpu.TOL_POSITION_FRACTION, mse(out), float((length[fg] >= 2).mean()), mse(acc)))
        sys.stdout.flush()
