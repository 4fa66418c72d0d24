"""fjgpu_denoise_temporal, fjgpu_scene_set_camera / get_camera / view and fjgpu_denoise_estimate_variance_albedo without a GPU
(include/fjgpu.h): the C ABI's layout and refusals, and the arithmetic through its host twin.

lib/libfj_temporal_host.so (csrc/tools/temporal_host.cc) calls fj_tp_pixel of csrc/device/fjgpu_temporal_math.h -- the function the kernel
k_tp_accumulate calls -- for every region pixel of host arrays; tests/temporal_model.py is the numpy restatement written from the header's
text.  The scene is analytic (tests/temporal_scene.py): exact position, normal and ids of a ground square and a sphere from cameras that
move sideways by a fraction of a pixel per frame, a colour that is a smooth function of the world position plus seeded noise.  Twin against
model: REL_TOL = 1e-4 with denoise_model.rel_err, the tolerance of the other denoise twins (there is no transcendental in this pass: the
two agree far better, the printed errors say how well); the history length -- which taps were valid -- must agree exactly.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_model as tm
import temporal_scene as ts
from fujiyama_renderer_amd import ffi, gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, REGION = ts.W, ts.H, ts.REGION

_twin = None


def twin():
    global _twin
    if _twin is None:
        _twin = ffi.load("libfj_temporal_host.so")
        _twin.fj_denoise_temporal_host.argtypes = [C.POINTER(ffi.TemporalDesc)] + [C.c_void_p] * 6 + [C.POINTER(ffi.View)] + [C.c_void_p] * 3 + \
            [C.POINTER(ffi.TemporalHistory)] * 2 + [C.c_void_p]
        _twin.fj_temporal_host_project.argtypes = [C.POINTER(ffi.View), C.c_float, C.c_float, C.c_float, C.POINTER(C.c_double)]
        _twin.fj_temporal_host_sizeof.argtypes = [C.c_char_p]
    return _twin


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def c_view(v):
    out = ffi.View()
    out.world_to_camera[:] = list(v.world_to_camera)
    out.uv_size[:] = list(v.uv_size)
    out.xres, out.yres = v.xres, v.yres
    return out


def c_desc(region=REGION, w=W, h=H, **params):
    d = ffi.TemporalDesc()
    d.xres, d.yres = w, h
    d.region[:] = region
    for k, v in dict(ts.PARAMS, **params).items():
        setattr(d, k, 0.0 if v is None else v)
    return d


def c_history(h):
    out = ffi.TemporalHistory()
    for k in ("color", "moments", "length"):
        setattr(out, k, h[k].ctypes.data)
    return out


def run_twin(cur, prev, prev_hist, albedo, vs, out=None, var_out=None, region=REGION, **params):
    h, w = cur["color"].shape[:2]
    d = c_desc(region, w, h, **params)
    out = tm.new_history(h, w) if out is None else out
    var_out = np.zeros((h, w), dtype=np.float32) if var_out is None else var_out
    hn = c_history(out)
    hp = C.byref(c_history(prev_hist)) if prev_hist is not None else None
    rc = twin().fj_denoise_temporal_host(C.byref(d), _p(cur["color"]), _p(cur["position"]), _p(cur["normal"]), _p(cur["ids"]),
                                         _p(cur["albedo"]) if albedo else None, _p(vs), C.byref(c_view(prev["view"])) if prev else None,
                                         _p(prev["position"]) if prev else None, _p(prev["normal"]) if prev else None,
                                         _p(prev["ids"]) if prev else None, hp, C.byref(hn), _p(var_out))
    assert rc == 0, rc
    return out, var_out


def test_symbols_and_layout():
    L = gpu.lib()
    for name, n in (("fjgpu_scene_get_camera", 2), ("fjgpu_scene_set_camera", 2), ("fjgpu_scene_view", 3), ("fjgpu_denoise_temporal", 17),
                    ("fjgpu_denoise_estimate_variance_albedo", 11)):
        assert len(getattr(L, name).argtypes) == n
    assert callable(gpu.temporal_accumulate) and callable(gpu.TemporalDenoiser) and gpu.MIN_HISTORY_VARIANCE == 4
    assert 0 < gpu.ALPHA_MIN <= 1 and gpu.MAX_HISTORY >= 1
    for name, t in (("fj_xform_sample", ffi.XformSample), ("fj_xform_desc", ffi.XformDesc), ("fj_camera_desc", ffi.CameraDesc),
                    ("fjgpu_view", ffi.View), ("fjgpu_temporal_history", ffi.TemporalHistory), ("fjgpu_temporal_desc", ffi.TemporalDesc)):
        assert twin().fj_temporal_host_sizeof(name.encode()) == C.sizeof(t), name
    assert C.sizeof(ffi.CameraDesc) == 816 and C.sizeof(ffi.View) == 120 and C.sizeof(ffi.TemporalDesc) == 48
    text = open(os.path.join(ROOT, "include", "fjgpu.h")).read()
    assert "no temporal reuse" not in text and "fjgpu_denoise_temporal(" in text


@pytest.mark.parametrize("albedo", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("spatial", [False, True], ids=["moments", "spatial"])
def test_twin_equals_model(albedo, spatial):
    ts.check_equal_to_model(run_twin, albedo, spatial, "twin %s %s" % ("albedo" if albedo else "plain", "spatial" if spatial else "moments"))


def test_twin_terms_off_and_nan_guides():
    """tol_position off (None -> 0, and +inf), cos_normal off: the terms compare nothing, so a NaN in the previous guides of an off term
    does not invalidate a tap; with the terms on it does"""
    f0, f1 = ts.pan_sequence(2)
    h0, _ = run_twin(f0, None, None, False, None)
    bad = dict(f0, position=f0["position"].copy(), normal=f0["normal"].copy())
    bad["position"][10:14] = np.nan
    bad["normal"][16:20] = np.nan
    for kw in (dict(tol_position=None, cos_normal=-1.0), dict(tol_position=float("inf"), cos_normal=-2.0), dict()):
        got, gv = run_twin(f1, bad, h0, False, None, **kw)
        ref, rv = ts.model_run(f1, bad, h0, False, None, **dict(ts.PARAMS, **kw))
        assert np.array_equal(got["length"], ref["length"]) and float(tm.rel_err(got["color"], ref["color"]).max()) <= ts.REL_TOL
    on, _ = run_twin(f1, bad, h0, False, None)
    off, _ = run_twin(f1, bad, h0, False, None, tol_position=None, cos_normal=-1.0)
    assert (off["length"] >= on["length"]).all() and (off["length"] > on["length"]).sum() > 20


def test_running_mean():
    """an identity move, alpha_min tiny: k frames give the running mean of their colours and length k, capped at max_history = 4.
    The projection of an f32 position misses its own pixel centre by at most 2^-23 |P| / (the pixel's footprint) of a pixel -- under 2e-5
    here --, which mixes that much of a neighbour in per frame; the noisy neighbours differ by less than 2: 6 frames stay within 3e-4."""
    frames = [ts.frame(noise=0.1, seed=7 + k) for k in range(6)]
    m = ts.inside() & (frames[0]["ids"][..., 0] >= 0)
    hist = None
    for k, cur in enumerate(frames):
        hist, var = run_twin(cur, frames[k - 1] if k else None, hist, False, None, alpha_min=1e-6, max_history=4.0, min_history_variance=0.0)
        # (the weighted mean of four equal lengths is that length up to an f32 rounding per tap and frame)
        assert float(np.abs(hist["length"][m] - min(k + 1, 4)).max()) <= 1e-5
        if k < 4:
            mean = np.mean([f["color"].astype(np.float64) for f in frames[:k + 1]], axis=0)
            err = float(np.abs(hist["color"][m] - mean[m]).max())
            print("running mean of %d frames: max abs err %.3e" % (k + 1, err))
            assert err <= 3e-4
            lum = [0.2126 * f["color"][..., 0].astype(np.float64) + 0.7152 * f["color"][..., 1] + 0.0722 * f["color"][..., 2] for f in frames[:k + 1]]
            pv = np.var(lum, axis=0)
            verr = float(np.abs(var[m] - pv[m]).max())
            print("             its luminance variance: max abs err %.3e" % verr)
            assert verr <= 1e-3
    assert (hist["length"][ts.inside() & ~m] == 1).all()


def _wall(eye_x):
    """a wall facing the camera at depth 4 in numbers that are exact in binary: uv_size = (W / 16, H / 16), so the point behind the centre
    of pixel (x, y) is ((x - 18) / 4 + eye_x, (14 - y) / 4, -4) and projects to (x + 4 eye_x, y) through the camera at the origin"""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    P = np.stack([(x - 18) * 0.25 + eye_x, (14 - y) * 0.25, np.full_like(x, -4.0)], axis=-1).astype(np.float32)
    view = tm.View([1, 0, 0, -eye_x, 0, 1, 0, 0, 0, 0, 1, 0], (W / 16.0, H / 16.0), W, H)
    rng = np.random.default_rng(int(eye_x * 100) + 3)
    N = np.zeros((H, W, 3), dtype=np.float32)
    N[..., 2] = 1
    return dict(view=view, position=P, normal=N, ids=np.zeros((H, W, 4), dtype=np.int32), color=rng.random((H, W, 4)).astype(np.float32),
                albedo=np.ones((H, W, 3), dtype=np.float32))


def test_exact_reprojection():
    """a move by exactly one pixel fetches the neighbour's history with weight 1: fx = x + 1 up to f64 rounding, so (a, b) are (0, 0) or
    (1 - 1e-16 -> 1.f, .) and one tap carries the whole weight; with length 1 there, n = 2, alpha = 1/2: C' = G + .5 (C - G), bit for bit"""
    a, b = _wall(0.0), _wall(0.25)
    assert np.array_equal(tm.project(a["view"], b["position"])[0].round(9), np.tile(np.arange(W) + 1.0, (H, 1)))
    g = tm.new_history(H, W)
    rng = np.random.default_rng(11)
    g["color"][:] = rng.random((H, W, 4))
    g["moments"][:] = rng.random((H, W, 2))
    g["length"][:] = 1
    got, _ = run_twin(b, a, g, False, None, alpha_min=1e-6, max_history=100.0, tol_position=1e-3, cos_normal=0.999)
    x0, y0, x1, y1 = REGION
    G = g["color"][y0:y1, x0 + 1:x1]
    want = G + np.float32(0.5) * (b["color"][y0:y1, x0:x1 - 1] - G)
    assert np.array_equal(got["color"][y0:y1, x0:x1 - 1], want)
    assert (got["length"][y0:y1, x0:x1 - 1] == 2).all()
    # the last column's neighbour is outside the region: no history
    assert (got["length"][y0:y1, x1 - 1] == 1).all() and np.array_equal(got["color"][y0:y1, x1 - 1], b["color"][y0:y1, x1 - 1])


def test_resets():
    """len = 1 and the current colour bit for bit: pixels disoccluded behind the sphere (a move of eight pixels at the sphere's distance,
    about three more than the ground behind it moves: every tap of their footprint in the previous frame shows the sphere), background
    pixels, pixels whose id changed"""
    f0 = ts.frame(noise=0.1, seed=1)
    f1 = ts.frame(dx=8 * ts.PIXEL_AT_SPHERE, noise=0.1, seed=2)
    h0, _ = run_twin(f0, None, None, True, None)
    got, var = run_twin(f1, f0, h0, True, None)
    m = ts.inside()
    fx, fy, ok = tm.project(f0["view"], f1["position"])
    qx, qy = np.floor(fx).astype(int), np.floor(fy).astype(int)
    sphere_behind = np.ones((H, W), dtype=bool)
    for j in range(2):
        for i in range(2):
            sphere_behind &= f0["ids"][np.clip(qy + j, 0, H - 1), np.clip(qx + i, 0, W - 1), 0] == 1
    disoccluded = m & (f1["ids"][..., 0] == 0) & ok & sphere_behind
    background = m & (f1["ids"][..., 0] < 0)
    print("resets: %d disoccluded, %d background pixels" % (disoccluded.sum(), background.sum()))
    assert disoccluded.sum() >= 5 and background.sum() >= 50
    for sel in (disoccluded, background):
        assert (got["length"][sel] == 1).all() and np.array_equal(got["color"][sel], f1["color"][sel]) and (var[sel] == 0).all()
    kept = m & (got["length"] > 1)
    assert kept.sum() > 300
    # a changed id: the sphere's pixels of the previous frame renumbered
    g0 = dict(f0, ids=np.where(f0["ids"] == 1, 5, f0["ids"]).astype(np.int32))
    got2, _ = run_twin(f1, g0, h0, True, None)
    on_sphere = m & (f1["ids"][..., 0] == 1)
    assert on_sphere.sum() >= 20 and (got["length"][on_sphere] > 1).sum() >= 20
    assert (got2["length"][on_sphere] == 1).all() and np.array_equal(got2["color"][on_sphere], f1["color"][on_sphere])
    ground = m & (f1["ids"][..., 0] == 0)
    assert np.array_equal(got2["color"][ground], got["color"][ground])


def test_pixels_outside_the_region_are_untouched():
    ts.check_untouched_and_unread(run_twin)


def test_converged_history():
    """noise-free colour under a sub-pixel move: what accumulates is the world-space function, up to the error of the bilinear fetches.  A
    frame of nothing but ground, four frames.  One fetch interpolates the previous accumulation, which is the function g on the previous
    pixel grid plus its error, so e_k <= e_(k-1) + b with b <= (max |g_xx| + max |g_yy|) / 8, the bilinear error on a unit cell; the second
    derivatives are measured as second differences of the noise-free frames, with a factor 1.5 for what lies between the grid points.
    Checked 7 pixels inside the region: a footprint cut by the region's border interpolates to first order, and what it gives travels
    less than 2 pixels per frame."""
    frames = [ts.frame(dx=k * 0.4 * ts.PIXEL_AT_SPHERE, tilt=-0.9, sphere=False) for k in range(4)]
    assert all((f["ids"][..., 0] == 0).all() for f in frames)
    d2 = 0.0
    for f in frames:
        c = f["clean"].astype(np.float64)
        d2 = max(d2, np.abs(c[:, 2:] - 2 * c[:, 1:-1] + c[:, :-2]).max() + np.abs(c[2:] - 2 * c[1:-1] + c[:-2]).max())
    b = 1.5 * d2 / 8
    hist = None
    for k, cur in enumerate(frames):
        hist, _ = run_twin(cur, frames[k - 1] if k else None, hist, False, None, alpha_min=1e-6, max_history=100.0)
    x0, y0, x1, y1 = REGION
    core = (slice(y0 + 7, y1 - 7), slice(x0 + 7, x1 - 7))
    assert float(np.abs(hist["length"][core] - 4).max()) <= 1e-5
    err = float(np.abs(hist["color"][core].astype(np.float64) - frames[-1]["clean"][core]).max())
    first_order = float(np.abs(frames[-1]["clean"][:, 1:].astype(np.float64) - frames[-1]["clean"][:, :-1]).max())
    print("converged history: max abs err %.3e, bound 3 b = %.3e (one-pixel colour step %.3e)" % (err, 3 * b, first_order))
    assert err <= 3 * b + 1e-5 and 3 * b < 0.25 * first_order


FAKE = [4096 * k for k in range(1, 20)]          # non-NULL, 16-byte aligned, 4 KiB apart: every refusal is decided before a pointer is followed

REFUSALS = {
    "null_desc": "null", "null_color": "null", "null_position": "guide", "null_normal": "guide", "null_ids": "guide", "null_next": "history",
    "null_next_member": "history", "null_prev_member": "history", "null_prev_view": "previous frame", "null_prev_ids": "previous frame",
    "region_empty": "region", "region_outside": "region", "region_negative": "region", "alpha_0": "alpha_min", "alpha_above_1": "alpha_min",
    "alpha_negative": "alpha_min", "max_history_0": "max_history", "nan_alpha": "NaN", "nan_max_history": "NaN", "nan_tol": "NaN",
    "nan_cos": "NaN", "nan_min_history": "NaN", "nan_floor": "NaN", "bad_floor": "albedo_floor", "next_is_prev": "overlap",
    "next_color_is_color": "overlap", "next_overlaps_prev": "overlap", "variance_out_is_spatial": "overlap", "next_members_equal": "overlap",
    "misaligned_color": "aligned", "misaligned_next": "aligned", "bad_view": "prev_view",
}

_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %r)
from fujiyama_renderer_amd import ffi, gpu
L = gpu.lib()
F = [4096 * k for k in range(1, 20)]
out = {}
for case in %r:
    d = ffi.TemporalDesc(); d.xres, d.yres = 16, 8; d.region[:] = (0, 0, 16, 8)
    d.alpha_min, d.max_history, d.tol_position, d.cos_normal, d.min_history_variance, d.albedo_floor = 0.1, 8.0, 0.5, 0.9, 4.0, 1e-4
    a = dict(color=F[0], position=F[1], normal=F[2], ids=F[3], albedo=None, vs=None, pp=F[4], pn=F[5], pi=F[6], vout=F[7])
    view = ffi.View(); view.xres, view.yres = 16, 8; view.uv_size[:] = (1.0, 0.5)
    prev = ffi.TemporalHistory(); prev.color, prev.moments, prev.length = F[8], F[9], F[10]
    nxt = ffi.TemporalHistory(); nxt.color, nxt.moments, nxt.length = F[11], F[12], F[13]
    dp, vp, pp, np_ = C.byref(d), C.byref(view), C.byref(prev), C.byref(nxt)
    if case == "null_desc": dp = None
    elif case in ("null_color", "null_position", "null_normal", "null_ids"): a[case[5:]] = None
    elif case == "null_next": np_ = None
    elif case == "null_next_member": nxt.moments = None
    elif case == "null_prev_member": prev.length = None
    elif case == "null_prev_view": vp = None
    elif case == "null_prev_ids": a["pi"] = None
    elif case.startswith("region"): d.region[:] = dict(region_empty=(4, 2, 4, 6), region_outside=(0, 0, 17, 8), region_negative=(0, -1, 16, 8))[case]
    elif case.startswith("alpha"): d.alpha_min = dict(alpha_0=0.0, alpha_above_1=1.5, alpha_negative=-0.5)[case]
    elif case == "max_history_0": d.max_history = 0.5
    elif case.startswith("nan"): setattr(d, dict(nan_alpha="alpha_min", nan_max_history="max_history", nan_tol="tol_position", nan_cos="cos_normal",
                                                 nan_min_history="min_history_variance", nan_floor="albedo_floor")[case], float("nan"))
    elif case == "bad_floor": a["albedo"] = F[14]; d.albedo_floor = 0.0
    elif case == "next_is_prev": nxt.color, nxt.moments, nxt.length = F[8], F[9], F[10]
    elif case == "next_color_is_color": nxt.color = F[0]
    elif case == "next_overlaps_prev": nxt.color = F[8] + 16
    elif case == "variance_out_is_spatial": a["vs"] = a["vout"] = F[15]
    elif case == "next_members_equal": nxt.moments = nxt.length
    elif case == "misaligned_color": a["color"] = F[0] + 4
    elif case == "misaligned_next": nxt.color = F[11] + 8
    elif case == "bad_view": view.xres = 0
    rc = L.fjgpu_denoise_temporal(0, dp, a["color"], a["position"], a["normal"], a["ids"], a["albedo"], a["vs"], vp, a["pp"], a["pn"], a["pi"], pp, np_,
                                  a["vout"], None, None)
    out[case] = [rc, L.fjgpu_last_error().decode()]
print("RESULT " + json.dumps(out))
'''

_refused = None


def refusals():
    """every case in ONE child process: a case that slipped through its refusal would follow addresses this process does not own"""
    global _refused
    if _refused is None:
        import json
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, sorted(REFUSALS))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        _refused = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    return _refused


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(case):
    rc, msg = refusals()[case]
    assert rc == -2, (rc, msg)                  # FJGPU_EINVAL
    assert msg.startswith("fjgpu_denoise_temporal:") and REFUSALS[case] in msg, msg


def test_valid_call_without_a_device_is_enodev():
    """the same child with a valid description: every argument check passes and the call stops at the missing device"""
    code = ("import ctypes as C, sys\nsys.path.insert(0, %r)\nfrom fujiyama_renderer_amd import ffi, gpu\n"
            "assert gpu.device_count() == 0, 'a device is visible'\nL = gpu.lib()\n"
            "d = ffi.TemporalDesc(); d.xres, d.yres = 16, 8; d.region[:] = (0, 0, 16, 8)\n"
            "d.alpha_min, d.max_history, d.tol_position, d.cos_normal, d.min_history_variance, d.albedo_floor = 0.1, 8.0, 0.5, 0.9, 4.0, 1e-4\n"
            "n = ffi.TemporalHistory(); n.color, n.moments, n.length = 4096, 8192, 12288\n"
            "rc = L.fjgpu_denoise_temporal(0, C.byref(d), 16384, 20480, 24576, 28672, None, None, None, None, None, None, None, C.byref(n), None, None, None)\n"
            "print('rc', rc, L.fjgpu_last_error().decode())\n"
            "dd = ffi.DenoiseDesc(); dd.xres, dd.yres = 16, 8; dd.region[:] = (0, 0, 16, 8); dd.sigma_normal = dd.sigma_position = 1.0\n"
            "rc = L.fjgpu_denoise_estimate_variance_albedo(0, C.byref(dd), 4096, None, None, None, 8192, 0.05, 12288, None, None)\n"
            "print('rc', rc, L.fjgpu_last_error().decode())\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "rc -1 fjgpu_denoise_temporal: no HIP device" in r.stdout and "rc -1 fjgpu_denoise_estimate_variance_albedo: no HIP device" in r.stdout, r.stdout


@pytest.mark.parametrize("case", ["bad_floor", "null_color", "null_out", "region", "out_is_albedo", "out_is_color"])
def test_estimate_variance_albedo_einval(case):
    d = ffi.DenoiseDesc()
    d.xres, d.yres = 16, 8
    d.region[:] = (0, 0, 16, 8)
    d.sigma_normal = d.sigma_position = 1.0
    color, albedo, floor, out, what = FAKE[0], FAKE[1], 0.05, FAKE[2], "null"
    if case == "bad_floor":
        floor, what = 0.0, "albedo_floor"
    elif case == "null_color":
        color = None
    elif case == "null_out":
        out = None
    elif case == "region":
        d.region[:] = (0, 0, 17, 8)
        what = "region"
    elif case == "out_is_albedo":
        out, what = albedo, "variance_out"
    else:
        out, what = color, "variance_out"
    rc = gpu.lib().fjgpu_denoise_estimate_variance_albedo(0, C.byref(d), color, None, None, None, albedo, floor, out, None, None)
    msg = gpu.lib().fjgpu_last_error().decode()
    assert rc == -2 and msg.startswith("fjgpu_denoise_estimate_variance_albedo:") and what in msg, (rc, msg)


def test_camera_entries_refuse_null():
    L = gpu.lib()
    cam, view, rd = ffi.CameraDesc(), ffi.View(), ffi.RenderDesc()
    for fn, args in (("fjgpu_scene_set_camera", (None, C.byref(cam))), ("fjgpu_scene_get_camera", (None, C.byref(cam))),
                     ("fjgpu_scene_view", (None, C.byref(rd), C.byref(view)))):
        rc = getattr(L, fn)(*args)
        msg = L.fjgpu_last_error().decode()
        assert rc == -2 and msg.startswith(fn + ":") and "null" in msg, (fn, rc, msg)


def test_projection_inverts_get_ray():
    """points along the rays through jittered (u, v), as Camera::GetRay forms them, come back to (u xres - .5, (1 - v) yres - .5) within 1e-9
    pixel; the twin's projection is the model's bit for bit"""
    rng = np.random.default_rng(2017)
    worst = 0.0
    for dx, pan in ((0.0, 0.0), (0.7, 0.3), (-2.0, -1.1)):
        M, view = ts.camera(dx, pan)
        u, v = rng.random(500), rng.random(500)
        eye, d = ts.rays(M, view, u, v)
        P = eye + (rng.random(500) * 50 + 0.01)[:, None] * d
        fx, fy, ok = tm.project(view, P)
        assert ok.all()
        worst = max(worst, float(np.abs(fx - (u * W - .5)).max()), float(np.abs(fy - ((1 - v) * H - .5)).max()))
        behind = eye - 3.0 * d
        assert not tm.project(view, behind)[2].any()
        cv, fxy = c_view(view), (C.c_double * 2)()
        P32 = P.astype(np.float32)
        mfx, mfy, _ = tm.project(view, P32)
        for k in range(0, 500, 25):
            assert twin().fj_temporal_host_project(C.byref(cv), P32[k, 0], P32[k, 1], P32[k, 2], fxy) == 1
            assert fxy[0] == mfx[k] and fxy[1] == mfy[k]
        assert twin().fj_temporal_host_project(C.byref(cv), *[float(x) for x in behind[0].astype(np.float32)], fxy) == 0
    print("projection against GetRay: max error %.3e pixel" % worst)
    assert worst <= 1e-9
