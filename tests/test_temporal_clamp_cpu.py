"""fjgpu_denoise_temporal_clamped without a GPU (include/fjgpu.h): the C ABI's layout and refusals, and the arithmetic through its host twin.

lib/libfj_temporal_host.so (csrc/tools/temporal_host.cc: fj_denoise_temporal_clamped_host) calls fj_tp_pixel_clamped of
csrc/device/fjgpu_temporal_math.h -- the function the kernels k_tp_accumulate_clamped<R> call -- for every region pixel of host arrays;
tests/temporal_clamp_model.py is the numpy restatement written from the header's text.  Scene, cases and tolerance are those of
tests/test_temporal_cpu.py (tests/temporal_clamp_cases.py): REL_TOL = 1e-4 with denoise_model.rel_err, the history length exact.  The clamp is
continuous in its inputs, so a comparison that falls the other way in twin and model costs an ulp, not a pixel.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import temporal_clamp_cases as tc
import temporal_model as tm
import temporal_scene as ts
from fujiyama_renderer_amd import ffi, gpu
from test_temporal_cpu import _p, c_desc, c_history, c_view, run_twin as run_twin_unclamped, twin as _twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, REGION = ts.W, ts.H, ts.REGION


def twin():
    t = _twin()
    t.fj_denoise_temporal_clamped_host.argtypes = [C.POINTER(ffi.TemporalDesc), C.POINTER(ffi.TemporalClamp)] + [C.c_void_p] * 6 + \
        [C.POINTER(ffi.View)] + [C.c_void_p] * 3 + [C.POINTER(ffi.TemporalHistory)] * 2 + [C.c_void_p]
    return t


def run_twin(cur, prev, prev_hist, albedo, vs, out=None, var_out=None, clamp=None, amount=None, **params):
    h, w = cur["color"].shape[:2]
    d = c_desc(REGION, w, h, **params)
    out = tm.new_history(h, w) if out is None else out
    var_out = np.zeros((h, w), dtype=np.float32) if var_out is None else var_out
    amount = np.zeros((h, w), dtype=np.float32) if amount is None else amount
    cl = None
    if clamp is not None:
        cl = ffi.TemporalClamp()
        cl.radius, cl.gamma, cl.stop_at_ids = clamp
        cl.amount = amount.ctypes.data
    hn = c_history(out)
    hp = C.byref(c_history(prev_hist)) if prev_hist is not None else None
    rc = twin().fj_denoise_temporal_clamped_host(C.byref(d), C.byref(cl) if cl is not None else None, _p(cur["color"]), _p(cur["position"]),
                                                 _p(cur["normal"]), _p(cur["ids"]), _p(cur["albedo"]) if albedo else None, _p(vs),
                                                 C.byref(c_view(prev["view"])) if prev else None, _p(prev["position"]) if prev else None,
                                                 _p(prev["normal"]) if prev else None, _p(prev["ids"]) if prev else None, hp, C.byref(hn),
                                                 _p(var_out))
    assert rc == 0, rc
    return out, var_out, amount


def test_layout():
    assert twin().fj_temporal_host_sizeof(b"fjgpu_temporal_clamp") == C.sizeof(ffi.TemporalClamp) == 24
    text = open(os.path.join(ROOT, "include", "fjgpu.h")).read()
    assert "} fjgpu_temporal_clamp;" in text and "int fjgpu_denoise_temporal_clamped(" in text
    L = gpu.lib()
    assert len(L.fjgpu_denoise_temporal_clamped.argtypes) == 18 and len(L.fjgpu_denoise_temporal.argtypes) == 17
    assert C.sizeof(ffi.TemporalDesc) == 48
    assert gpu.CLAMP_RADIUS in (1, 2, 3) and gpu.CLAMP_GAMMA > 0 and gpu.CLAMP_STOP_AT_IDS in (True, False)


@pytest.mark.parametrize("radius,albedo,stop", tc.CASES, ids=tc.CASE_IDS)
def test_twin_equals_model(radius, albedo, stop):
    tc.check_equal_to_model(run_twin, radius, albedo, stop, "twin r%d %s %s" % (radius, "albedo" if albedo else "plain", "stop" if stop else "nostop"))


def test_null_clamp_is_the_unclamped_twin():
    hist_a, hist_b, prev = None, None, None
    for k, cur in enumerate(ts.pan_sequence()):
        vs = ts.spatial_variance(k)
        hist_a, var_a = run_twin_unclamped(cur, prev, hist_a, True, vs)
        hist_b, var_b, amt = run_twin(cur, prev, hist_b, True, vs, clamp=None, **ts.PARAMS)
        for name in hist_a:
            assert np.array_equal(hist_a[name], hist_b[name]), (k, name)
        assert np.array_equal(var_a, var_b) and not amt.any()
        prev = cur


def test_huge_gamma_is_no_clamp():
    """gamma = 1e30, radius 1, the noisy pan: the box holds every history, so rgb, alpha and moments of foreground pixels are the
    unclamped result bit for bit and amount is 0 there"""
    hist_a, hist_b, prev = None, None, None
    for k, cur in enumerate(ts.pan_sequence()):
        hist_a, _ = run_twin_unclamped(cur, prev, hist_a, False, None)
        hist_b, _, amt = run_twin(cur, prev, hist_b, False, None, clamp=(1, 1e30, 0), **ts.PARAMS)
        fg = ts.inside() & (cur["ids"][..., 0] >= 0)
        assert np.array_equal(hist_a["color"][fg], hist_b["color"][fg]) and np.array_equal(hist_a["moments"][fg], hist_b["moments"][fg]), k
        assert np.array_equal(hist_a["length"], hist_b["length"]) and (amt[fg] == 0).all()
        prev = cur
    assert (hist_b["length"][fg] >= 2).mean() > 0.8


@pytest.mark.parametrize("radius,stop", [(1, 0), (3, 1)])
def test_bound_by_construction(radius, stop):
    """for every pixel with history and every colour channel |O - m| <= (1 - alpha) gamma sd + alpha |C - m| + 1e-5 (1 + |m|): the clipped
    history is within gamma sd of m and the blend is a convex combination; m, sd from the model's window, alpha from the output length"""
    gamma = 0.75
    frames = ts.pan_sequence()
    hist, prev = None, None
    x0, y0, x1, y1 = REGION
    for k, cur in enumerate(frames):
        new, _, _ = run_twin(cur, prev, hist, False, None, clamp=(radius, gamma, stop), **ts.PARAMS)
        det = {}
        tc.model_run(cur, prev, hist, False, None, clamp=(radius, gamma, stop), details=det, **ts.PARAMS)
        have = det["have"]
        if k:
            assert have.sum() > 300
        n = new["length"][y0:y1, x0:x1].astype(np.float64)
        alpha = np.maximum(1.0 / n, ts.PARAMS["alpha_min"])[..., None]
        m, sd = det["m"][..., :4].astype(np.float64), det["sd"][..., :4].astype(np.float64)
        O = new["color"][y0:y1, x0:x1].astype(np.float64)
        Cc = cur["color"][y0:y1, x0:x1].astype(np.float64)
        slack = (1 - alpha) * gamma * sd + alpha * np.abs(Cc - m) + 1e-5 * (1 + np.abs(m)) - np.abs(O - m)
        assert (slack[have] >= 0).all(), (k, float(slack[have].min()))
        hist, prev = new, cur


def test_ghost():
    """the sphere's radiance drops to 0.3 of its value at frame 4 while every guide stays put: the clamp (radius 1, gamma 1, no id stop)
    brings the sphere's error to at most 0.5 of the unclamped pass's and leaves the ground's within 1.05 of it"""
    sphere, ground, share = tc.ghost(run_twin)
    print("ghost ratios (twin): sphere %.4f, ground %.4f" % (sphere, ground))
    msphere, mground, _ = tc.ghost(tc.model_run)
    print("ghost ratios (model): sphere %.4f, ground %.4f" % (msphere, mground))
    assert sphere <= 0.5 and ground <= 1.05 and share > 0.5
    assert abs(sphere - msphere) <= 1e-3 and abs(ground - mground) <= 1e-3


def test_untouched_and_unread():
    tc.check_untouched_and_unread(run_twin)


# ---- refusals: one child process that sees no device
OLD = "next_color_is_color"            # the unclamped entry's LAST refusal, the overlap of its buffers: the clamp's come after it
CLAMP_DEFECTS = {
    "radius_0": "radius", "radius_4": "radius", "radius_negative": "radius", "gamma_nan": "gamma", "gamma_inf": "gamma", "gamma_0": "gamma",
    "gamma_negative": "gamma", "amount_is_color": "amount", "amount_in_ids": "amount", "amount_is_prev_length": "amount",
    "amount_is_next_moments": "amount", "amount_is_variance_out": "amount", "amount_is_albedo": "amount",
}

_CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %r)
from fujiyama_renderer_amd import ffi, gpu
assert gpu.device_count() == 0, "a device is visible"
L = gpu.lib()
F = [4096 * k for k in range(1, 24)]
out = {}
for case in %r:
    d = ffi.TemporalDesc(); d.xres, d.yres = 16, 8; d.region[:] = (0, 0, 16, 8)
    d.alpha_min, d.max_history, d.tol_position, d.cos_normal, d.min_history_variance, d.albedo_floor = 0.1, 8.0, 0.5, 0.9, 4.0, 1e-4
    a = dict(color=F[0], position=F[1], normal=F[2], ids=F[3], albedo=F[14], vs=None, pp=F[4], pn=F[5], pi=F[6], vout=F[7])
    view = ffi.View(); view.xres, view.yres = 16, 8; view.uv_size[:] = (1.0, 0.5)
    prev = ffi.TemporalHistory(); prev.color, prev.moments, prev.length = F[8], F[9], F[10]
    nxt = ffi.TemporalHistory(); nxt.color, nxt.moments, nxt.length = F[11], F[12], F[13]
    cl = ffi.TemporalClamp(); cl.radius, cl.gamma, cl.stop_at_ids, cl.amount = 2, 1.0, 1, F[16]
    cp = C.byref(cl)
    for part in case.split("+"):
        if part == "radius_0": cl.radius = 0
        elif part == "radius_4": cl.radius = 4
        elif part == "radius_negative": cl.radius = -1
        elif part == "gamma_nan": cl.gamma = float("nan")
        elif part == "gamma_inf": cl.gamma = float("inf")
        elif part == "gamma_0": cl.gamma = 0.0
        elif part == "gamma_negative": cl.gamma = -1.0
        elif part == "amount_is_color": cl.amount = F[0]
        elif part == "amount_in_ids": cl.amount = F[3] + 1024
        elif part == "amount_is_prev_length": cl.amount = F[10]
        elif part == "amount_is_next_moments": cl.amount = F[12]
        elif part == "amount_is_variance_out": cl.amount = F[7]
        elif part == "amount_is_albedo": cl.amount = F[14]
        elif part == "next_color_is_color": nxt.color = F[0]
        elif part == "alpha_0": d.alpha_min = 0.0
        elif part == "null_clamp": cp = None
        elif part == "null_amount": cl.amount = None
        elif part == "valid": pass
        else: raise SystemExit("unknown case " + part)
    rc = L.fjgpu_denoise_temporal_clamped(0, C.byref(d), cp, a["color"], a["position"], a["normal"], a["ids"], a["albedo"], a["vs"], C.byref(view),
                                          a["pp"], a["pn"], a["pi"], C.byref(prev), C.byref(nxt), a["vout"], None, None)
    out[case] = [rc, L.fjgpu_last_error().decode()]
print("RESULT " + json.dumps(out))
'''

CHILD_CASES = sorted(CLAMP_DEFECTS) + sorted(c + "+" + OLD for c in CLAMP_DEFECTS) + \
    ["valid", "null_clamp", "null_amount", OLD, "alpha_0", "alpha_0+radius_0", "null_clamp+radius_0"]
_refused = None


def refusals():
    """every case in ONE child process: a case that slipped through its refusal stops at the missing device and follows no address"""
    global _refused
    if _refused is None:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, CHILD_CASES)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        _refused = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    return _refused


@pytest.mark.parametrize("case", sorted(CLAMP_DEFECTS))
def test_refusals(case):
    rc, msg = refusals()[case]
    assert rc == -2 and msg.startswith("fjgpu_denoise_temporal_clamped:") and CLAMP_DEFECTS[case] in msg, (rc, msg)


@pytest.mark.parametrize("case", sorted(CLAMP_DEFECTS))
def test_refusals_come_after_the_unclamped_entrys(case):
    """paired with the unclamped entry's last refusal, that one answers -- with its text of tests/image_api_refusals.json under the new name"""
    table = json.load(open(os.path.join(ROOT, "tests", "image_api_refusals.json")))["fjgpu_denoise_temporal"]
    old_texts = {m for _, m in table.values()}
    rc, msg = refusals()[case + "+" + OLD]
    assert rc == -2 and msg == "fjgpu_denoise_temporal_clamped: an output buffer (next, variance_out) overlaps prev or an input", (rc, msg)
    assert msg.replace("fjgpu_denoise_temporal_clamped:", "fjgpu_denoise_temporal:") in old_texts
    assert refusals()[OLD][1] == msg
    rc, msg = refusals()["alpha_0+radius_0"]
    assert rc == -2 and msg == refusals()["alpha_0"][1] == "fjgpu_denoise_temporal_clamped: alpha_min must be in (0, 1]"


def test_valid_calls_without_a_device_are_enodev():
    for case in ("valid", "null_clamp", "null_amount", "null_clamp+radius_0"):
        rc, msg = refusals()[case]
        assert rc == -1 and msg == "fjgpu_denoise_temporal_clamped: no HIP device is visible", (case, rc, msg)
