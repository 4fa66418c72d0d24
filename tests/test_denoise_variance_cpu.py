"""fjgpu_denoise_estimate_variance and fjgpu_denoise_variance without a GPU (include/fjgpu.h): the C ABI's refusals, and the arithmetic
through its host twin.

lib/libfj_denoise_variance_host.so (csrc/tools/denoise_variance_host.cc) runs plain loops over host arrays whose every tap goes through
csrc/device/fjgpu_denoise_var_math.h, the source k_dn_variance and k_dn_atrous_var compile; tests/denoise_variance_model.py is the numpy
restatement written from the header's text.  Twin against model: REL_TOL = 1e-4 with denoise_model.rel_err (denominator floored at 1e-3);
the two differ in expf (glibc against numpy, a few ulp) and in nothing else.  Every comparison prints the largest error it saw.

Bit tests.  With sigma_luminance = 0 the luminance term is |dl| * 0.f = +0, what d2c * 0.f is in fj_dn_tap: the colours are those of
fj_denoise_host at sigma_color = 0.  With every term off the weights are the B3-spline products, integers over 256; their squares are
integers over 65536 and sum to 4900 / 65536, and wsum is exactly 1: a constant power-of-two variance comes back as c * 4900 / 65536.
A constant image of powers of two comes back bit-identical (tests/test_denoise_cpu.py's argument; the luminance difference is exactly 0
whatever k_l is).  Its estimated variance is not exactly 0: m = s1 / s0 carries the roundings of 49 products, 98 additions and one
division, at most 150 * 2^-24 relative in all, so |l - m| <= 150 * 2^-24 L and V, a weighted mean of (l - m)^2, is at most its square.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_model as dm
import denoise_variance_model as dvm
from fujiyama_renderer_amd import ffi, gpu
from test_albedo_cpu import FLOOR, random_albedo
from test_denoise_cpu import PARAMETER_SETS, REGION, desc, random_inputs, run_twin

REL_TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUIDES = dict(sigma_normal=0.8, sigma_position=1.2)
SIGMA_L = 2.5

_twin = None


def twin():
    global _twin
    if _twin is None:
        _twin = ffi.load("libfj_denoise_variance_host.so")
        _twin.fj_denoise_estimate_variance_host.argtypes = [C.POINTER(ffi.DenoiseDesc)] + [C.c_void_p] * 5
        _twin.fj_denoise_variance_host.argtypes = [C.POINTER(ffi.DenoiseDesc), C.c_float] + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 3
        _twin.fj_denoise_variance_host_kl.argtypes = [C.c_float, C.c_float]
        _twin.fj_denoise_variance_host_kl.restype = C.c_float
    return _twin


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _desc(color, kw):
    kw = {k: v for k, v in kw.items() if k != "sigma_color"}          # ignored by both entries
    H, W = color.shape[:2]
    return desc(W, H, sigma_color=0.0, **kw)


def twin_estimate(color, normal=None, position=None, ids=None, out=None, **kw):
    d = _desc(color, kw)
    out = np.zeros(color.shape[:2], dtype=np.float32) if out is None else out
    assert twin().fj_denoise_estimate_variance_host(C.byref(d), _p(color), _p(normal), _p(position), _p(ids), _p(out)) == 0
    return out


def twin_filter(color, normal=None, position=None, ids=None, sigma_luminance=SIGMA_L, albedo=None, albedo_floor=FLOOR, variance=None,
                out=None, var_out=None, **kw):
    d = _desc(color, kw)
    out = color.copy() if out is None else out
    var_out = np.zeros(color.shape[:2], dtype=np.float32) if var_out is None else var_out
    assert twin().fj_denoise_variance_host(C.byref(d), sigma_luminance, _p(color), _p(normal), _p(position), _p(ids), _p(albedo), albedo_floor,
                                           _p(variance), _p(out), _p(var_out)) == 0
    return out, var_out


def model_kw(kw):
    """the parameters of a twin call as the model takes them"""
    return {k: (bool(v) if k == "stop_at_ids" else v) for k, v in kw.items() if k != "sigma_color"}


def check(got, ref, what):
    err = float(dm.rel_err(got, ref).max())
    print("denoise_variance twin %-46s max rel err %.3e" % (what, err))
    assert np.isfinite(got).all()
    assert err <= REL_TOL, (what, err)


def test_symbol_bindings_and_layout():
    L = gpu.lib()
    assert L.fjgpu_denoise_estimate_variance.argtypes is not None and len(L.fjgpu_denoise_estimate_variance.argtypes) == 9
    assert L.fjgpu_denoise_variance.argtypes is not None and len(L.fjgpu_denoise_variance.argtypes) == 14
    assert callable(gpu.estimate_variance) and callable(gpu.denoise_variance) and gpu.SIGMA_LUMINANCE > 0
    assert hasattr(twin(), "fj_denoise_variance_host") and hasattr(twin(), "fj_denoise_estimate_variance_host")
    assert C.sizeof(ffi.DenoiseDesc) == 44 and C.sizeof(ffi.GpuStats) == 208
    text = open(os.path.join(ROOT, "include", "fjgpu.h")).read()
    assert "no variance guidance" not in text and "fjgpu_denoise_variance(" in text and "fjgpu_denoise_estimate_variance(" in text


FAKE, FAKE2, FAKE3 = 4096, 8192, 12288          # non-NULL, 16-byte aligned addresses: every refusal is decided before a pointer is followed

FILTER_CASES = ["null_desc", "null_in", "null_out", "region_empty", "region_outside", "region_negative", "iterations_0", "iterations_9",
                "nan_luminance", "nan_normal", "nan_position", "nan_color", "vout_is_vin", "vout_is_cout", "vout_is_cin", "bad_floor"]


@pytest.mark.parametrize("case", FILTER_CASES)
def test_filter_einval(case):
    d = desc(64, 48)
    a = dict(sl=1.0, cin=FAKE, albedo=None, floor=0.0, vin=None, cout=FAKE, vout=None)
    what = "null"
    if case == "null_desc":
        d = None
    elif case == "null_in":
        a["cin"] = None
    elif case == "null_out":
        a["cout"] = None
    elif case.startswith("region"):
        d.region[:] = dict(region_empty=(10, 5, 10, 20), region_outside=(0, 0, 65, 48), region_negative=(-1, 0, 64, 48))[case]
        what = "region"
    elif case.startswith("iterations"):
        d.iterations = int(case[-1])
        what = "iterations"
    elif case == "nan_luminance":
        a["sl"] = float("nan")
        what = "sigma_luminance is NaN"
    elif case.startswith("nan"):
        setattr(d, "sigma_" + case[4:], float("nan"))
        what = "NaN"
    elif case == "vout_is_vin":
        a["vin"] = a["vout"] = FAKE2
        what = "variance_out"
    elif case == "vout_is_cout":
        a["cout"] = a["vout"] = FAKE3
        what = "variance_out"
    elif case == "vout_is_cin":
        a["vout"] = FAKE
        what = "variance_out"
    else:
        a["albedo"], a["floor"] = FAKE2, 0.0
        what = "albedo_floor"
    rc = gpu.lib().fjgpu_denoise_variance(0, None if d is None else C.byref(d), a["sl"], a["cin"], None, None, None, a["albedo"], a["floor"],
                                          a["vin"], a["cout"], a["vout"], None, None)
    msg = gpu.lib().fjgpu_last_error().decode()
    assert rc == -2, (rc, msg)                  # FJGPU_EINVAL
    assert msg.startswith("fjgpu_denoise_variance:") and what in msg, msg


@pytest.mark.parametrize("case", ["null_desc", "null_color", "null_out", "region_empty", "region_outside", "nan_normal", "nan_color", "out_is_color"])
def test_estimate_einval(case):
    d = desc(64, 48, iterations=0)              # iterations is not the estimate's business
    color, out = FAKE, FAKE2
    what = "null"
    if case == "null_desc":
        d = None
    elif case == "null_color":
        color = None
    elif case == "null_out":
        out = None
    elif case.startswith("region"):
        d.region[:] = dict(region_empty=(10, 5, 10, 20), region_outside=(0, 0, 65, 48))[case]
        what = "region"
    elif case.startswith("nan"):
        setattr(d, "sigma_" + case[4:], float("nan"))
        what = "NaN"
    else:
        out = color
        what = "variance_out"
    rc = gpu.lib().fjgpu_denoise_estimate_variance(0, None if d is None else C.byref(d), color, None, None, None, out, None, None)
    msg = gpu.lib().fjgpu_last_error().decode()
    assert rc == -2, (rc, msg)
    assert msg.startswith("fjgpu_denoise_estimate_variance:") and what in msg, msg


def test_valid_calls_without_a_device_are_enodev():
    """valid descriptions on a process that sees no device: FJGPU_ENODEV from both entries.  Run in a child whose HIP runtime is told to
    show none, and the child checks that before it passes addresses it does not own."""
    code = ("import ctypes as C, sys\n"
            "sys.path.insert(0, %r)\n"
            "from fujiyama_renderer_amd import ffi, gpu\n"
            "assert gpu.device_count() == 0, 'a device is visible'\n"
            "d = ffi.DenoiseDesc(); d.xres, d.yres = 64, 48; d.region[:] = (0, 0, 64, 48); d.iterations = 5\n"
            "d.sigma_color = d.sigma_normal = d.sigma_position = 1.0\n"
            "L = gpu.lib()\n"
            "rc = L.fjgpu_denoise_variance(0, C.byref(d), 4.0, 4096, None, None, None, None, 0.0, None, 4096, 8192, None, None)\n"
            "print('rc', rc, L.fjgpu_last_error().decode())\n"
            "rc = L.fjgpu_denoise_estimate_variance(0, C.byref(d), 4096, None, None, None, 8192, None, None)\n"
            "print('rc', rc, L.fjgpu_last_error().decode())\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "rc -1 fjgpu_denoise_variance:" in r.stdout and "rc -1 fjgpu_denoise_estimate_variance:" in r.stdout, r.stdout


def test_k_l_constant():
    for s, g in ((4.0, 0.25), (1.0, 0.0), (16.0, 3.7e-5), (0.5, 1e12)):
        assert twin().fj_denoise_variance_host_kl(s, g) == float(dvm.k_l(s, np.float32(g)))
    assert twin().fj_denoise_variance_host_kl(1.0, 0.0) == float(np.float32(1) / np.float32(1e-6))
    for s in (0.0, -1.0, float("inf")):
        assert twin().fj_denoise_variance_host_kl(s, 0.3) == 0.0


@pytest.mark.parametrize("stop", [0, 1])
def test_estimate_twin_equals_model(stop):
    color, normal, position, ids = random_inputs()
    got = twin_estimate(color, normal, position, ids, region=REGION, stop_at_ids=stop, **GUIDES)
    ref = dvm.estimate_variance(color, normal, position, ids, region=REGION, stop_at_ids=bool(stop), **GUIDES)
    check(got, ref, "estimate 67x21 region, stop %d" % stop)
    assert got[REGION[1]:REGION[3], REGION[0]:REGION[2]].min() > 0
    got = twin_estimate(color, None, None, None, stop_at_ids=stop)
    check(got, dvm.estimate_variance(color, stop_at_ids=bool(stop)), "estimate without guides, stop %d" % stop)


@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("supplied", [False, True], ids=["estimated", "supplied"])
def test_filter_twin_equals_model(iterations, supplied):
    """67 x 21 frame, region (3, 2, 61, 19): at spacing 16 most taps of the 58 x 17 region fall outside it"""
    color, normal, position, ids = random_inputs()
    variance = (np.random.default_rng(5).random(color.shape[:2]) * 0.5).astype(np.float32) if supplied else None
    got, var = twin_filter(color, normal, position, ids, variance=variance, region=REGION, iterations=iterations, **GUIDES)
    ref, ref_var = dvm.denoise_variance(color, normal, position, ids, variance=variance, region=REGION, iterations=iterations,
                                        sigma_luminance=SIGMA_L, **GUIDES)
    check(got, ref, "colour, %d iterations, %s" % (iterations, "supplied" if supplied else "estimated"))
    check(var, ref_var, "variance, %d iterations, %s" % (iterations, "supplied" if supplied else "estimated"))
    assert not np.array_equal(got, color) and var[REGION[1]:REGION[3], REGION[0]:REGION[2]].min() > 0


def test_filter_twin_equals_model_with_albedo():
    color, normal, position, ids = random_inputs()
    albedo = random_albedo()
    got, var = twin_filter(color, normal, position, ids, albedo=albedo, region=REGION, iterations=3, **GUIDES)
    ref, ref_var = dvm.denoise_variance(color, normal, position, ids, albedo=albedo, albedo_floor=FLOOR, region=REGION, iterations=3,
                                        sigma_luminance=SIGMA_L, **GUIDES)
    check(got, ref, "colour, demodulated")
    check(var, ref_var, "variance, demodulated")
    plain, _ = twin_filter(color, normal, position, ids, region=REGION, iterations=3, **GUIDES)
    assert not np.array_equal(plain, got)


def test_estimate_is_the_population_variance_when_the_guides_are_off():
    color, _, _, _ = random_inputs(W=37, H=13)
    got = twin_estimate(color, sigma_normal=0.0, sigma_position=0.0, stop_at_ids=0)
    l = 0.2126 * color[..., 0].astype(np.float64) + 0.7152 * color[..., 1].astype(np.float64) + 0.0722 * color[..., 2].astype(np.float64)
    ref = np.array([[l[y - 3:y + 4, x - 3:x + 4].var() for x in range(3, 34)] for y in range(3, 10)])
    err = float(dm.rel_err(got[3:10, 3:34].astype(np.float64), ref).max())
    print("estimate against the f64 7 x 7 population variance: max rel err %.3e" % err)
    assert err <= REL_TOL


@pytest.mark.parametrize("guides", [True, False])
@pytest.mark.parametrize("stop", [0, 1])
def test_sigma_luminance_0_is_the_plain_filter_bit_for_bit(guides, stop):
    color, normal, position, ids = random_inputs()
    g = (normal, position, ids) if guides else (None, None, None)
    for kw in (dict(iterations=1), dict(iterations=5, region=REGION)):
        got, _ = twin_filter(color, *g, sigma_luminance=0.0, stop_at_ids=stop, **kw, **GUIDES)
        ref = run_twin(color, *g, sigma_color=0.0, stop_at_ids=stop, **kw, **GUIDES)
        assert np.array_equal(got, ref)
        assert not np.array_equal(got, color)
        # ... which a luminance term that is on does not give
        on, _ = twin_filter(color, *g, sigma_luminance=1.0, stop_at_ids=stop, **kw, **GUIDES)
        assert not np.array_equal(on, ref)


@pytest.mark.parametrize("c", [1.0, 0.125, 64.0])
def test_variance_propagation_is_exact(c):
    color, _, _, _ = random_inputs(W=37, H=13)
    variance = np.full(color.shape[:2], c, dtype=np.float32)
    _, var = twin_filter(color, sigma_luminance=0.0, variance=variance, iterations=1, sigma_normal=0.0, sigma_position=0.0, stop_at_ids=0)
    assert (var[2:-2, 2:-2] == np.float32(c * 4900 / 65536)).all()
    assert (var[0, :] != np.float32(c * 4900 / 65536)).all()          # fewer taps at the border, renormalised


def _bound(rgb):
    L = 0.2126 * rgb[0] + 0.7152 * rgb[1] + 0.0722 * rgb[2]
    return (150 * 2.0 ** -24 * L) ** 2


@pytest.mark.parametrize("kw", PARAMETER_SETS)
def test_constant_image_is_a_fixed_point(kw):
    _, normal, position, ids = random_inputs()
    rgba = (0.25, 2.0, 0.0078125, 1.0)
    color = np.empty((21, 67, 4), dtype=np.float32)
    color[:] = rgba
    for guides in ((normal, position, ids), (None, None, None)):
        for sl in (gpu.SIGMA_LUMINANCE, 0.3):
            got, var = twin_filter(color, *guides, sigma_luminance=sl, **kw)
            assert np.array_equal(got, color)
            assert np.isfinite(var).all()
        est = twin_estimate(color, *guides, **{k: v for k, v in kw.items() if k != "iterations"})
        print("constant image: largest estimated variance %.3e (bound %.3e)" % (float(est.max()), _bound(rgba)))
        assert (est >= 0).all() and float(est.max()) <= _bound(rgba)


@pytest.mark.parametrize("kw", PARAMETER_SETS)
def test_stop_at_ids_keeps_half_planes_apart(kw):
    _, normal, position, _ = random_inputs()
    color = np.empty((21, 67, 4), dtype=np.float32)
    ids = np.zeros((21, 67, 4), dtype=np.int32)
    left, right = (0.5, 0.25, 4.0, 1.0), (2.0, 8.0, 0.125, 0.5)
    color[:, :30] = left
    color[:, 30:] = right
    ids[:, :30, 0] = 7
    ids[:, 30:, 0] = -1                         # background is an id like any other
    kw = dict(kw, stop_at_ids=1)
    got, _ = twin_filter(color, normal, position, ids, sigma_luminance=gpu.SIGMA_LUMINANCE, **kw)
    assert np.array_equal(got, color)
    est = twin_estimate(color, normal, position, ids, **{k: v for k, v in kw.items() if k != "iterations"})
    x0, y0, x1, y1 = kw.get("region", (0, 0, 67, 21))
    assert (est >= 0).all() and float(est[y0:y1, x0:30].max()) <= _bound(left) and float(est[y0:y1, 30:x1].max()) <= _bound(right)
    # the premise: without the stop the colours bleed across the edge, and the estimate sees the edge
    off = dict(kw, stop_at_ids=0, sigma_normal=0.0, sigma_position=0.0)
    bled, _ = twin_filter(color, normal, position, ids, sigma_luminance=0.0, **off)
    assert not np.array_equal(bled[:, 26:34], color[:, 26:34])
    assert float(twin_estimate(color, normal, position, ids, **{k: v for k, v in off.items() if k != "iterations"})[10, 28:32].min()) > 0.1


def test_pixels_outside_the_region_are_untouched():
    color, normal, position, ids = random_inputs()
    albedo = random_albedo()
    variance = (np.random.default_rng(5).random(color.shape[:2]) * 0.5).astype(np.float32)
    inside = np.zeros((21, 67), dtype=bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    kw = dict(region=REGION, iterations=5, **GUIDES)

    def runs():
        res = []
        for v in (None, variance):
            res.append(twin_filter(color, normal, position, ids, albedo=albedo, variance=v, out=np.full_like(color, -7.5),
                                   var_out=np.full(color.shape[:2], -7.5, dtype=np.float32), **kw))
        res.append((twin_estimate(color, normal, position, ids, out=np.full(color.shape[:2], -7.5, dtype=np.float32), region=REGION, **GUIDES),) * 2)
        return res

    first = runs()
    for out, var in first:
        assert (out[~inside] == np.float32(-7.5)).all() and (var[~inside] == np.float32(-7.5)).all()
        assert (out[inside] != np.float32(-7.5)).all() and (var[inside] >= 0).all()
    # ... and nothing outside the region was read: garbage there changes nothing inside
    for a in (color, normal, position, albedo, variance):
        a[~inside] = np.float32(1e30)
    ids[~inside] = 12345
    for (out, var), (out0, var0) in zip(runs(), first):
        assert np.array_equal(out, out0) and np.array_equal(var, var0)


def test_an_outlier_is_spread():
    """what the feature is for: one pixel at 100 times the grey of a flat frame, no guides.  Its estimated variance is large, so the
    luminance term lets it mix with its neighbours; told that the frame has no variance, the filter leaves it alone."""
    grey = np.float32(0.5)
    color = np.empty((33, 33, 4), dtype=np.float32)
    color[:] = (grey, grey, grey, 1.0)
    color[16, 16, :3] = 100 * grey
    got, _ = twin_filter(color, sigma_luminance=gpu.SIGMA_LUMINANCE, iterations=5, stop_at_ids=0)
    print("outlier %.3f -> %.3f after 5 iterations at sigma_luminance %g" % (float(color[16, 16, 0]), float(got[16, 16, 0]), gpu.SIGMA_LUMINANCE))
    assert float(got[16, 16, 0]) < 0.5 * float(color[16, 16, 0])
    model, _ = dvm.denoise_variance(color, sigma_luminance=gpu.SIGMA_LUMINANCE, iterations=5, stop_at_ids=False)
    check(got, model, "outlier frame")
    kept, _ = twin_filter(color, sigma_luminance=gpu.SIGMA_LUMINANCE, variance=np.zeros((33, 33), dtype=np.float32), iterations=5, stop_at_ids=0)
    err = float(dm.rel_err(kept[16, 16], color[16, 16]).max())
    print("outlier with zero variance: rel err %.3e" % err)
    assert err <= REL_TOL
