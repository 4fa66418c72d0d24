"""fjgpu_denoise without a GPU (include/fjgpu.h): the C ABI's layout and refusals, and the filter's arithmetic through its host twin.

lib/libfj_denoise_host.so (csrc/tools/denoise_host.cc) runs a plain loop over host arrays whose every tap goes through
csrc/device/fjgpu_denoise_math.h, the source k_dn_atrous compiles; tests/denoise_model.py is the numpy restatement written from the
header's text.  Twin against model: REL_TOL = 1e-4 with the error measure of tests/test_gpu_parity.py (denominator floored at 1e-3) --
the two differ in expf (glibc against numpy, a few ulp) and in nothing else.

Bit-identity.  out = (sum of w_q C_q) / (sum of w_q) returns C for a constant image only where every product w_q C is exact; for
arbitrary weights (any sigmas, random guides) that is so exactly when C is a power of two (scaling by 2^k commutes with every f32
rounding of the sums, and (2^k x) / x = 2^k exactly).  The constant-image and half-plane tests therefore use powers of two per channel
and ask for bit-identity under every parameter set.  An arbitrary positive constant comes back within 80 ulp per iteration: the worst
case of the roundings -- at most 25 products and 25 additions in the numerator (positive terms: a partial sum is not above the total),
25 additions in the denominator and one division, each 2^-24 relative, 76 in all.  The same bound holds for the comparison with the
f64 B3-spline convolution.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_model as dm
from fujiyama_renderer_amd import ffi, gpu

REL_TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_twin = None


def twin():
    global _twin
    if _twin is None:
        _twin = ffi.load("libfj_denoise_host.so")
        _twin.fj_denoise_host.argtypes = [C.POINTER(ffi.DenoiseDesc)] + [C.c_void_p] * 5
        _twin.fj_denoise_host_constants.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p]
        _twin.fj_denoise_host_constants.restype = None
    return _twin


def desc(W, H, region=None, iterations=1, sigma_color=1.0, sigma_normal=1.0, sigma_position=1.0, stop_at_ids=1):
    d = ffi.DenoiseDesc()
    d.xres, d.yres = W, H
    d.region[:] = (0, 0, W, H) if region is None else region
    d.iterations = iterations
    d.sigma_color, d.sigma_normal, d.sigma_position = sigma_color, sigma_normal, sigma_position
    d.stop_at_ids = stop_at_ids
    return d


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_twin(color, normal=None, position=None, ids=None, out=None, **kw):
    H, W = color.shape[:2]
    d = desc(W, H, **kw)
    out = color.copy() if out is None else out
    assert twin().fj_denoise_host(C.byref(d), _p(color), _p(normal), _p(position), _p(ids), _p(out)) == 0
    return out


def random_inputs(W=67, H=21, seed=20100625):
    """seeded random frame: colours in [0, 2), unit normals, positions in a 3-unit box, instance ids -1..2"""
    rng = np.random.default_rng(seed)
    color = (rng.random((H, W, 4), dtype=np.float32) * 2).astype(np.float32)
    normal = rng.standard_normal((H, W, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    position = (rng.random((H, W, 3), dtype=np.float32) * 3).astype(np.float32)
    ids = rng.integers(-1, 3, (H, W, 4)).astype(np.int32)
    return color, normal, position, ids


REGION = (3, 2, 61, 19)
SIGMAS = dict(sigma_color=1.5, sigma_normal=0.8, sigma_position=1.2)


def test_symbol_bindings_and_layout():
    L = gpu.lib()
    assert hasattr(L, "fjgpu_denoise") and L.fjgpu_denoise.argtypes is not None
    assert callable(gpu.denoise) and callable(gpu.Scene.render_denoised)
    # fjgpu_denoise_desc: int32 xres, yres, region[4], iterations; float sigma x 3; int32 stop_at_ids -- 11 four-byte members, no padding
    assert C.sizeof(ffi.DenoiseDesc) == 44
    assert [n for n, _ in ffi.DenoiseDesc._fields_] == ["xres", "yres", "region", "iterations", "sigma_color", "sigma_normal",
                                                        "sigma_position", "stop_at_ids"]
    assert ffi.DenoiseDesc.region.offset == 8 and ffi.DenoiseDesc.iterations.offset == 24 and ffi.DenoiseDesc.stop_at_ids.offset == 40
    # the header says the same
    text = open(os.path.join(ROOT, "include", "fjgpu.h")).read()
    body = text[text.index("typedef struct fjgpu_denoise_desc {"):text.index("} fjgpu_denoise_desc;")]
    members = [ln.split("/*")[0].strip() for ln in body.splitlines()[1:] if ln.strip()]
    assert members == ["int32_t xres, yres;", "int32_t region[4];", "int32_t iterations;", "float   sigma_color;", "float   sigma_normal;",
                       "float   sigma_position;", "int32_t stop_at_ids;"]
    assert hasattr(twin(), "fj_denoise_host")
    # the struct of per-call statistics did not grow
    assert C.sizeof(ffi.GpuStats) == 208


FAKE = 4096          # a non-NULL, 16-byte aligned address: every refusal below is decided before any pointer is followed


def _refused(d, cin=FAKE, cout=FAKE):
    rc = gpu.lib().fjgpu_denoise(0, None if d is None else C.byref(d), cin, None, None, None, cout, None, None)
    return rc, gpu.lib().fjgpu_last_error().decode()


@pytest.mark.parametrize("case", ["null_desc", "null_in", "null_out", "region_empty", "region_outside", "region_negative", "iterations_0",
                                  "iterations_9", "nan_color", "nan_normal", "nan_position"])
def test_einval(case):
    d = desc(64, 48)
    cin, cout = FAKE, FAKE
    what = "null"
    if case == "null_desc":
        d = None
    elif case == "null_in":
        cin = None
    elif case == "null_out":
        cout = None
    elif case.startswith("region"):
        d.region[:] = dict(region_empty=(10, 5, 10, 20), region_outside=(0, 0, 65, 48), region_negative=(-1, 0, 64, 48))[case]
        what = "region"
    elif case.startswith("iterations"):
        d.iterations = int(case[-1])
        what = "iterations"
    else:
        setattr(d, "sigma_" + case[4:], float("nan"))
        what = "NaN"
    rc, msg = _refused(d, cin, cout)
    assert rc == -2, (rc, msg)                  # FJGPU_EINVAL
    assert "fjgpu_denoise" in msg and what in msg, msg


def test_valid_call_without_a_device_is_enodev():
    """a valid description on a process that sees no device: FJGPU_ENODEV.  Run in a child whose HIP runtime is told to show none, so
    that the answer is the same on a machine with GPUs -- and the child checks that before it passes addresses it does not own."""
    code = ("import ctypes as C, sys\n"
            "sys.path.insert(0, %r)\n"
            "from fujiyama_renderer_amd import ffi, gpu\n"
            "assert gpu.device_count() == 0, 'a device is visible'\n"
            "d = ffi.DenoiseDesc(); d.xres, d.yres = 64, 48; d.region[:] = (0, 0, 64, 48); d.iterations = 5\n"
            "d.sigma_color = d.sigma_normal = d.sigma_position = 1.0\n"
            "rc = gpu.lib().fjgpu_denoise(0, C.byref(d), 4096, None, None, None, 4096, None, None)\n"
            "print('rc', rc, gpu.lib().fjgpu_last_error().decode())\n") % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "rc -1 fjgpu_denoise" in r.stdout, r.stdout          # FJGPU_ENODEV


@pytest.mark.parametrize("i", range(8))
def test_constants_f64_rounded_once(i):
    got = np.zeros(3, dtype=np.float32)
    for sig in ((3.0, 1.0, 0.1732), (0.3, 0.1, 1e-3), (0.0, -1.0, float("inf")), (1e-30, 1e30, 7.0)):
        twin().fj_denoise_host_constants(sig[0], sig[1], sig[2], i, _p(got))
        assert got.tolist() == [float(v) for v in dm.constants(sig[0], sig[1], sig[2], i)], (sig, i)
        assert np.isfinite(got).all()
    twin().fj_denoise_host_constants(2.0, 2.0, 2.0, i, _p(got))
    assert got.tolist() == [0.25 * 4.0 ** i, 0.25, 0.25]         # only the colour sigma halves


@pytest.mark.parametrize("iterations", [1, 2, 5])
def test_twin_equals_model(iterations):
    """67 x 21 frame, region (3, 2, 61, 19): at spacing 16 most taps of the 58 x 17 region fall outside it"""
    color, normal, position, ids = random_inputs()
    got = run_twin(color, normal, position, ids, region=REGION, iterations=iterations, **SIGMAS)
    ref = dm.denoise(color, normal, position, ids, iterations=iterations, region=REGION, **SIGMAS)
    err = float(dm.rel_err(got, ref).max())
    print("twin vs model, %d iterations: max rel err %.3e" % (iterations, err))
    assert err <= REL_TOL
    assert not np.array_equal(got, color)


def _b3_reference(color):
    """separable B3-spline convolution with per-pixel renormalisation at the borders, by np.convolve on values and on weights (f64)"""
    h = np.array([1, 4, 6, 4, 1], dtype=np.float64) / 16
    H, W = color.shape[:2]
    c = color.astype(np.float64)
    rows = np.stack([np.stack([np.convolve(c[y, :, k], h, mode="same") for k in range(4)], axis=1) for y in range(H)])
    full = np.stack([np.stack([np.convolve(rows[:, x, k], h, mode="same") for k in range(4)], axis=1) for x in range(W)], axis=1)
    wx = np.convolve(np.ones(W), h, mode="same")
    wy = np.convolve(np.ones(H), h, mode="same")
    return full / (wy[:, None] * wx[None, :])[:, :, None]


def test_all_terms_off_is_the_b3_spline():
    color, _, _, _ = random_inputs(W=37, H=13)
    got = run_twin(color, iterations=1, sigma_color=0.0, sigma_normal=float("inf"), sigma_position=-1.0, stop_at_ids=0)
    ref = _b3_reference(color)
    # f32 rounding: the worst case of the module's docstring, 80 x 2^-24 relative (colours are positive)
    err = np.abs(got.astype(np.float64) - ref)
    print("B3 spline: max relative error %.3e" % float((err / np.abs(ref)).max()))
    assert float((err / np.abs(ref)).max()) <= 80 * 2.0 ** -24
    # ... and the model agrees with the same convolution
    model = dm.denoise(color, iterations=1, sigma_color=0.0, stop_at_ids=False).astype(np.float64)
    assert float((np.abs(model - ref) / np.abs(ref)).max()) <= 80 * 2.0 ** -24


PARAMETER_SETS = [dict(iterations=1), dict(iterations=5), dict(iterations=8, sigma_color=1e-3, sigma_normal=1e-2, sigma_position=1e-2),
                  dict(iterations=3, sigma_color=0.0, sigma_normal=0.3, sigma_position=float("inf"), stop_at_ids=0),
                  dict(iterations=4, region=REGION)]


@pytest.mark.parametrize("kw", PARAMETER_SETS)
def test_constant_image_is_a_fixed_point(kw):
    _, normal, position, ids = random_inputs()
    color = np.empty((21, 67, 4), dtype=np.float32)
    color[:] = (0.25, 2.0, 0.0078125, 1.0)
    for guides in ((normal, position, ids), (None, None, None)):
        got = run_twin(color, *guides, **kw)
        assert np.array_equal(got, color)
    # an arbitrary constant: within the roundings' worst case
    color[:] = (0.1, 0.7, 1.3, 0.9)
    got = run_twin(color, normal, position, ids, **kw)
    assert (np.abs(got - color) <= 80 * kw["iterations"] * np.spacing(color)).all()


@pytest.mark.parametrize("kw", PARAMETER_SETS)
def test_stop_at_ids_keeps_half_planes_apart(kw):
    _, normal, position, _ = random_inputs()
    color = np.empty((21, 67, 4), dtype=np.float32)
    ids = np.zeros((21, 67, 4), dtype=np.int32)
    color[:, :30] = (0.5, 0.25, 4.0, 1.0)
    color[:, 30:] = (2.0, 8.0, 0.125, 0.5)
    ids[:, :30, 0] = 7
    ids[:, 30:, 0] = -1                         # background is an id like any other
    kw = dict(kw, stop_at_ids=1)
    got = run_twin(color, normal, position, ids, **kw)
    assert np.array_equal(got, color)
    # the premise: without the stop the colours bleed across the edge
    off = dict(sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0)
    bled = run_twin(color, normal, position, ids, **dict(kw, stop_at_ids=0, **off))
    assert not np.array_equal(bled[:, 26:34], color[:, 26:34])
    # ids given but stop_at_ids 0, and stop_at_ids 1 without ids: no stop
    assert np.array_equal(run_twin(color, normal, position, None, **dict(kw, **off)), bled)


def test_pixels_outside_the_region_are_untouched():
    color, normal, position, ids = random_inputs()
    out = np.full_like(color, -7.5)
    got = run_twin(color, normal, position, ids, out=out, region=REGION, iterations=5, **SIGMAS)
    inside = np.zeros((21, 67), dtype=bool)
    inside[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    assert (got[~inside] == np.float32(-7.5)).all()
    assert (got[inside] != np.float32(-7.5)).all()
    # ... and nothing outside the region was read: garbage there changes nothing inside
    for a in (color, normal, position):
        a[~inside] = np.float32(1e30)
    ids[~inside] = 12345
    again = run_twin(color, normal, position, ids, out=np.full_like(color, -7.5), region=REGION, iterations=5, **SIGMAS)
    assert np.array_equal(again, got)
