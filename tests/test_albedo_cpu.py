"""The albedo pass and albedo-demodulated denoising without a GPU (include/fjgpu.h: fjgpu_render_aov_albedo, fjgpu_denoise_albedo):
exports, the Python face, the refusals that are decided before a device is touched, the demodulation's arithmetic through the host
twin (csrc/tools/denoise_host.cc: fj_denoise_albedo_host, the three functions of fjgpu_denoise_math.h the kernels compile) and the
numpy texture lookup of tests/albedo_model.py against hand-computed texels.

Twin against numpy: demodulation and remodulation are one IEEE f32 division and one multiplication per value, which numpy's f32
operators are too, so "numpy-demodulate, fj_denoise_host, numpy-remodulate" is asked for BIT for bit; against the numpy filter
(albedo_model.demodulated_denoise) the bound is test_denoise_cpu's REL_TOL (the two filters differ in expf).
"""
import ctypes as C
import inspect

import numpy as np
import pytest

import albedo_model as am
import denoise_model as dm
from fujiyama_renderer_amd import ffi, gpu
from test_denoise_cpu import FAKE, REGION, REL_TOL, SIGMAS, _p, desc, random_inputs, run_twin, twin

FJGPU_EINVAL = -2
FLOOR = 0.05


def _err():
    return gpu.lib().fjgpu_last_error().decode("utf-8", "replace")


def albedo_twin():
    t = twin()
    t.fj_denoise_albedo_host.argtypes = [C.POINTER(ffi.DenoiseDesc)] + [C.c_void_p] * 5 + [C.c_float, C.c_void_p]
    return t


def run_albedo_twin(color, normal, position, ids, albedo, albedo_floor, out=None, **kw):
    H, W = color.shape[:2]
    d = desc(W, H, **kw)
    out = color.copy() if out is None else out
    assert albedo_twin().fj_denoise_albedo_host(C.byref(d), _p(color), _p(normal), _p(position), _p(ids), _p(albedo), albedo_floor, _p(out)) == 0
    return out


def random_albedo(W=67, H=21, seed=1848, floor=FLOOR):
    """values in (0, 2), a tenth of them below the floor, a tenth exact zeros"""
    rng = np.random.default_rng(seed)
    a = (rng.random((H, W, 3), dtype=np.float32) * 2).astype(np.float32)
    a = np.maximum(a, np.float32(1e-6))
    pick = rng.random((H, W, 3))
    a[pick < 0.1] = (rng.random((H, W, 3), dtype=np.float32) * np.float32(floor))[pick < 0.1]
    a[pick > 0.9] = 0
    assert (a == 0).any() and ((a > 0) & (a < floor)).any() and (a > 1).any()
    return a


# ---- exports and face

def test_exports_and_python_face():
    L = gpu.lib()
    assert callable(L.fjgpu_render_aov_albedo) and callable(L.fjgpu_denoise_albedo)
    assert hasattr(albedo_twin(), "fj_denoise_albedo_host")
    assert gpu.AOV_NAMES == ("depth", "position", "normal", "uv", "ids", "coverage")
    assert gpu.AOV_ALL == gpu.AOV_NAMES + ("albedo",) and gpu.AOV_CHANNELS["albedo"] == 3
    assert inspect.signature(gpu.Scene.render_aov).parameters["want"].default == gpu.AOV_NAMES
    assert inspect.signature(gpu.Scene.render_aov_albedo).parameters["want"].default == gpu.AOV_ALL
    assert list(inspect.signature(gpu.Scene.render_aov_albedo).parameters) == list(inspect.signature(gpu.Scene.render_aov).parameters)
    p = inspect.signature(gpu.denoise).parameters
    assert p["albedo"].default is None and p["albedo_floor"].default == gpu.ALBEDO_FLOOR
    assert np.isfinite(gpu.ALBEDO_FLOOR) and gpu.ALBEDO_FLOOR > 0
    assert inspect.signature(gpu.Scene.render_denoised).parameters["demodulate"].default is False
    # no struct grew
    assert C.sizeof(ffi.AovBuffers) == 6 * C.sizeof(C.c_void_p) and C.sizeof(ffi.DenoiseDesc) == 44 and C.sizeof(ffi.GpuStats) == 208


def test_names_are_checked_per_entry_point():
    """render_aov keeps its six names ("albedo" is not one of fjgpu_aov_buffers' members); render_aov_albedo knows seven"""
    class _NoScene(gpu.Scene):
        def __init__(self):
            self._h = C.c_void_p()
            self._device = 0
    with pytest.raises(ValueError, match="unknown AOV 'albedo'"):
        _NoScene().render_aov(ffi.RenderDesc(), want=("albedo",))
    with pytest.raises(ValueError, match="unknown AOV 'emission'.*albedo"):
        _NoScene().render_aov_albedo(ffi.RenderDesc(), want=("albedo", "emission"))


# ---- refusals decided before any device is touched (FAKE: a non-NULL address that is never followed)

def test_render_aov_albedo_refusals():
    L = gpu.lib()
    rd, bufs, st = ffi.RenderDesc(), ffi.AovBuffers(), ffi.GpuStats()
    assert L.fjgpu_render_aov_albedo(None, C.byref(rd), None, 0, C.byref(bufs), FAKE, None, C.byref(st)) == FJGPU_EINVAL
    assert "fjgpu_render_aov_albedo" in _err() and "null" in _err().lower()
    assert L.fjgpu_render_aov_albedo(FAKE, None, None, 0, C.byref(bufs), FAKE, None, None) == FJGPU_EINVAL
    assert "fjgpu_render_aov_albedo" in _err()
    # nothing wanted: buffers NULL, or all its members NULL, and no albedo
    for b in (None, C.byref(bufs)):
        assert L.fjgpu_render_aov_albedo(FAKE, C.byref(rd), None, 0, b, None, None, None) == FJGPU_EINVAL
        assert "fjgpu_render_aov_albedo" in _err() and "NULL" in _err()
    # ... and the old entry point keeps its own name
    assert L.fjgpu_render_aov(FAKE, C.byref(rd), None, 0, C.byref(bufs), None, None) == FJGPU_EINVAL
    assert "fjgpu_render_aov:" in _err() and "NULL" in _err()


@pytest.mark.parametrize("floor", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_denoise_albedo_refuses_a_bad_floor(floor):
    d = desc(64, 48)
    rc = gpu.lib().fjgpu_denoise_albedo(0, C.byref(d), FAKE, None, None, None, FAKE, floor, FAKE, None, None)
    assert rc == FJGPU_EINVAL and "albedo_floor" in _err() and "fjgpu_denoise_albedo" in _err()


@pytest.mark.parametrize("case", ["null_desc", "null_in", "null_out", "region_empty", "region_outside", "iterations_0", "iterations_9", "nan_color"])
@pytest.mark.parametrize("floor", [0.0, 0.01])
def test_denoise_albedo_without_albedo_refuses_what_fjgpu_denoise_refuses(case, floor):
    """albedo NULL: the same codes, whatever albedo_floor holds (it is ignored)"""
    d = desc(64, 48)
    cin, cout = FAKE, FAKE
    if case == "null_desc":
        d = None
    elif case == "null_in":
        cin = None
    elif case == "null_out":
        cout = None
    elif case.startswith("region"):
        d.region[:] = dict(region_empty=(10, 5, 10, 20), region_outside=(0, 0, 65, 48))[case]
    elif case.startswith("iterations"):
        d.iterations = int(case[-1])
    else:
        d.sigma_color = float("nan")
    L = gpu.lib()
    dp = None if d is None else C.byref(d)
    rc0 = L.fjgpu_denoise(0, dp, cin, None, None, None, cout, None, None)
    msg0 = _err()
    rc1 = L.fjgpu_denoise_albedo(0, dp, cin, None, None, None, None, floor, cout, None, None)
    assert rc0 == rc1 == FJGPU_EINVAL and _err() == msg0
    # ... and with an albedo and a good floor the same arguments are refused the same way
    assert L.fjgpu_denoise_albedo(0, dp, cin, None, None, None, FAKE, 0.01, cout, None, None) == FJGPU_EINVAL and _err() == msg0


# ---- the host twin

@pytest.fixture(scope="module")
def frames():
    color, normal, position, ids = random_inputs()
    return color, normal, position, ids, random_albedo()


@pytest.mark.parametrize("iterations", [1, 5])
def test_twin_is_numpy_demodulate_filter_remodulate(frames, iterations):
    """region (3, 2, 61, 19) of the 67 x 21 frame: bit-identical to the three steps done apart; pixels outside the region untouched; the
    alpha channel is the plain filter's on (D, alpha)"""
    color, normal, position, ids, albedo = frames
    kw = dict(region=REGION, iterations=iterations, **SIGMAS)
    got = run_albedo_twin(color, normal, position, ids, albedo, FLOOR, out=np.full_like(color, -7.5), **kw)
    D, a = am.demodulate(color, albedo, FLOOR, REGION)
    F = run_twin(D, normal, position, ids, **kw)
    x0, y0, x1, y1 = REGION
    ref = np.full_like(color, -7.5)
    ref[y0:y1, x0:x1, :3] = F[y0:y1, x0:x1, :3] * a[y0:y1, x0:x1]
    ref[y0:y1, x0:x1, 3] = F[y0:y1, x0:x1, 3]
    assert np.array_equal(got, ref)
    inside = np.zeros(color.shape[:2], dtype=bool)
    inside[y0:y1, x0:x1] = True
    assert (got[~inside] == np.float32(-7.5)).all() and (got[inside] != np.float32(-7.5)).all()
    assert np.array_equal(got[y0:y1, x0:x1, 3], F[y0:y1, x0:x1, 3])
    # the clamp did something: values below the floor and exact zeros were divided by the floor
    assert np.isfinite(got[inside]).all() and (a[y0:y1, x0:x1] == np.float32(FLOOR)).any()
    # the numpy filter in between instead: the project's tolerance
    model = am.demodulated_denoise(color, normal, position, ids, albedo=albedo, albedo_floor=FLOOR, region=REGION, iterations=iterations, **SIGMAS)
    err = float(dm.rel_err(got[y0:y1, x0:x1], model[y0:y1, x0:x1]).max())
    print("albedo twin vs model, %d iterations: max rel err %.3e" % (iterations, err))
    assert err <= REL_TOL
    # only region pixels of the albedo are read
    junk = albedo.copy()
    junk[~inside] = np.nan
    assert np.array_equal(run_albedo_twin(color, normal, position, ids, junk, FLOOR, out=np.full_like(color, -7.5), **kw), got)


def test_twin_without_albedo_is_the_plain_twin(frames):
    color, normal, position, ids, _ = frames
    kw = dict(region=REGION, iterations=3, **SIGMAS)
    assert np.array_equal(run_albedo_twin(color, normal, position, ids, None, 0.0, **kw), run_twin(color, normal, position, ids, **kw))


def test_twin_refuses_a_bad_floor(frames):
    color, normal, position, ids, albedo = frames
    d = desc(67, 21)
    out = color.copy()
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        assert albedo_twin().fj_denoise_albedo_host(C.byref(d), _p(color), None, None, None, _p(albedo), floor, _p(out)) == FJGPU_EINVAL


# ---- demodulation as identity

def test_albedo_of_ones_gives_the_plain_filter(frames):
    """x / 1 and x * 1 are exact"""
    color, normal, position, ids, _ = frames
    ones = np.ones((21, 67, 3), dtype=np.float32)
    kw = dict(region=REGION, iterations=5, **SIGMAS)
    assert np.array_equal(run_albedo_twin(color, normal, position, ids, ones, FLOOR, **kw), run_twin(color, normal, position, ids, **kw))


@pytest.mark.parametrize("kw", [dict(iterations=1), dict(iterations=5), dict(iterations=4, region=REGION),
                                dict(iterations=3, sigma_color=0.0, sigma_normal=0.3, sigma_position=float("inf"), stop_at_ids=0)])
def test_constant_illumination_under_any_albedo_is_a_fixed_point(frames, kw):
    """C = a L with L a power of two per channel and a >= floor comes back bit for bit.  a L is exact (scaling by a power of two, no
    under- or overflow here), so D = (a L) / a = L exactly: the filter sees a constant image whose channels are powers of two, which it
    returns bit for bit under any weights (test_denoise_cpu.py: scaling by 2^k commutes with every f32 rounding of the sums, and
    (2^k x) / x = 2^k exactly); out = L a = C exactly again.  Alpha is a power of two as well."""
    _, normal, position, ids, albedo = frames
    a = np.maximum(albedo, np.float32(FLOOR))
    L = np.array([0.25, 2.0, 0.0078125], dtype=np.float32)
    color = np.empty((21, 67, 4), dtype=np.float32)
    color[:, :, :3] = a * L
    color[:, :, 3] = 0.5
    assert len(np.unique(color[:, :, 0])) > 100          # (the frame itself is anything but constant)
    got = run_albedo_twin(color, normal, position, ids, a, FLOOR, **kw)
    assert np.array_equal(got, color)
    # the premise: the plain filter does not leave this frame alone
    assert not np.array_equal(run_twin(color, normal, position, ids, **kw), color)


# ---- albedo_model.tex_lookup against hand-computed texels

def _synthetic(nch, ts=64, xnt=2, ynt=1):
    """tile-major texture whose texel (tile, row, column) channel c holds 1000 tile + 10 row + column / 8 + c / 64: exact in f32"""
    tiles = np.empty((ynt * xnt, ts, ts, nch), dtype=np.float32)
    for t in range(ynt * xnt):
        for c in range(nch):
            tiles[t, :, :, c] = 1000 * t + 10 * np.arange(ts)[:, None] + np.arange(ts)[None, :] / 8 + c / 64
    return am.make_texture(xnt * ts, ynt * ts, nch, ts, tiles)


def _texel(t, r, col, c=0):
    return np.float32(1000 * t + 10 * r + col / 8 + c / 64)


@pytest.mark.parametrize("nch", [1, 3, 4])
def test_tex_lookup_hand_computed(nch):
    tex = _synthetic(nch)
    rgb = lambda t, r, col: [_texel(t, r, col, c if nch > 1 else 0) for c in range(3)]
    # u 0.25 of two tiles across: su = 0.5 -> tile 0, column (int) (0.5 * 64) = 32; v 0.25: sv = (1 - 0.25) * 1 -> row 48 (v is flipped)
    assert am.tex_lookup(tex, 0.25, 0.25)[0].tolist() == rgb(0, 48, 32)
    # u 0.75: su = 1.5 -> tile 1, column 32; v 0.75 -> row 16
    assert am.tex_lookup(tex, 0.75, 0.75)[0].tolist() == rgb(1, 16, 32)
    # wrap: -0.75 and 1.25 are 0.25; v -0.25 is 0.75, v 2.25 is 0.25
    assert am.tex_lookup(tex, -0.75, -0.25)[0].tolist() == rgb(0, 16, 32)
    assert am.tex_lookup(tex, 1.25, 2.25)[0].tolist() == rgb(0, 48, 32)
    # the corners: u = 0 -> column 0; v = 0: tv = 0, sv = 1 -> the tile index clamps to 0 and the fraction is 0 -> row 0
    assert am.tex_lookup(tex, 0.0, 0.0)[0].tolist() == rgb(0, 0, 0)
    # u just below 1: su just below 2 -> tile 1, column 63; v just below 1 -> sv tiny -> row 0
    lo = np.nextafter(np.float32(1), np.float32(0))
    assert am.tex_lookup(tex, lo, lo)[0].tolist() == rgb(1, 0, 63)
    # arrays in, [n, 3] out
    out = am.tex_lookup(tex, np.array([0.25, 0.75], dtype=np.float32), np.array([0.25, 0.75], dtype=np.float32))
    assert out.dtype == np.float32 and out.tolist() == [rgb(0, 48, 32), rgb(1, 16, 32)]


def test_tex_lookup_width_zero_and_outside_the_tile():
    assert am.tex_lookup(am.make_texture(0, 0, 3, 64, None), 0.3, 0.4)[0].tolist() == [np.float32(1), np.float32(.63), np.float32(.63)]
    # tiles of 32: the in-tile pixel is (fraction * 64), so fractions of a half and more lie outside the stored pixels -> zeros
    tex = _synthetic(3, ts=32, xnt=2, ynt=1)
    assert am.tex_lookup(tex, 0.25, 0.9)[0].tolist() == [0, 0, 0]                    # su = 0.5: column 32 >= 32
    # u 0.1: su = 0.2 -> tile 0, column (int) 12.8 = 12; v 0.9: sv = (1 - 0.9f) -> row (int) (0.1 * 64) = 6
    assert am.tex_lookup(tex, 0.1, 0.9)[0].tolist() == [_texel(0, 6, 12, c) for c in range(3)]
    assert am.texel_index(tex, np.float32(0.25), np.float32(0.9)) == -1


def test_tex_lookup_is_the_oracles():
    """the restatement against the CPU oracle's Texture::Lookup on random coordinates, wraps included"""
    import oracle_ffi

    class _T(C.Structure):
        _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("nchannels", C.c_int32), ("tilesize", C.c_int32), ("tiles", C.c_void_p)]
    tex = _synthetic(3, ts=64, xnt=2, ynt=3)
    t = _T(tex["width"], tex["height"], 3, 64, tex["tiles"].ctypes.data)
    rng = np.random.default_rng(5)
    uv = (rng.random((4000, 2), dtype=np.float32) * 6 - 3).astype(np.float32)
    out = np.empty((4000, 4), dtype=np.float32)
    oracle_ffi.lib().fjo_texture_lookup(C.byref(t), 4000, _p(uv), _p(out))
    assert np.array_equal(am.tex_lookup(tex, uv[:, 0], uv[:, 1]), out[:, :3])


# ---- the exclusion cap of tests/test_gpu_albedo.py, counted with the oracle's uv alone

def test_fragile_samples_stay_under_the_cap(asset_dir):
    """pixels holding a sample whose texel a one-ulp move of its uv changes are left out of the GPU comparison; at most 1 % of the
    textured pixels may be.  Counted here on the textured scene with the oracle's sampler, camera and trace."""
    import edge_scenes
    import oracle_ffi
    from test_gpu_aov import SceneView, all_tiles, prepare
    sp, rd = prepare(edge_scenes.custom_scene(asset_dir, **edge_scenes.EDGE_CASES["textures_diffuse_and_bump"]))
    view, tab = SceneView(sp), am.Tables(sp)
    osc = oracle_ffi.OracleScene(sp)
    try:
        e = am.expected_albedo(am.OracleSamples(sp), osc, view, tab, rd, all_tiles(rd))
    finally:
        osc.close()
    n_tex, n_out = int(e["textured"].sum()), int((e["textured"] & e["fragile"]).sum())
    print("textured pixels %d, left out %d" % (n_tex, n_out))
    assert n_tex > 1000 and n_out <= 0.01 * n_tex
    a = e["albedo"][e["textured"] & ~e["fragile"]]
    assert len(np.unique(a, axis=0)) > 50          # the sky map varies over the dome
