"""fjgpu_render_aov_matte without a GPU (include/fjgpu.h): the prototype and its refusals, and the definition through its host twin.

lib/libfj_matte_host.so (csrc/tools/matte_host.cc) runs fj_mt_pixel of csrc/device/fjgpu_matte_math.h -- the header the kernel
k_aov_matte compiles -- over host arrays laid out as the AOV pass holds its samples; tests/matte_model.py is the numpy restatement
written from the header's text.

Bounds.  Own mode (weights 1): every sum is a count, so ids, coverage, rest and distinct are EQUAL.  Filtered mode: ids and distinct equal,
coverage and rest within one f32 ulp of the model's value (the output's rounding) + 1e-12 (twin and model add the same f64 weights in
another order) -- the random weights of these cases put no two keys of a pixel within 1e-12 W of each other, which the tests assert
before they compare rank by rank.
"""
import ctypes as C

import numpy as np
import pytest

import matte_model as mm
import sample_variance_model as svm
from fujiyama_renderer_amd import ffi, gpu
from test_gpu_aov import shader_slot, ulp32

F = np.float32


class MtFrame(C.Structure):            # fj_mt_host_frame
    _fields_ = ([(n, C.c_int32) for n in ("xres", "yres", "rate_x", "rate_y", "npx_x", "npx_y")] + [("fw", C.c_double), ("fh", C.c_double)]
                + [("margin_x", C.c_int32), ("margin_y", C.c_int32)])


class MtTile(C.Structure):             # fj_mt_host_tile
    _fields_ = [(n, C.c_int32) for n in ("xmin", "ymin", "xmax", "ymax", "nx", "ny")] + [("sample_offset", C.c_uint32), ("pad", C.c_int32)]


_twin = None


def twin():
    global _twin
    if _twin is None:
        _twin = ffi.load("libfj_matte_host.so")
        _twin.fj_matte_host.argtypes = [C.POINTER(MtFrame), C.POINTER(MtTile), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
        _twin.fj_matte_host_shader_key.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return _twin


def run_twin(frame, tiles, s_uv, keys, filtered, ranks, rc_want=0):
    fr = MtFrame(**frame)
    ts = (MtTile * len(tiles))(*[MtTile(T["xmin"], T["ymin"], T["xmax"], T["ymax"], T["nx"], T["ny"], T["sample_offset"], 0) for T in tiles])
    H, W = frame["yres"], frame["xres"]
    k = max(1, min(ranks, 16))
    out = dict(ids=np.full((H, W, k), -9, np.int32), coverage=np.full((H, W, k), -9, np.float32), rest=np.full((H, W, 1), -9, np.float32),
               distinct=np.full((H, W, 1), -9, np.int32))
    s_uv = np.ascontiguousarray(s_uv, dtype=np.float64)
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    rc = twin().fj_matte_host(C.byref(fr), ts, len(tiles), int(filtered), ranks, s_uv.ctypes.data, keys.ctypes.data, out["ids"].ctypes.data,
                              out["coverage"].ctypes.data, out["rest"].ctypes.data, out["distinct"].ctypes.data)
    assert rc == rc_want, rc
    return out


def batch(rng, xres, yres, tile_w, rate, filt, n_keys, p_miss=.2, jitter=1.0):
    """the sample arrays of a frame cut into tiles tile_w wide, as the AOV pass lays them out (per tile rate * size + 2 margin samples a
    side, the tiles one after the other): jittered film positions, random keys out of n_keys (sparse, not consecutive) and misses"""
    rx, ry = rate
    mx, my = svm.sampler_margin(rx, filt[0]), svm.sampler_margin(ry, filt[1])
    frame = dict(xres=xres, yres=yres, rate_x=rx, rate_y=ry, npx_x=rx + 2 * mx, npx_y=ry + 2 * my, fw=float(F(filt[0])), fh=float(F(filt[1])),
                 margin_x=mx, margin_y=my)
    tiles, uvs, off = [], [], 0
    for xmin in range(0, xres, tile_w):
        xmax = min(xmin + tile_w, xres)
        nx, ny = rx * (xmax - xmin) + 2 * mx, ry * yres + 2 * my
        y, x = np.mgrid[0:ny, 0:nx]
        u = (.5 + x + (xmin * rx - mx) + jitter * (rng.random((ny, nx)) - .5)) / (rx * xres)
        v = 1 - (.5 + y - my + jitter * (rng.random((ny, nx)) - .5)) / (ry * yres)
        tiles.append(dict(xmin=xmin, ymin=0, xmax=xmax, ymax=yres, nx=nx, ny=ny, sample_offset=off))
        uvs.append(np.stack([u.reshape(-1), v.reshape(-1)], axis=1))
        off += nx * ny
    s_uv = np.concatenate(uvs)
    labels = np.sort(rng.choice(1000, size=n_keys, replace=False)).astype(np.int32)
    keys = labels[rng.integers(0, n_keys, size=off)]
    keys[rng.random(off) < p_miss] = -1
    return frame, tiles, s_uv, keys


def compare(got, exp, filtered, ranks):
    """twin against model with the bounds of the module's docstring -> the worst filtered deviation in units of its bound"""
    assert np.array_equal(got["distinct"], exp["distinct"])
    if not filtered:
        for name in ("ids", "coverage", "rest"):
            assert np.array_equal(got[name], exp[name]), name
        return 0.0
    A, W = exp["A"], exp["W"]
    gap = (np.abs(A[:, :, :-1] - A[:, :, 1:]) / W[:, :, None])[(A[:, :, :-1] >= 0) & (A[:, :, 1:] >= 0)]
    assert gap.size == 0 or gap.min() > 1e-12          # (the premise of a rank-by-rank comparison)
    assert np.array_equal(got["ids"], exp["ids"])
    worst = 0.0
    for name in ("coverage", "rest"):
        err = np.abs(got[name].astype(np.float64) - exp[name].astype(np.float64))
        bound = ulp32(exp[name]) + 1e-12
        assert (err <= bound).all(), (name, float(err.max()))
        worst = max(worst, float((err / bound).max()))
    return worst


# rate, filter widths -> window: 1 sample; 5 x 3 (own 3 x 1); 11 x 10, more than 64 (own 5 x 4)
WINDOWS = {"1": ((1, 1), (1.0, 1.0), (1, 1)), "5x3": ((3, 1), (1.5, 3.0), (5, 3)), "11x10": ((5, 4), (2.0, 2.5), (11, 10))}


@pytest.mark.parametrize("ranks", [1, 3, 16])
@pytest.mark.parametrize("filtered", [0, 1])
@pytest.mark.parametrize("window", sorted(WINDOWS))
def test_twin_matches_model(window, filtered, ranks):
    rate, filt, npx = WINDOWS[window]
    rng = np.random.default_rng(1000 * sorted(WINDOWS).index(window) + 100 * filtered + ranks)
    frame, tiles, s_uv, keys = batch(rng, 7, 5, 4, rate, filt, n_keys=6)
    assert (frame["npx_x"], frame["npx_y"]) == npx and len(tiles) == 2
    got = run_twin(frame, tiles, s_uv, keys, filtered, ranks)
    exp = mm.tiles_matte(frame, tiles, s_uv, keys, filtered, ranks)
    worst = compare(got, exp, filtered, ranks)
    print("window %s filtered %d ranks %d: worst deviation %.3f of the bound" % (window, filtered, ranks, worst))
    if npx[0] * npx[1] > 1:
        assert exp["distinct"].max() > 1
    if ranks == 1 and npx[0] * npx[1] > 1:
        assert (exp["rest"] > 0).any()


@pytest.mark.parametrize("filtered", [0, 1])
def test_every_sample_a_miss(filtered):
    rng = np.random.default_rng(5)
    frame, tiles, s_uv, keys = batch(rng, 5, 4, 3, (3, 2), (2.0, 2.0), n_keys=3, p_miss=1.0)
    assert (keys == -1).all()
    for impl in (run_twin(frame, tiles, s_uv, keys, filtered, 4), mm.tiles_matte(frame, tiles, s_uv, keys, filtered, 4)):
        assert (impl["ids"] == -1).all() and not impl["coverage"].any() and not impl["rest"].any() and not impl["distinct"].any()


@pytest.mark.parametrize("filtered", [0, 1])
def test_more_keys_than_ranks(filtered):
    """12 keys over windows of 110 samples, 2 ranks: the two greatest shares are kept, the others are `rest`, `distinct` counts them all"""
    rng = np.random.default_rng(11)
    rate, filt, _ = WINDOWS["11x10"]
    frame, tiles, s_uv, keys = batch(rng, 4, 3, 4, rate, filt, n_keys=12, p_miss=.1)
    got2 = run_twin(frame, tiles, s_uv, keys, filtered, 2)
    got16 = run_twin(frame, tiles, s_uv, keys, filtered, 16)
    exp2 = mm.tiles_matte(frame, tiles, s_uv, keys, filtered, 2)
    compare(got2, exp2, filtered, 2)
    assert got2["distinct"].min() > 2 and (got2["rest"] > 0).all()
    assert np.array_equal(got2["distinct"], got16["distinct"]) and not got16["rest"][got16["distinct"] <= 16].any()
    assert np.array_equal(got2["ids"], got16["ids"][:, :, :2]) and np.array_equal(got2["coverage"], got16["coverage"][:, :, :2])
    tail = got16["coverage"][:, :, 2:].astype(np.float64).sum(axis=2)
    assert np.abs(got2["rest"][:, :, 0] - tail).max() <= 16 * 2.0 ** -24       # (the f32 roundings of up to 14 shares and of rest)


def test_exact_ties_in_own_mode_keep_ascending_keys():
    """one pixel, 2 x 3 own samples: keys 40, 7, 40, 7, 19, miss -> 7 and 40 tie at 2/6 and come out in ascending key order before 19"""
    frame = dict(xres=1, yres=1, rate_x=2, rate_y=3, npx_x=2, npx_y=3, fw=1.0, fh=1.0, margin_x=0, margin_y=0)
    tile = dict(xmin=0, ymin=0, xmax=1, ymax=1, nx=2, ny=3, sample_offset=0)
    keys = np.array([40, 7, 40, 7, 19, -1], dtype=np.int32)
    uv = np.full((6, 2), .5)
    for impl in (run_twin, mm.tiles_matte):
        out = impl(frame, [tile], uv, keys, 0, 4)
        assert out["ids"][0, 0].tolist() == [7, 40, 19, -1]
        assert np.array_equal(out["coverage"][0, 0], np.array([F(2) / F(6), F(2) / F(6), F(1) / F(6), 0], dtype=np.float32))
        assert out["distinct"][0, 0, 0] == 3 and out["rest"][0, 0, 0] == 0
        out = impl(frame, [tile], uv, keys, 0, 1)                   # the first of the tie keeps the rank, the other two are `rest`
        assert out["ids"][0, 0].tolist() == [7] and out["rest"][0, 0, 0] == F(3) / F(6) and out["distinct"][0, 0, 0] == 3
    # three keys at 2/6 each into two ranks: the greatest key never enters the full list
    keys = np.array([5, 3, 9, 9, 3, 5], dtype=np.int32)
    for impl in (run_twin, mm.tiles_matte):
        out = impl(frame, [tile], uv, keys, 0, 2)
        assert out["ids"][0, 0].tolist() == [3, 5] and out["rest"][0, 0, 0] == F(2) / F(6)


@pytest.mark.parametrize("filtered", [0, 1])
def test_relabelling_keeps_the_coverages(filtered):
    """keys mapped by an order-preserving map: the same sums in the same order, so the same bits, under the mapped ids"""
    rng = np.random.default_rng(3)
    frame, tiles, s_uv, keys = batch(rng, 6, 4, 6, (3, 2), (2.0, 2.0), n_keys=5)
    relabel = np.where(keys >= 0, 3 * keys.astype(np.int64) + 100000, -1).astype(np.int32)
    for impl in (run_twin, mm.tiles_matte):
        a = impl(frame, tiles, s_uv, keys, filtered, 3)
        b = impl(frame, tiles, s_uv, relabel, filtered, 3)
        assert np.array_equal(np.where(a["ids"] >= 0, 3 * a["ids"] + 100000, -1), b["ids"])
        for name in ("coverage", "rest", "distinct"):
            assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("filtered", [0, 1])
@pytest.mark.parametrize("ranks", [1, 3, 16])
def test_shares_sum_to_one(filtered, ranks):
    """sum(coverage) + rest + the misses' share = 1 within the f32 roundings of ranks + 2 terms"""
    rng = np.random.default_rng(17 + ranks)
    rate, filt, _ = WINDOWS["5x3"]
    frame, tiles, s_uv, keys = batch(rng, 6, 4, 6, rate, filt, n_keys=5, p_miss=.3)
    got = run_twin(frame, tiles, s_uv, keys, filtered, ranks)
    # the misses' share: the model's, with every hit relabelled a miss and every miss one key
    miss = mm.tiles_matte(frame, tiles, s_uv, np.where(keys < 0, 1, -1).astype(np.int32), filtered, 1)["coverage"][:, :, 0]
    total = got["coverage"].astype(np.float64).sum(axis=2) + got["rest"][:, :, 0] + miss
    assert np.abs(total - 1).max() <= (ranks + 2) * 2.0 ** -24
    assert (miss > 0).any() and (miss < 1).any()


def test_twin_refuses_what_the_entry_point_refuses():
    rng = np.random.default_rng(1)
    frame, tiles, s_uv, keys = batch(rng, 4, 3, 4, (2, 2), (2.0, 2.0), n_keys=3)
    for ranks in (0, 17):
        run_twin(frame, tiles, s_uv, keys, 1, ranks, rc_want=-2)
    short = dict(tiles[0], nx=tiles[0]["nx"] - 1)
    run_twin(frame, [short], s_uv, keys, 1, 2, rc_want=-2)


def test_shader_key_slot_rules():
    """fj_mt_shader_key against test_gpu_aov.shader_slot: a group out of range or an unassigned slot gives slot 0, -1 where that is unassigned"""
    for shaders, n in (([4, 2, -1, 9, -1, -1, -1, -1], 4), ([-1, 6, -1, -1, -1, -1, -1, -1], 2), ([3, -1, -1, -1, -1, -1, -1, -1], 1)):
        arr = np.array(shaders, dtype=np.int32)
        for sg in range(-2, 9):
            assert twin().fj_matte_host_shader_key(sg, n, arr.ctypes.data) == shader_slot(dict(shaders=shaders, n_shaders=n), sg)
    assert twin().fj_matte_host_shader_key(1, 2, np.array([-1, 6] + [-1] * 6, dtype=np.int32).ctypes.data) == 6
    assert twin().fj_matte_host_shader_key(0, 2, np.array([-1, 6] + [-1] * 6, dtype=np.int32).ctypes.data) == -1


def test_matte_select_numpy():
    ids = np.array([[[3, 7, -1], [7, 3, 5]], [[-1, -1, -1], [5, -1, -1]]], dtype=np.int32)
    cov = np.array([[[.5, .25, 0], [.75, .125, .125]], [[0, 0, 0], [1, 0, 0]]], dtype=np.float32)
    assert np.array_equal(gpu.matte_select(ids, cov, [7]), np.array([[.25, .75], [0, 0]], dtype=np.float32))
    assert np.array_equal(gpu.matte_select(ids, cov, [3, 5]), np.array([[.5, .25], [0, 1]], dtype=np.float32))
    assert np.array_equal(gpu.matte_select(ids, cov, 5), np.array([[0, .125], [0, 1]], dtype=np.float32))
    assert not gpu.matte_select(ids, cov, []).any() and gpu.matte_select(ids, cov, [7]).dtype == np.float32
    assert not gpu.matte_select(ids, cov, [-1]).any()          # (an empty rank holds coverage 0)


def test_entry_point_refuses_null_arguments():
    """no device work before the refusals: FJGPU_EINVAL, the message naming the entry point"""
    L = gpu.lib()
    rd = ffi.RenderDesc()
    desc = ffi.MatteDesc(0, 4, 1, 0)
    bufs = ffi.MatteBuffers()
    assert L.fjgpu_render_aov_matte(None, C.byref(rd), None, 0, C.byref(desc), C.byref(bufs), None, None) == -2
    assert "fjgpu_render_aov_matte" in L.fjgpu_last_error().decode()
    assert (ffi.MATTE_KEYS, ffi.MATTE_MAX_RANKS) == ({"instance": 0, "shader": 1}, 16)
    assert C.sizeof(ffi.MatteDesc) == 16 and C.sizeof(ffi.MatteBuffers) == 32
