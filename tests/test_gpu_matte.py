"""GPU suite (-m gpu): the ranked id/coverage mattes (include/fjgpu.h: fjgpu_render_aov_matte) against tests/matte_model.py.

Every expected value is the numpy model's (matte_model.py, written from csrc/device/fjgpu_matte_math.h) over the oracle's trace of the
very rays the device traced (Scene.camera_samples), with the film positions recomputed from the sampler's formula.

Bounds.  Own mode (filtered = 0): every sum is a count -- ids, coverage, rest and distinct are EQUAL.  Filtered mode: distinct equal;
coverage and rest within one f32 ulp of the model's value (the output's own rounding) + 1e-12 (the kernel's butterfly and numpy's
pairwise sum add the same f64 weights in another order); ids equal rank by rank, except that ranks whose model weights differ by less
than 1e-12 W -- which such a reordering of the sums can swap -- are compared as a set (a set cut by the end of the list: as a subset).
"""
import ctypes as C

import numpy as np
import pytest

import edge_scenes
import matte_model as mm
import oracle_ffi
from fujiyama_renderer_amd import ffi, gpu, workloads
from test_gpu_aov import RAGGED, SceneView, all_tiles, prepare, sampler_margin, shader_slot, ulp32

pytestmark = pytest.mark.gpu

KEYS = {"instance": mm.KEY_INSTANCE, "shader": mm.KEY_SHADER}
SENTINEL = dict(ids=-77, coverage=-7.5, rest=-7.5, distinct=-77)
TIE = 1e-12
FIGURES = dict(worst=0.0, set_pixels=0, pixels=0)          # the worst filtered deviation in units of its bound, the set-compared pixels


class Case(object):
    """a scene on the device and the oracle's trace of every tile's camera rays (it depends on neither key, ranks nor mode), taken at once:
    the device scene copied the description, the oracle reads the host's, which the next prepare() replaces"""

    def __init__(self, text, render=False):
        self.sp, self.rd = prepare(text)
        self.view = SceneView(self.sp)
        self.gs = gpu.Scene(self.sp)
        osc = oracle_ffi.OracleScene(self.sp)
        self.traces = {t: osc.trace(self.view.target_group, self.gs.camera_samples(self.rd, t))[1] for t in all_tiles(self.rd)}
        self.oracle_frame = osc.render(self.rd)[0] if render else None
        osc.close()

    def close(self):
        self.gs.close()

    def expected(self, key, ranks, filtered, tile_ids=None, prefill=None):
        rd = self.rd
        tiles = all_tiles(rd) if tile_ids is None else tile_ids
        out = None
        if prefill is not None:
            H, W = rd.yres, rd.xres
            out = dict(ids=np.full((H, W, ranks), prefill["ids"], np.int32), coverage=np.full((H, W, ranks), prefill["coverage"], np.float32),
                       rest=np.full((H, W, 1), prefill["rest"], np.float32), distinct=np.full((H, W, 1), prefill["distinct"], np.int32))
        return mm.expected_matte(gpu.lib(), self.gs, None, self.view, rd, {int(t): gpu.tile_rect(rd, int(t)) for t in tiles},
                                 sampler_margin(rd), KEYS[key], ranks, filtered, shader_slot, out=out, traces=self.traces)

    def check(self, key, ranks, filtered, **kw):
        """the pass against the model -> (device buffers, stats, expected)"""
        got, st = self.gs.render_matte(self.rd, key=key, ranks=ranks, filtered=bool(filtered))
        exp, n_rays = self.expected(key, ranks, filtered)
        full = self.expected(key, ffi.MATTE_MAX_RANKS, filtered)[0] if filtered and ranks < ffi.MATTE_MAX_RANKS else exp
        assert_matte(got, exp, filtered, full, **kw)
        assert st.rays.camera == n_rays and st.rays.total() == n_rays
        return got, st, exp


def assert_matte(got, exp, filtered, full=None, where=None):
    """the bounds of the module's docstring; full: the model with FJGPU_MATTE_MAX_RANKS ranks (the weights behind the end of the list);
    where: a mask of the pixels to compare (None: all)"""
    K = exp["ids"].shape[2]
    for name, dtype in (("ids", np.int32), ("coverage", np.float32), ("rest", np.float32), ("distinct", np.int32)):
        assert got[name].dtype == dtype and got[name].shape == exp[name].shape, name
    m = np.ones(exp["W"].shape, dtype=bool) if where is None else where
    assert np.array_equal(got["distinct"][m], exp["distinct"][m])
    if not filtered:
        for name in ("ids", "coverage", "rest"):
            assert np.array_equal(got[name][m], exp[name][m]), name
        return
    full = exp if full is None else full
    assert full["distinct"].max() <= full["ids"].shape[2]            # (every key's weight is in `full`)
    worst = 0.0
    for name in ("coverage", "rest"):
        err = np.abs(got[name].astype(np.float64) - exp[name].astype(np.float64))[m]
        bound = (ulp32(exp[name]) + 1e-12)[m]
        worst = max(worst, float((err / bound).max()))
        print("matte %-8s max |err| %.3e, worst err / bound %.3f" % (name, float(err.max()), float((err / bound).max())))
        assert (err <= bound).all(), (name, float(err.max()))
    # ids: rank by rank; runs of ranks the model holds within TIE x W of each other as sets
    A, W = full["A"], full["W"]
    near = (np.abs(A[:, :, :-1] - A[:, :, 1:]) < TIE * W[:, :, None]) & (A[:, :, 1:] >= 0)
    plain = m & ~near.any(axis=2)
    assert np.array_equal(got["ids"][plain], exp["ids"][plain])
    n_set = 0
    for y, x in zip(*np.nonzero(m & near.any(axis=2))):
        n_set += 1
        a = 0
        while a < K:
            b = a + 1
            while b < A.shape[2] and near[y, x, b - 1]:
                b += 1
            g, e = got["ids"][y, x, a:min(b, K)].tolist(), full["ids"][y, x, a:b].tolist()
            assert len(set(g)) == len(g) and set(g) <= set(e) and (b > K or set(g) == set(e)), (y, x, g, e)
            a = b
    print("matte ids: %d of %d pixels compared as sets" % (n_set, int(m.sum())))
    FIGURES["worst"] = max(FIGURES["worst"], worst)
    FIGURES["set_pixels"] += n_set
    FIGURES["pixels"] += int(m.sum())
    print("so far in this module: worst filtered deviation %.3f of the bound, %d of %d pixels compared as sets"
          % (FIGURES["worst"], FIGURES["set_pixels"], FIGURES["pixels"]))


@pytest.fixture(scope="module")
def ragged(asset_dir):
    case = Case(workloads.buddhas(asset_dir, **RAGGED))
    yield case
    case.close()


@pytest.mark.parametrize("filtered", [0, 1])
@pytest.mark.parametrize("key", ["instance", "shader"])
def test_ragged_frame_matches_model(ragged, key, filtered):
    """several transformed instances, ragged last tiles (40 x 24 in 16 x 16 tiles), 3 x 2 spp, filter width 2 (a 7 x 4 window), jitter"""
    rd = ragged.rd
    assert gpu.tile_count(rd) == 6 and sampler_margin(rd) == (2, 1) and (rd.rate_x, rd.rate_y) == (3, 2) and rd.jitter == 1
    got, st, exp = ragged.check(key, 4, filtered)
    d = got["distinct"][:, :, 0]
    assert (d >= 2).sum() > 50 and (d == 0).sum() > 50
    assert len(set(got["ids"][got["ids"] >= 0].tolist())) > 4                  # several instances / several shaders
    assert (got["ids"][d == 0] == -1).all() and not got["coverage"][d == 0].any()
    assert st.batches == 1 and st.resolve_ms > 0


@pytest.mark.parametrize("filtered", [0, 1])
def test_more_keys_than_ranks(asset_dir, filtered):
    """64 instances in 24 x 16 pixels at 3 x 3 spp: pixels see more than 2 instances (the oracle's trace: up to 4 among a pixel's own
    samples, up to 7 in its window), so with 2 ranks `rest` is what the two greatest shares leave"""
    case = Case(workloads.crowd(asset_dir, res=(24, 16), spp=(3, 3), mesh="tiny", n=64))
    try:
        got2, _, exp2 = case.check("instance", 2, filtered)
        got8, _, exp8 = case.check("instance", 8, filtered)
    finally:
        case.close()
    many = exp2["distinct"][:, :, 0] > 2
    assert many.sum() > 20 and exp8["distinct"].max() <= 8
    assert (got2["rest"][many] > 0).all() and not got8["rest"].any()
    assert np.array_equal(got2["distinct"], got8["distinct"])
    # the two greatest shares are the first two of the longer list (ties at the cut aside: the model's lists agree there too)
    same = (exp2["ids"] == exp8["ids"][:, :, :2]).all(axis=2)
    assert same.mean() > .9
    assert np.array_equal(got2["coverage"][same], got8["coverage"][:, :, :2][same])
    assert (got8["coverage"][:, :, :-1] >= got8["coverage"][:, :, 1:]).all()


WINDOW_CASES = {
    # 19 x 16 = 304 samples a window (72 own): the lanes loop, past the samples they keep in registers
    "over_64": dict(res=(8, 6), spp=(9, 8), extra=(("filterwidth", (2, 2)),)),
    "one": dict(res=(24, 16), spp=(1, 1), extra=(("filterwidth", (1, 1)), ("sample_jitter", (0,)))),
    "two_by_two": dict(res=(24, 16), spp=(2, 2), extra=(("sample_jitter", (0,)),)),
}


@pytest.mark.parametrize("filtered", [0, 1])
@pytest.mark.parametrize("name", sorted(WINDOW_CASES))
def test_window_sizes(asset_dir, name, filtered):
    case = Case(workloads.buddhas(asset_dir, mesh="tiny", **WINDOW_CASES[name]))
    try:
        rd = case.rd
        mx, my = sampler_margin(rd)
        nwin = (rd.rate_x + 2 * mx) * (rd.rate_y + 2 * my)
        got, st, exp = case.check("instance", 4, filtered)
    finally:
        case.close()
    if name == "over_64":
        assert nwin == 19 * 16 > 256 and rd.rate_x * rd.rate_y == 72
    if name == "one":
        assert nwin == 1 and rd.jitter == 0
        assert set(np.unique(got["coverage"]).tolist()) == {0.0, 1.0} and got["distinct"].max() == 1 and not got["rest"].any()
    if name == "two_by_two":
        assert rd.jitter == 0
        c = got["coverage"]
        if filtered:
            # unjittered samples lie symmetric about the pixel's centre: equal weights, the set comparison's case
            A, W = exp["A"], exp["W"]
            assert ((np.abs(A[:, :, 0] - A[:, :, 1]) < TIE * W) & (A[:, :, 1] >= 0)).sum() > 3
        else:
            split = (c[:, :, 0] == .5) & (c[:, :, 1] == .5)
            assert split.sum() > 10
            assert (got["ids"][:, :, 0][split] < got["ids"][:, :, 1][split]).all()      # an exact tie: ascending key


@pytest.mark.parametrize("key", ["instance", "shader"])
def test_curves(asset_dir, key):
    """the scene of test_gpu_aov.py::test_curves: a curve hit's shading group is 0"""
    case = Case(workloads.furry(asset_dir, res=(32, 24), spp=(2, 2), mesh="furball", nlights=1))
    try:
        curves = [k for k, I in enumerate(case.view.instances) if I["curve"]]
        got, _, _ = case.check(key, 4, 1)
        got0, _, _ = case.check(key, 4, 0)
    finally:
        case.close()
    assert curves
    want = set(curves) if key == "instance" else {shader_slot(case.view.instances[k], 0) for k in curves}
    for g in (got, got0):
        assert want <= set(g["ids"].ravel().tolist()) and g["distinct"].max() >= 2


@pytest.mark.parametrize("filtered", [0, 1])
def test_face_groups_select_the_shader(asset_dir, filtered):
    """the OBJ mesh of test_gpu_aov.py's shader-slot test: face groups with an unassigned slot and an id past the end of the instance's
    shader list; the shader key follows every sample's own face group"""
    case = Case(edge_scenes.custom_scene(asset_dir, **edge_scenes.EDGE_CASES["obj_face_groups"]))
    try:
        got, _, _ = case.check("shader", 4, filtered)
        goti, _, _ = case.check("instance", 4, filtered)
    finally:
        case.close()
    obj = [k for k, I in enumerate(case.view.instances) if not I["curve"] and case.view.meshes[I["primset"]]["fg"] is not None
           and case.view.meshes[I["primset"]]["fg"].max() > 0]
    assert len(obj) == 1
    I = case.view.instances[obj[0]]
    only = (goti["distinct"][:, :, 0] == 1) & (goti["ids"][:, :, 0] == obj[0])          # pixels that see this instance alone ...
    assert only.sum() > 20 and got["distinct"][only].max() >= 2                          # ... and yet several of its shaders
    assert {I["shaders"][0], I["shaders"][1]} <= set(got["ids"][only].ravel().tolist())


def test_tile_subset_prefill_and_batches(ragged):
    """listed tiles (in reverse order) correct, every other pixel keeps the sentinels; one tile per batch gives the same bits"""
    gs, rd = ragged.gs, ragged.rd
    subset = all_tiles(rd)[::-1][::2]
    assert 1 < len(subset) < gpu.tile_count(rd)
    touched = np.zeros((rd.yres, rd.xres), dtype=bool)
    for t in subset:
        x0, y0, x1, y1 = gpu.tile_rect(rd, t)
        touched[y0:y1, x0:x1] = True
    for filtered in (0, 1):
        got, st = gs.render_matte(rd, key="shader", ranks=3, filtered=bool(filtered), tile_ids=subset, prefill=SENTINEL)
        exp, n_rays = ragged.expected("shader", 3, filtered, tile_ids=subset, prefill=SENTINEL)
        assert_matte(got, exp, filtered, ragged.expected("shader", 16, 1, tile_ids=subset)[0] if filtered else None, where=touched)
        for name in gpu.MATTE_NAMES:
            assert (got[name][~touched] == np.full((), SENTINEL[name], dtype=got[name].dtype)).all(), name
            assert (got[name][touched] != np.full((), SENTINEL[name], dtype=got[name].dtype)).all(), name
        assert st.rays.camera == n_rays and st.batches == 1
        whole, st1 = gs.render_matte(rd, key="shader", ranks=3, filtered=bool(filtered))
        gs.set_option("aov_batch_samples", 1)
        try:
            again, stn = gs.render_matte(rd, key="shader", ranks=3, filtered=bool(filtered))
        finally:
            gs.set_option("aov_batch_samples", 0)
        assert stn.batches == gpu.tile_count(rd) >= 3 and stn.rays.camera == st1.rays.camera
        for name in gpu.MATTE_NAMES:
            assert np.array_equal(again[name], whole[name]), name
            assert np.array_equal(got[name][touched], whole[name][touched]), name


def test_own_mode_agrees_with_render_aov(ragged):
    """ranks >= distinct: the ranks' counts add up to render_aov's hit count, and its nearest sample's instance is among them"""
    gs, rd = ragged.gs, ragged.rd
    nown = rd.rate_x * rd.rate_y
    got, _ = gs.render_matte(rd, key="instance", ranks=16, filtered=False)
    aov, _ = gs.render_aov(rd, want=("ids", "coverage"))
    assert got["distinct"].max() <= 16 and not got["rest"].any()
    counts = np.round(got["coverage"].astype(np.float64) * nown)
    assert np.array_equal(counts.sum(axis=2), np.round(aov["coverage"][:, :, 0].astype(np.float64) * nown))
    assert np.array_equal((got["ids"] >= 0).sum(axis=2), got["distinct"][:, :, 0])
    hit = aov["ids"][:, :, 0] >= 0
    assert hit.sum() > 100 and (got["ids"][hit] == aov["ids"][:, :, 0][hit][:, None]).any(axis=1).all()
    assert np.array_equal(hit, got["distinct"][:, :, 0] > 0)


def test_filtered_shares_add_up_to_the_beauty_alpha(asset_dir):
    """An opaque scene (plastic at opacity 1, a constant-shader dome): a sample's alpha is 1 on a hit and 0 on a miss, so the beauty pixel's
    alpha is the hit share of its window, sum(coverage) + rest.  Bound: 2e-7 + one f32 ulp of every share added.  2e-7 is what the oracle's
    frame -- the reference's arithmetic: f64 products added into f32 accumulators, 28 of them here -- differs from the f64 model by on this
    frame (measured without a device: 1.916e-07, asserted below as the premise; it also shows that alpha is 1 / 0 per sample)."""
    case = Case(workloads.buddhas(asset_dir, **RAGGED), render=True)
    try:
        gs, rd = case.gs, case.rd
        fb, _ = gs.render_frame(rd)
        got, _ = gs.render_matte(rd, key="instance", ranks=4, filtered=True)
        full = case.expected("instance", 16, 1)[0]
    finally:
        case.close()
    share = np.where(full["A"] >= 0, full["A"], 0).sum(axis=2) / full["W"]
    ref = case.oracle_frame
    premise = float(np.abs(ref[:, :, 3].astype(np.float64) - share).max())
    print("oracle frame alpha against the model's hit share: max |diff| %.3e" % premise)
    assert premise <= 2e-7
    total = got["coverage"].astype(np.float64).sum(axis=2) + got["rest"][:, :, 0]
    bound = 2e-7 + ulp32(got["coverage"]).sum(axis=2) + ulp32(got["rest"][:, :, 0])
    err = np.abs(fb[:, :, 3].astype(np.float64) - total)
    print("beauty alpha against sum(coverage) + rest: max |err| %.3e, worst err / bound %.3f" % (float(err.max()), float((err / bound).max())))
    assert ((total > 0) & (total < 1)).sum() > 50
    assert (err <= bound).all()


def test_matte_select_on_device_tensors(ragged):
    import torch
    t, _ = ragged.gs._render_matte_device(ragged.rd, key="instance", ranks=4, filtered=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in t.values())
    ids, cov = t["ids"].cpu().numpy(), t["coverage"].cpu().numpy()
    keys = sorted(set(ids[ids >= 0].tolist()))[:3]
    dev = gpu.matte_select(t["ids"], t["coverage"], keys)
    assert dev.is_cuda and dev.shape == ids.shape[:2] and dev.dtype == torch.float32
    host = gpu.matte_select(ids, cov, keys)
    assert host.any() and np.array_equal(dev.cpu().numpy(), host)
    everything = gpu.matte_select(ids, cov, sorted(set(ids[ids >= 0].tolist())))
    assert np.abs(everything - cov.sum(axis=2)).max() <= 4 * 2.0 ** -24


def test_does_not_disturb_rendering(asset_dir):
    """render_frame, render_aov and render_aov_albedo before and after matte calls in one process: bit-identical.  The frame is the
    reproducible one of test_gpu_aov.py::test_does_not_disturb_rendering (one light, no bounces)."""
    kw = dict(RAGGED, nlights=1)
    kw["extra"] = RAGGED["extra"] + (("max_reflect_depth", (0,)), ("max_refract_depth", (0,)))
    sp, rd = prepare(workloads.buddhas(asset_dir, **kw))
    gs = gpu.Scene(sp)
    try:
        fb0, st0 = gs.render_frame(rd)
        aov0, _ = gs.render_aov(rd)
        alb0, _ = gs.render_aov_albedo(rd)
        work0 = gs.query("work_bytes")
        for key in ("instance", "shader"):
            for filtered in (True, False):
                _, stm = gs.render_matte(rd, key=key, ranks=4, filtered=filtered)
                assert stm.rays.camera == st0.rays.camera and stm.closest_launches == stm.batches == 1
        assert gs.query("work_bytes") == work0
        fb1, st1 = gs.render_frame(rd)
        aov1, _ = gs.render_aov(rd)
        alb1, _ = gs.render_aov_albedo(rd)
    finally:
        gs.close()
    assert fb0.any() and np.array_equal(fb0, fb1) and st0.rays.as_dict() == st1.rays.as_dict()
    for name in aov0:
        assert np.array_equal(aov0[name], aov1[name]), name
    for name in alb0:
        assert np.array_equal(alb0[name], alb1[name]), name


def test_refusals(asset_dir):
    """the AOV pass's refusals under this entry's name, and its own: each with its error code, the reason naming fjgpu_render_aov_matte"""
    sp, rd = prepare(workloads.buddhas(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny", extra=(("sampler_type", (1,)),)))
    gs = gpu.Scene(sp)
    with pytest.raises(gpu.GpuError, match=r"error -3: fjgpu_render_aov_matte: the adaptive sampler"):
        gs.render_matte(rd)
    gs.close()
    sp, rd = prepare(workloads.motion(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny", kind="object"))
    gs = gpu.Scene(sp)
    with pytest.raises(gpu.GpuError, match=r"error -3: fjgpu_render_aov_matte: a scene with motion"):
        gs.render_matte(rd)
    gs.close()
    sp, rd = prepare(workloads.buddhas(asset_dir, res=(16, 12), spp=(1, 1), mesh="tiny"))
    gs = gpu.Scene(sp)
    try:
        for ranks in (0, 17):
            with pytest.raises(gpu.GpuError, match=r"error -2: fjgpu_render_aov_matte: ranks %d outside 1\.\.16" % ranks):
                gs.render_matte(rd, ranks=ranks)
        with pytest.raises(gpu.GpuError, match=r"error -2: fjgpu_render_aov_matte: unknown key 2"):
            gs.render_matte(rd, key=2)
        with pytest.raises(ValueError):
            gs.render_matte(rd, key="object")
        import torch
        L = gpu.lib()
        desc = ffi.MatteDesc(0, 4, 1, 0)
        ids = torch.zeros((rd.yres, rd.xres, 4), dtype=torch.int32, device="cuda")
        cov = torch.zeros((rd.yres, rd.xres, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for bufs, d in ((None, desc), (ffi.MatteBuffers(), desc), (ffi.MatteBuffers(ids=ids.data_ptr()), desc),
                        (ffi.MatteBuffers(coverage=cov.data_ptr()), desc), (ffi.MatteBuffers(ids=ids.data_ptr(), coverage=cov.data_ptr()), None)):
            rc = L.fjgpu_render_aov_matte(gs._h, C.byref(rd), None, 0, None if d is None else C.byref(d), None if bufs is None else C.byref(bufs),
                                          None, None)
            assert rc == -2 and "fjgpu_render_aov_matte" in L.fjgpu_last_error().decode()
            assert ("null" in L.fjgpu_last_error().decode().lower())
        assert not ids.any() and not cov.any()
        got, _ = gs.render_matte(rd, ranks=16)          # (the largest rank count is served)
        assert got["ids"].shape == (rd.yres, rd.xres, 16)
    finally:
        gs.close()
