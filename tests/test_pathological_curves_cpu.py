"""The host's view of the curve BLAS (fjgpu_host_curve_blas: the pieces' leaf boxes, f32 capsules, cached split depths, the grid)
against the oracle's per-(ray, curve) ribbon test, on the adversarial sets of pathological_curves.py.  No device needed.

Conservativeness: a walk reaches a curve's ribbon test only through a BLAS slot of that curve whose leaf box the ray enters and
whose capsule it passes.  So for every (ray, curve) pair the oracle reports as a hit, SOME slot of the curve must hold the hit point
o + t d in its leaf box and have its chord within `reach` of the ray's line -- tested here in plain f64 from the geometry, with no
allowance.  (Shrinking `reach` in fjgpu_curve_build.cc by 1 %, or dropping piece_radius from the box pad, fails this file.)
"""
import numpy as np
import pytest

import oracle_ffi
import pathological_curves as pc
from fujiyama_renderer_amd import gpu

SEGDEPTHS = (0, 4, 5)
ALL = sorted(pc.FAMILIES) + sorted(pc.MOVING)


def line_segment_distance(o, d, A, B):
    """distance between the line o + s d and the segment AB, rows of [n, 3] arrays: drop the component along d (the line becomes the
    origin of the plane across it), then the distance from the origin to the projected segment"""
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    a, b = A - o, B - o
    a = a - (a * u).sum(axis=1, keepdims=True) * u
    b = b - (b * u).sum(axis=1, keepdims=True) * u
    e = b - a
    ee = (e * e).sum(axis=1)
    s = np.clip(np.where(ee > 0, -(a * e).sum(axis=1) / np.where(ee > 0, ee, 1.), 0.), 0., 1.)
    return np.linalg.norm(a + s[:, None] * e, axis=1)


_oracle = {}


def oracle_pairs(name, cs, osc):
    """every ray of the family against every curve, by the oracle's Curve::ray_intersect alone (moving sets: at a random time per
    ray) -> rays, kinds, times, hit [n_rays, n_curves], t; computed once per family"""
    if name not in _oracle:
        fam = pc.family(name)
        rays, kinds = pc.base_rays(fam)
        m = len(fam["indices"])
        times = np.random.RandomState(5).uniform(0, 1, size=len(rays)) if fam["velocity"] is not None else np.zeros(len(rays))
        hit, t, _ = osc.curve_ray(0, np.repeat(rays, m, axis=0), np.tile(np.arange(m, dtype=np.int32), len(rays)), np.repeat(times, m))
        _oracle[name] = (rays, kinds, times, hit.reshape(len(rays), m), t.reshape(len(rays), m))
        for a in _oracle[name]:
            a.setflags(write=False)
    return _oracle[name]


@pytest.mark.parametrize("name", ALL)
def test_pieces_are_conservative_and_depths_and_grid_are_the_oracles(name, asset_dir, monkeypatch):
    fam = pc.family(name)
    cs = pc.CurveScene(asset_dir, fam)
    osc = oracle_ffi.OracleScene(cs.sp)
    try:
        rays, kinds, times, hit, t = oracle_pairs(name, cs, osc)
        info = osc.curve_info(0)
    finally:
        osc.close()
    m = len(fam["indices"])
    aimed = kinds == pc.KINDS.index("aimed")
    ray_hit = hit.any(axis=1)
    n_hit, n_miss = int(ray_hit[aimed].sum()), int((~ray_hit[aimed]).sum())
    nan = pc.nan_frame(rays)
    print("%-14s curves %3d  rays %5d  aimed hits %4d misses %4d  hit pairs %6d  NaN-frame rays %3d (hits among them %d)  depths %s" % (
        name, m, len(rays), n_hit, n_miss, int(hit.sum()), int(nan.sum()), int(ray_hit[nan].sum()), np.bincount(info["depth"], minlength=6)[1:]))
    # the test is not vacuous: the aimed rays straddle the ribbons' edges -- or the family cannot be hit at all
    if name in pc.NO_HITS:
        assert int(hit[~nan].sum()) == 0
    elif name in pc.FAMILIES:
        assert n_hit >= pc.HIT_FLOOR and n_miss >= pc.HIT_FLOOR, (n_hit, n_miss)
    # a NaN frame (x and y of ray space are NaN, z is not): no comparison rejects, so Curve::ray_intersect itself reports a "hit" for
    # curves in front of the origin -- with t = NaN (or REAL_MAX where the other half of a split missed: `t_left < t_right` is false
    # and the miss's REAL_MAX is taken), which the caller's tmin <= t <= tmax and the grid's cell rule then refuse.  Never a t on the ray.
    t_nan = t[nan][hit[nan]]
    assert nan.sum() >= 150 and np.all(np.isnan(t_nan) | (t_nan == np.finfo(np.float64).max))
    assert np.all(np.isfinite(t[~nan][hit[~nan]])) and np.all(t[~nan][hit[~nan]] < 1e6)

    ri, ci = np.nonzero(hit & ~nan[:, None])
    o, d = rays[ri, 0:3], rays[ri, 3:6]
    p_hit = o + t[ri, ci][:, None] * d
    for seg_depth in SEGDEPTHS:
        monkeypatch.setenv("FJGPU_CURVE_SEGDEPTH", str(seg_depth))
        blas = gpu.host_curve_blas(cs.sp, 0)
        S = 1 << seg_depth
        assert len(blas["curve"]) == m * S and np.array_equal(np.bincount(blas["curve"], minlength=m), np.full(m, S))
        # split depth and grid: the oracle's, for every slot
        assert np.array_equal(blas["depth"], info["depth"][blas["curve"]]), seg_depth
        assert np.array_equal(blas["grid_n"], info["grid_n"]) and np.array_equal(blas["grid_cell"], info["grid_cell"])
        assert np.array_equal(blas["bounds"], info["bounds"])
        assert np.all(blas["box"][:, :3] <= blas["box"][:, 3:]) and np.all(np.isfinite(blas["box"]))
        if fam["velocity"] is not None:
            assert np.all(np.isinf(blas["reach"]))
        else:
            assert np.all(np.isfinite(blas["reach"])) and np.all(blas["reach"] > 0)
        if not len(ri):
            continue
        slots = np.argsort(blas["curve"], kind="stable").reshape(m, S)          # the S slots of every curve
        ok = np.zeros(len(ri), dtype=bool)
        for k in range(S):
            s = slots[ci, k]
            box = blas["box"][s].astype(np.float64)
            inside = np.all((box[:, :3] <= p_hit) & (p_hit <= box[:, 3:]), axis=1)
            dist = line_segment_distance(o, d, blas["A"][s].astype(np.float64), blas["B"][s].astype(np.float64))
            ok |= inside & (dist <= blas["reach"][s].astype(np.float64))
        bad = np.flatnonzero(~ok)
        assert len(bad) == 0, "segdepth %d: %d of %d hit pairs have no slot that admits them, first (ray %d, curve %d, kind %s)" % (
            seg_depth, len(bad), len(ri), ri[bad[0]], ci[bad[0]], pc.KINDS[kinds[ri[bad[0]]]])


def test_bounds_helper_restates_the_hosts_compute_bounds(asset_dir):
    """pathological_curves.compute_bounds on the stock fur set gives the bounds the host's Curve::ComputeBounds wrote"""
    import ctypes as C
    from fujiyama_renderer_amd import host, workloads
    host.run_scene_text(workloads.furry(asset_dir, res=(32, 24), spp=(1, 1), mesh="furball", nlights=1), deferred=True)
    sp, _ = host.get_desc()
    c = C.cast(sp, C.POINTER(pc._Scene)).contents.curves[0]
    P = np.ctypeslib.as_array(C.cast(c.P, C.POINTER(C.c_double)), shape=(c.n_points, 3))
    w = np.ctypeslib.as_array(C.cast(c.width, C.POINTER(C.c_double)), shape=(c.n_points,))
    ix = np.ctypeslib.as_array(C.cast(c.indices, C.POINTER(C.c_int32)), shape=(c.n_curves,))
    assert np.array_equal(pc.compute_bounds(P, w, ix), np.array(list(c.bounds)))


def test_families_are_what_they_claim():
    f = {n: pc.family(n) for n in ALL}
    cps = lambda s: np.stack([s["P"][s["indices"] + k] for k in range(4)], axis=1)
    for n, s in f.items():
        assert 1 <= len(s["indices"]) <= 64, n
    assert len(f["single"]["indices"]) == 1
    c = cps(f["straight_even"])
    assert np.all(c[:, 0] - 2 * c[:, 1] + c[:, 2] == 0) and np.all(c[:, 1] - 2 * c[:, 2] + c[:, 3] == 0)
    assert np.all(f["zero_width"]["width"] == 0)
    w = f["needle"]["width"]
    ix = f["needle"]["indices"]
    assert np.all((w[ix] == 0) ^ (w[ix + 3] == 0))
    w, ix = f["reverse_taper"]["width"], f["reverse_taper"]["indices"]
    assert np.all(w[ix + 3] == 1000 * w[ix])
    c = cps(f["point"])
    assert np.all(c == c[:, :1])
    c = cps(f["closed_loop"])
    assert np.all(c[:, 0] == c[:, 3])
    c = cps(f["blob"])
    assert np.all(np.linalg.norm(np.diff(c, axis=1), axis=2).sum(axis=1) < f["blob"]["width"][f["blob"]["indices"] + 3])
    c = cps(f["duplicates"])
    assert np.array_equal(c[0::2], c[1::2]) and not np.array_equal(f["duplicates"]["Cd"][0::8], f["duplicates"]["Cd"][4::8])
    ix = f["chained"]["indices"]
    assert np.all(np.diff(ix).reshape(-1)[np.arange(len(ix) - 1) % 5 != 4] == 3)
    assert np.all(f["flat_set"]["P"][:, 1] == 0)
    assert abs(np.linalg.norm(f["far_offset"]["P"].mean(axis=0)) - 1e3) < 30
    assert np.all(f["velocity_zero"]["velocity"] == 0) and np.array_equal(f["velocity_zero"]["P"], f["chained"]["P"])
    v = f["velocity_large"]
    assert np.median(np.linalg.norm(v["velocity"], axis=1)) > 2 * .09
    # on_cell_faces: every inner curve lies on grid planes of the two axes it does not run along
    s = f["on_cell_faces"]
    n, cell, b = pc.grid_of(pc.compute_bounds(s["P"], s["width"], s["indices"]), len(s["indices"]))
    c = cps(s)[8:]
    for i in range(len(c)):
        for a in range(3):
            if a != i % 3:
                k = (c[i, 0, a] - b[a]) / cell[a]
                assert abs(k - round(k)) < 1e-9 and np.all(c[i, :, a] == c[i, 0, a])
