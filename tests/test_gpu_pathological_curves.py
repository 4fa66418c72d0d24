"""GPU suite, adversarial curve sets (-m gpu): the families of pathological_curves.py through the curve BLAS and every curve walk,
against the CPU oracle.  tests/test_pathological_curves_cpu.py shows with the oracle alone that the ray sets hit and graze what they
are meant to, and that the BLAS pieces admit every hit; here the walks themselves run.

Closest hits: every family x four instance transforms x FJGPU_CURVE_SEGDEPTH 0 / 4 / 5 (one box per curve, the default 16 pieces,
32 pieces): hits must not depend on the culling structure.  t is compared bit for bit (NaN equals NaN).  The reference leaves
prim_id of a curve hit at 0, so which of two coincident curves wins shows in a frame's colour only: the `duplicates` frames.
Frames: 48 x 32 at 2 x 2 samples under 1 and 4 point lights, HairShader on the curves; counting and production instantiations alike.
Shadow walks: the options curve_anyhit, inst_lds and compact_squeue on and off."""
import numpy as np
import pytest

import oracle_ffi
import pathological_curves as pc
import test_gpu_parity as tg
from fujiyama_renderer_amd import gpu

pytestmark = pytest.mark.gpu

REL_TOL = tg.REL_TOL
FRAME_FAMILIES = ("duplicates", "chained", "blob", "hairpin", "flat_set", "far_offset", "single")
_trace = {}
_frames = {}


def trace_case(name, xform, asset_dir):
    """the scene of (family, instance transform) and, computed once per session: world rays (the family's base rays through the
    instance matrix plus the tmin / tmax brackets around the hits of a first oracle pass) and the oracle's (t, ids) per group"""
    fam = pc.family(name)
    cs = pc.CurveScene(asset_dir, fam, xform=xform, translate=pc.FRAME_TRANSLATE.get(name, (0, 0, 0)) if xform == "identity" else (.05, -.02, .03))
    key = (name, xform)
    if key not in _trace:
        base, kinds = pc.base_rays(fam)
        world = cs.to_world(base)
        osc = oracle_ffi.OracleScene(cs.sp)
        t0, i0, _ = osc.trace(cs.target_group, world)
        rays = np.concatenate([world, pc.bracket_rays(world, t0, i0[:, 0] == cs.curve_inst)], axis=0)
        assert len(rays) <= 20000
        want = {g: osc.trace(g, rays)[:2] for g in cs.groups()}
        osc.close()
        # object-space directions as the instance level derives them (MatTransformVector with the inverse): after a rotation the
        # +-y rays come back with |dx|, |dz| ~ 1e-17, a frame that is nearly but not exactly degenerate
        mi, dw = cs.Minv, rays[:, 3:6]
        d_obj = np.stack([mi[r, 0] * dw[:, 0] + mi[r, 1] * dw[:, 1] + mi[r, 2] * dw[:, 2] for r in range(3)], axis=1)
        nan = (d_obj[:, 0] == 0) & (d_obj[:, 2] == 0)
        for a in (rays, nan) + tuple(x for v in want.values() for x in v):
            a.setflags(write=False)
        _trace[key] = (rays, nan, want)
    return (cs,) + _trace[key]


@pytest.mark.parametrize("seg_depth", [0, 4, 5])
@pytest.mark.parametrize("xform", sorted(pc.XFORMS))
@pytest.mark.parametrize("name", sorted(pc.FAMILIES))
def test_closest_hits_are_the_oracles(name, xform, seg_depth, asset_dir, monkeypatch):
    monkeypatch.setenv("FJGPU_CURVE_SEGDEPTH", str(seg_depth))
    cs, rays, nan, want = trace_case(name, xform, asset_dir)
    gs = gpu.Scene(cs.sp)
    try:
        assert int(gs.query("closest_kernel")) == 2
        got = {g: gs.trace(g, rays)[:2] for g in cs.groups()}
    finally:
        gs.close()
    assert cs.target_group in want and 0 in want
    for g in cs.groups():
        (t, ids), (to, io) = got[g], want[g]
        assert np.array_equal(ids[:, 0], io[:, 0]), (g, int((ids[:, 0] != io[:, 0]).sum()))
        assert pc.same_t(t, to), (g, int((t != to).sum()))
        mesh_hit = (io[:, 0] >= 0) & (io[:, 0] != cs.curve_inst)
        assert np.array_equal(ids[mesh_hit, 1], io[mesh_hit, 1]), g
    on_curves = int((want[cs.target_group][1][:, 0] == cs.curve_inst).sum())
    if name in pc.NO_HITS or (name, xform) == ("far_offset", "mirrored"):
        # (far_offset mirrored: the reference boxes an instance with the ABSOLUTE scale factors -- merge_sampled_bounds,
        # src/fj_object_instance.cc:313-356 -- so the box of a set 600 units off the mirror plane lies on the wrong side and
        # nothing is ever found; the device must lose these hits too)
        assert on_curves == 0
    else:
        assert on_curves >= pc.HIT_FLOOR, on_curves
    # rays with a NaN frame are in the set (identity: the +-y rays exactly), and the oracle never reports a curve for them
    assert (nan.sum() >= 150 or xform != "identity") and not (want[cs.target_group][1][nan, 0] == cs.curve_inst).any()


def render_case(name, nlights, asset_dir, options=None):
    """(scene, device frame, device stats, oracle frame, oracle counts, facts); counting and production instantiations render alike.
    `options`: global options set while the scene is created and rendered, restored to 1 afterwards.  The oracle's frame is computed once per
    (family, lights)."""
    cs = pc.CurveScene(asset_dir, pc.family(name), translate=pc.FRAME_TRANSLATE.get(name, (0, 0, 0)), nlights=nlights)
    # (curve_anyhit and inst_lds are copied into the scene when it is created, compact_squeue is read at every render call: the options
    # stay set until both frames are rendered)
    for k, v in (options or {}).items():
        gpu.global_option(k, v)
    try:
        gs = gpu.Scene(cs.sp)
        try:
            facts = {k: int(gs.query(k)) for k in ("closest_kernel", "curve_anyhit")}
            gs.set_option("count_nodes", 1)
            fb, st = gs.render_frame(cs.rd)
            gs.set_option("count_nodes", 0)
            fb2, st2 = gs.render_frame(cs.rd)
            facts["work_bytes"] = int(gs.query("work_bytes"))
        finally:
            gs.close()
    finally:
        for k in (options or {}):
            gpu.global_option(k, 1)
    assert st.rays.as_dict() == st2.rays.as_dict()
    assert np.array_equal(fb, fb2) or float(tg.rel_err(fb, fb2).max()) <= 1e-6
    key = (name, nlights)
    if key not in _frames:
        osc = oracle_ffi.OracleScene(cs.sp)
        ref, rc = osc.render(cs.rd)
        osc.close()
        ref.setflags(write=False)
        _frames[key] = (ref, rc.as_dict())
    ref, rc = _frames[key]
    return cs, fb, st, ref, rc, facts


def assert_frame(fb, st, ref, rc):
    assert st.rays.as_dict() == rc, (st.rays.as_dict(), rc)
    assert float(tg.rel_err(fb, ref).max()) <= REL_TOL, float(tg.rel_err(fb, ref).max())


@pytest.mark.parametrize("nlights", [1, 4])
@pytest.mark.parametrize("name", FRAME_FAMILIES + tuple(sorted(pc.MOVING)))
def test_frames_are_the_oracles(name, nlights, asset_dir):
    """ties (`duplicates`: the two curves of a pair differ in colour), chained strands, wide and deep curves, the one-cell-thick
    grid, large coordinates, a set of one, and the motion kernels"""
    cs, fb, st, ref, rc, facts = render_case(name, nlights, asset_dir)
    assert_frame(fb, st, ref, rc)
    assert facts["closest_kernel"] == (3 if name in pc.MOVING else 2)
    assert rc["camera"] > 0 and rc["shadow"] > 0
    if name == "duplicates":
        # the pairs are on screen: the frame differs from the one in which the FIRST curve of every pair is alone
        fam = pc.family(name)
        alone = dict(fam, indices=fam["indices"][0::2])
        cs1 = pc.CurveScene(asset_dir, alone, nlights=nlights)
        osc = oracle_ffi.OracleScene(cs1.sp)
        ref1, _ = osc.render(cs1.rd)
        osc.close()
        assert int((tg.rel_err(ref1, ref) > 1e-2).any(axis=2).sum()) >= 20


def test_zero_velocity_renders_the_static_set(asset_dir):
    """a velocity array of zeros goes through the motion kernels, the moving cell predicate and reach = inf, and gives the static
    family's frame"""
    _, fb_s, st_s, ref_s, rc_s, facts_s = render_case("chained", 4, asset_dir)
    _, fb_v, st_v, ref_v, rc_v, facts_v = render_case("velocity_zero", 4, asset_dir)
    assert facts_s["closest_kernel"] == 2 and facts_v["closest_kernel"] == 3
    assert_frame(fb_v, st_v, ref_v, rc_v)
    assert st_v.rays.as_dict() == st_s.rays.as_dict()
    assert float(tg.rel_err(fb_v, fb_s).max()) <= 1e-6


@pytest.mark.parametrize("option,tol", [("curve_anyhit", 1e-5), ("inst_lds", 1e-5), ("compact_squeue", 1e-6)])
@pytest.mark.parametrize("name", FRAME_FAMILIES)
def test_shadow_walk_options_change_nothing(name, option, tol, asset_dir):
    out = []
    for on in (1, 0):
        cs, fb, st, ref, rc, facts = render_case(name, 4, asset_dir, options={option: on})
        assert_frame(fb, st, ref, rc)
        if option == "curve_anyhit":
            assert facts["curve_anyhit"] == on              # the query reports the kernel that ran
        out.append((fb, st, facts))
    assert rc["shadow"] > 0
    if option == "compact_squeue":
        # the work arena holds one shadow-queue record per possible shadow ray: 56 bytes with the option on, 80 off
        assert out[0][2]["work_bytes"] < out[1][2]["work_bytes"], (out[0][2], out[1][2])
    assert out[0][1].rays.as_dict() == out[1][1].rays.as_dict()
    assert float(tg.rel_err(out[0][0], out[1][0]).max()) <= tol
