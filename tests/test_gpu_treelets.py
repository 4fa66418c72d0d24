"""GPU suite, SAH treelet restructuring of the device-built BLAS (-m gpu): global option "blas_treelet_passes" / environment
FJGPU_TREELET_PASSES, scene queries "blas_treelet_passes", "blas_treelets_changed", "blas_sah_cost_initial", "blas_sah_cost"
(fjgpu_lbvh.hip: k_treelet_pass between tree formation and the collapse).

Closest hits do not depend on the culling structure, so every tree is checked bit for bit against the reference's grid vectors or
the CPU oracle; the cost figures are checked against the model the pass optimises (the collapse's leaf rule):
  C(triangle) = A,  C(inner) = min(trav A + C(l) + C(r), A count where count <= 4),  A = half area,  reported C(root) / A(root).
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import golden_io
import oracle_ffi
import pathological_meshes as pm
import test_gpu_parity as tg
from test_gpu_pathological import builder, family_case, gpu_trace
from fujiyama_renderer_amd import gpu, host, workloads

pytestmark = pytest.mark.gpu

REL_TOL = tg.REL_TOL
ENV = ("FJGPU_TREELET_PASSES", "FJGPU_TRAV_COST", "FJGPU_PLOC_TOP", "FJGPU_PLOC_RADIUS")
QUERIES = ("blas_treelet_passes", "blas_treelets_changed", "blas_sah_cost_initial", "blas_sah_cost", "blas_nodes", "stack_need")
TRAV = float(np.float32(1.2))       # the builder's node-step cost (FJGPU_TRAV_COST unset)
MAX_LEAF = 4                        # FJ_MAX_LEAF_PRIMS


@contextmanager
def treelets(how, passes, monkeypatch):
    """scenes created inside are built by `how` (test_gpu_pathological.BUILDERS) with `passes` treelet passes; None leaves the
    option alone.  The environment is cleared first, option and builder are restored on exit."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    try:
        if passes is not None:
            gpu.global_option("blas_treelet_passes", passes)
        with builder(how, monkeypatch):
            yield
    finally:
        gpu.global_option("blas_treelet_passes", 0)
        gpu.global_option("device_build", -1)


def golden_trace(asset_dir, golden_dir):
    """the 20 000-triangle golden mesh traced with the golden rays: t, ids, the scene's figures, nodes visited"""
    import test_oracle_golden as og
    sp, _ = tg.prepare(og._mesh_scene(asset_dir))
    rays = np.load(os.path.join(golden_dir, "mesh_trace_rays.npy"))
    gs = gpu.Scene(sp)
    gs.set_option("count_nodes", 1)
    facts = {k: gs.query(k) for k in QUERIES}
    t, ids, uv, st = gs.trace(0, rays)
    gs.close()
    facts["nodes_visited"] = int(st.nodes_visited)
    return t, ids, facts


@pytest.fixture(scope="module")
def vectors(golden_dir):
    return golden_io.read_vectors(os.path.join(golden_dir, "ref_vectors.bin"))


@pytest.fixture(scope="module", autouse=True)
def untouched(asset_dir, golden_dir):
    """blas_nodes / nodes_visited of the golden mesh on both device builders, taken before any test of this module touches the
    option (no other module does)"""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for how in ("radix", "ploc_root_r16"):
            with treelets(how, None, mp):
                out[how] = golden_trace(asset_dir, golden_dir)[2]
    finally:
        mp.undo()
    return out


# ---------------------------------------------------------------------------------------------------------- 1. off means today
@pytest.mark.parametrize("how", ["radix", "ploc_root_r16"])
def test_zero_passes_build_todays_tree(how, asset_dir, golden_dir, vectors, untouched, monkeypatch):
    with treelets(how, 0, monkeypatch):
        t, ids, f = golden_trace(asset_dir, golden_dir)
    assert np.array_equal(t, vectors["grid_t"]) and np.array_equal(ids[:, 1], vectors["grid_prim"])
    assert f["blas_treelets_changed"] == 0 and f["blas_treelet_passes"] == 0
    assert f["blas_sah_cost"] == f["blas_sah_cost_initial"] > 0
    assert f["blas_nodes"] == untouched[how]["blas_nodes"] and f["nodes_visited"] == untouched[how]["nodes_visited"]
    assert f["stack_need"] == untouched[how]["stack_need"]


# ----------------------------------------------------------------------------------------------------- 2. optimum on a whole tree
def model_optimum(verts, tris):
    """the cheapest binary tree over the triangles' boxes in the cost model, by dynamic programming over the subsets (f64),
    over the half area of all of them.  Boxes as the builder makes them: f32 bounds one ulp outward."""
    p = verts[tris]                                           # [k, 3, 3] f32
    lo = np.nextafter(p.min(axis=1), np.float32(-np.inf)).astype(np.float64)
    hi = np.nextafter(p.max(axis=1), np.float32(np.inf)).astype(np.float64)
    k = len(tris)
    area, cost = np.zeros(1 << k), np.zeros(1 << k)
    for s in range(1, 1 << k):
        m = [j for j in range(k) if s >> j & 1]
        d = hi[m].max(axis=0) - lo[m].min(axis=0)
        area[s] = d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    for s in sorted(range(1, 1 << k), key=lambda s: bin(s).count("1")):
        size = bin(s).count("1")
        if size == 1:
            cost[s] = area[s]
            continue
        best, q = np.inf, (s - 1) & s
        while q:
            best = min(best, cost[q] + cost[s ^ q])
            q = (q - 1) & s
        cost[s] = TRAV * area[s] + best
        if size <= MAX_LEAF:
            cost[s] = min(cost[s], area[s] * size)
    return cost[-1] / area[-1]


def tiny_facts(k, passes, tmp_path, monkeypatch):
    v, t = pm.tiny(k)
    assert v.dtype == np.float32
    path = pm.write_mesh(tmp_path, "tiny%d" % k, v, t)
    with treelets("radix", passes, monkeypatch):
        sp, _ = tg.prepare(pm.trace_scene(path))
        gs = gpu.Scene(sp)
        f = {q: gs.query(q) for q in QUERIES}
        gs.close()
    return f, model_optimum(v, t)


def test_seven_triangles_reach_the_model_optimum(tmp_path, monkeypatch):
    """7 triangles: the treelet of the root is the entire tree, so one pass leaves the optimum of the model over ALL binary trees
    (1e-4 relative: f32 area arithmetic on extents ~0.3 at coordinates ~2 is ~1e-6 per box)"""
    f, best = tiny_facts(7, 1, tmp_path, monkeypatch)
    print("tiny7", f, "model optimum", best)
    assert f["blas_treelet_passes"] == 1
    assert abs(f["blas_sah_cost"] - best) <= 1e-4 * best
    assert f["blas_sah_cost"] <= f["blas_sah_cost_initial"] * (1 + 1e-5)
    assert (f["blas_treelets_changed"] > 0) == (f["blas_sah_cost"] != f["blas_sah_cost_initial"])


def test_six_triangles_have_no_treelet(tmp_path, monkeypatch):
    f, best = tiny_facts(6, 1, tmp_path, monkeypatch)
    print("tiny6", f, "model optimum", best)
    assert f["blas_treelets_changed"] == 0 and f["blas_sah_cost"] == f["blas_sah_cost_initial"] > 0
    assert f["blas_sah_cost"] >= best * (1 - 1e-4)


def test_eight_triangles_do_not_get_worse(tmp_path, monkeypatch):
    f, best = tiny_facts(8, 1, tmp_path, monkeypatch)
    print("tiny8", f, "model optimum", best)
    assert 0 < f["blas_sah_cost"] <= f["blas_sah_cost_initial"]
    assert f["blas_sah_cost"] >= best * (1 - 1e-4)


# ----------------------------------------------------------------------------------- 3. never worse, always the oracle's hits
FOUR_BUILDERS = ("radix", "ploc_root_r16", "ploc_hybrid64", "ploc_default")
CASES = [(name, how, 3) for name in sorted(pm.FAMILIES) for how in FOUR_BUILDERS]
CASES += [(name, how, passes) for name in ("blocks257", "blocks4099", "flat_sheet_y", "same_centroid") for how in FOUR_BUILDERS for passes in (1, 8)]


def check_figures(f, passes):
    # the DP compares f32 sums of <= 13 terms (~8e-7 relative), the report is f64
    assert f["blas_sah_cost"] <= f["blas_sah_cost_initial"] * (1 + 1e-5)
    assert 0 <= f["blas_treelet_passes"] <= passes
    assert (f["blas_treelets_changed"] == 0) <= (f["blas_sah_cost"] == f["blas_sah_cost_initial"])


@pytest.mark.parametrize("name,how,passes", CASES)
def test_restructured_trees_give_the_oracles_hits(name, how, passes, tmp_path, monkeypatch):
    path, rays, to, io = family_case(name, tmp_path)
    with treelets(how, passes, monkeypatch):
        sp, _ = tg.prepare(pm.trace_scene(path))
        gs = gpu.Scene(sp)
        t, ids, uv, st = gs.trace(0, rays)
        f = {q: gs.query(q) for q in QUERIES}
        gs.close()
    print(name, how, passes, f)
    assert np.array_equal(t, to)
    assert np.array_equal(ids, io)
    check_figures(f, passes)
    if len(pm.FAMILIES[name]()[1]) >= 7:
        assert f["blas_treelet_passes"] >= 1 and f["blas_sah_cost_initial"] > 0


@pytest.fixture(scope="module")
def dup_case(tmp_path_factory):
    path, rays, tied, winner = pm.duplicate_ties(tmp_path_factory.mktemp("dup_treelets"))
    to, io = pm.oracle_trace(pm.trace_scene(path), rays)
    assert tied.sum() >= 200
    return path, rays, tied, winner, to, io


@pytest.mark.parametrize("how", ["radix", "ploc_root_r16"])
def test_ties_still_go_to_the_largest_id(how, dup_case, monkeypatch):
    path, rays, tied, winner, to, io = dup_case
    with treelets(how, 3, monkeypatch):
        t, ids, _ = gpu_trace(pm.trace_scene(path), rays)
    assert np.array_equal(ids[tied, 1], winner[tied])
    assert np.array_equal(t, to) and np.array_equal(ids, io)


# ------------------------------------------------------------------------------------------------------- 4. it does something
@pytest.mark.parametrize("how", ["radix", "ploc_root_r16"])
def test_three_passes_lower_the_cost_of_the_golden_mesh(how, asset_dir, golden_dir, vectors, untouched, monkeypatch):
    """20 000 triangles, 3 passes: treelets are rewritten and the reported cost falls; on the radix tree the golden rays visit no
    more nodes than in the tree as formed.  (Clustering tree: the ratios are printed, only never-worse is asserted.)"""
    with treelets(how, 3, monkeypatch):
        t, ids, f = golden_trace(asset_dir, golden_dir)
    base = untouched[how]
    print("golden mesh, %s, 3 passes: SAH cost %.6f -> %.6f (ratio %.4f), nodes visited %d -> %d (ratio %.4f), %d treelets rewritten in %d passes"
          % (how, f["blas_sah_cost_initial"], f["blas_sah_cost"], f["blas_sah_cost"] / f["blas_sah_cost_initial"], base["nodes_visited"],
             f["nodes_visited"], f["nodes_visited"] / base["nodes_visited"], f["blas_treelets_changed"], f["blas_treelet_passes"]))
    assert np.array_equal(t, vectors["grid_t"]) and np.array_equal(ids[:, 1], vectors["grid_prim"])
    assert f["blas_sah_cost_initial"] == base["blas_sah_cost_initial"]
    assert f["blas_sah_cost"] <= f["blas_sah_cost_initial"] * (1 + 1e-5)
    if how == "radix":
        assert f["blas_treelets_changed"] > 0
        assert f["blas_sah_cost"] < f["blas_sah_cost_initial"]
        assert f["nodes_visited"] <= base["nodes_visited"]


# ------------------------------------------------------------------------------------------------------------------- 5. frames
@pytest.mark.parametrize("how", ["radix", "ploc_root_r16"])
def test_frames_on_restructured_trees(how, asset_dir, monkeypatch):
    """a static scene and one with vertex velocities + object motion (swept boxes) on trees after 3 passes"""
    with treelets(how, 3, monkeypatch):
        for text in (workloads.dragon(asset_dir, res=(96, 54), spp=(3, 3), mesh="small"),
                     workloads.motion(asset_dir, res=(64, 48), spp=(2, 2), mesh="tiny", kind="velocity+object")):
            fb, st, ref, rc = tg.render_both(text)
            assert st.rays.as_dict() == rc.as_dict()
            assert float(tg.rel_err(fb, ref).max()) <= REL_TOL


# --------------------------------------------------------------------------------------------------- 6. same tree every time
def test_the_same_tree_in_every_run(asset_dir, golden_dir, monkeypatch):
    runs = []
    with treelets("radix", 3, monkeypatch):
        for _ in range(3):
            f = golden_trace(asset_dir, golden_dir)[2]
            runs.append((f["blas_nodes"], f["stack_need"], f["blas_treelets_changed"], np.float64(f["blas_sah_cost"]).tobytes(), f["nodes_visited"]))
    assert runs[0][2] > 0
    assert runs[0] == runs[1] == runs[2]


# ------------------------------------------------------------------------------------------------------------ 7. through Si*
def test_si_render_scene_with_the_environment_variable(asset_dir, monkeypatch):
    """SiRenderScene builds on the device by itself (single_frame_build); FJGPU_TREELET_PASSES reaches that build"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    gpu.global_option("blas_treelet_passes", 0)
    gpu.global_option("device_build", -1)
    try:
        monkeypatch.setenv("FJGPU_TREELET_PASSES", "3")
        host.run_scene_text(workloads.teapot(asset_dir, res=(64, 64), spp=(2, 2)), deferred=False)
        fb = host.framebuffer(0)
        st = host.last_stats()
        sp, rd = host.get_desc()
        # (the same scene created by hand, as SiRenderScene creates it: the variable is what switches the passes on)
        gpu.global_option("device_build", 1)
        gs = gpu.Scene(sp)
        ran, changed = gs.query("blas_treelet_passes"), gs.query("blas_treelets_changed")
        gs.close()
    finally:
        monkeypatch.delenv("FJGPU_TREELET_PASSES", raising=False)
        gpu.global_option("blas_treelet_passes", 0)
        gpu.global_option("device_build", -1)
    osc = oracle_ffi.OracleScene(sp)
    ref, rc = osc.render(rd)
    osc.close()
    assert float(tg.rel_err(fb, ref).max()) <= REL_TOL
    assert st.rays.as_dict() == rc.as_dict()
    assert ran >= 1 and changed >= 0
