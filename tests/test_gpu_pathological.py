"""GPU suite, adversarial inputs (-m gpu): the meshes of pathological_meshes.py through every BLAS builder and every traversal
stack, against the CPU oracle.  tests/test_pathological_meshes_cpu.py shows with the oracle alone that the ray sets hit what they
are meant to hit, so "bit-exact" below is never a comparison of misses.

Builders: the host's binned SAH (device_build 0), the radix tree of the Morton codes (2), and the locally-ordered clustering (1) --
which below 65 536 triangles runs NO round by default (FJGPU_PLOC_TOP: the tree is the host's top tree over the leaves), so it is
also run with FJGPU_PLOC_TOP=1 (rounds down to the root; window radius 1, 16, 128) and FJGPU_PLOC_TOP=64 (hybrid).

Traversal stacks: a walk keeps FJ_STACK_LDS* entries per lane in LDS and the rest in the global overflow area
(DScene.stack_overflow / stack_overflow_shadow).  The queries stack_peak_closest / stack_peak_shadow (counting instantiations) say
how many entries a lane held at most: above the walk's LDS figure means the overflow area was written and read back.
"""
import numpy as np
import pytest

import oracle_ffi
import pathological_meshes as pm
import test_gpu_parity as tg
from fujiyama_renderer_amd import gpu, synth

pytestmark = pytest.mark.gpu

REL_TOL = tg.REL_TOL

# entries per lane in LDS (fjgpu_types.h; the scene query "stack_lds*" reports the built values, checked below)
STACK_LDS = 32            # FJ_STACK_LDS: k_trace_closest, k_trace_closest_phased, k_trace_closest_flat, k_shadow_trace
STACK_LDS_ANYHIT = 12     # FJ_STACK_LDS_ANYHIT: k_shadow_anyhit (lean any-hit walk)
STACK_LDS_CANYHIT = 16    # FJ_STACK_LDS_CANYHIT (fjgpu_dev_anyhit_curves.h): k_shadow_anyhit_curves
STACK_LDS_CURVES = 20     # FJ_STACK_LDS_CURVES: the curve instantiations of k_trace_closest / k_shadow_trace

PLOC_ENV = ("FJGPU_PLOC_TOP", "FJGPU_PLOC_RADIUS")
BUILDERS = {
    "host_sah": (0, {}),
    "radix": (2, {}),
    "ploc_root_r1": (1, {"FJGPU_PLOC_TOP": "1", "FJGPU_PLOC_RADIUS": "1"}),
    "ploc_root_r16": (1, {"FJGPU_PLOC_TOP": "1", "FJGPU_PLOC_RADIUS": "16"}),
    "ploc_root_r128": (1, {"FJGPU_PLOC_TOP": "1", "FJGPU_PLOC_RADIUS": "128"}),
    "ploc_hybrid64": (1, {"FJGPU_PLOC_TOP": "64"}),
    "ploc_default": (1, {}),
}
THREE_BUILDERS = ("host_sah", "radix", "ploc_root_r16")


class builder(object):
    """global option device_build + the clustering's environment for the scenes created inside; restored on exit"""
    def __init__(self, name, monkeypatch):
        self.mode, self.env, self.mp = BUILDERS[name][0], BUILDERS[name][1], monkeypatch

    def __enter__(self):
        for k in PLOC_ENV:
            self.mp.delenv(k, raising=False)
        for k, v in self.env.items():
            self.mp.setenv(k, v)
        gpu.global_option("device_build", self.mode)

    def __exit__(self, *exc):
        gpu.global_option("device_build", -1)
        for k in PLOC_ENV:
            self.mp.delenv(k, raising=False)


_cache = {}


def family_case(name, directory):
    """(mesh path written into `directory`, rays, oracle t, oracle ids) of a family: per-triangle rays + the soup (+ the axis rays of
    the telescope); the oracle's answer is computed once per session and shared"""
    v, t = pm.FAMILIES[name]()
    path = pm.write_mesh(directory, name, v, t)
    if name not in _cache:
        rays = [pm.per_triangle_rays(v, t), pm.soup_rays(v)]
        if name == "telescope":
            rays.append(pm.axis_rays())
        rays = np.concatenate(rays, axis=0)
        to, io = pm.oracle_trace(pm.trace_scene(path), rays)
        to.setflags(write=False); io.setflags(write=False); rays.setflags(write=False)
        _cache[name] = (rays, to, io)
    return (path,) + _cache[name]


def gpu_trace(text, rays, group=0, count=False):
    sp, _ = tg.prepare(text)
    gs = gpu.Scene(sp)                      # (fails on a builder error: "clustering round merged nothing", ...)
    if count:
        gs.set_option("count_nodes", 1)
    t, ids, uv, st = gs.trace(group, rays)
    facts = {k: int(gs.query(k)) for k in ("stack_need", "blas_nodes", "stack_peak", "stack_peak_closest", "closest_kernel")}
    gs.close()
    return t, ids, facts


def test_lds_constants_are_what_this_file_states(asset_dir):
    sp, _ = tg.prepare(tg._custom_scene(asset_dir, lights=1))
    gs = gpu.Scene(sp)
    assert int(gs.query("stack_lds")) == STACK_LDS and int(gs.query("stack_lds_anyhit")) == STACK_LDS_ANYHIT
    assert int(gs.query("stack_lds_curves")) == STACK_LDS_CURVES and int(gs.query("stack_lds_min")) == min(STACK_LDS_ANYHIT, STACK_LDS)
    assert int(gs.query("stack_lds_canyhit")) == STACK_LDS_CANYHIT
    assert int(gs.query("stack_peak")) == 0
    gs.close()


# ------------------------------------------------------------------------------------------------ 1. builders x meshes
@pytest.mark.parametrize("how", sorted(BUILDERS))
@pytest.mark.parametrize("name", sorted(pm.FAMILIES))
def test_every_builder_gives_the_oracles_hits(name, how, tmp_path, monkeypatch):
    """t, instance and primitive ids bit-exact against the oracle on the per-triangle rays and the soup, for every mesh family and
    builder variant; scene creation succeeds (no "merged nothing": flat_sheet has equal merge distances everywhere, same_centroid
    equal Morton keys) and the tree reports itself"""
    path, rays, to, io = family_case(name, tmp_path)
    with builder(how, monkeypatch):
        t, ids, facts = gpu_trace(pm.trace_scene(path), rays)
    assert np.array_equal(t, to)
    assert np.array_equal(ids, io)
    assert facts["stack_need"] >= 0 and facts["blas_nodes"] >= 1
    assert (io[:, 0] >= 0).sum() >= len(pm.FAMILIES[name]()[1]) * 3 // 4


# ------------------------------------------------------------------------------------------------- 2. ties in one mesh
@pytest.fixture(scope="module")
def dup_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("dup")
    path, rays, tied, winner = pm.duplicate_ties(d)
    to, io = pm.oracle_trace(pm.trace_scene(path), rays)
    assert tied.sum() >= 200
    return path, rays, tied, winner, to, io


@pytest.mark.parametrize("how", sorted(BUILDERS))
def test_ties_inside_one_mesh_go_to_the_largest_id(how, dup_case, monkeypatch):
    path, rays, tied, winner, to, io = dup_case
    with builder(how, monkeypatch):
        t, ids, _ = gpu_trace(pm.trace_scene(path), rays)
    assert np.array_equal(ids[tied], io[tied])
    assert np.array_equal(ids[tied, 1], winner[tied])
    assert np.array_equal(t, to) and np.array_equal(ids, io)


@pytest.mark.parametrize("flat,lds", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_duplicates_frame(flat, lds, dup_case, asset_dir):
    """the same mesh as one plastic object in a 48 x 32 frame: coincident faces shade like the oracle's winner whichever closest-hit
    walk runs (flat_groups, inst_lds on and off)"""
    text = pm.frame_scene(asset_dir, dup_case[0], lights=((2, 6, 4), (-3, 5, 2)), instances=(((-1.2, .3, 0), (0, 0, 0)),), scale=1.0)
    gpu.global_option("flat_groups", flat)
    gpu.global_option("inst_lds", lds)
    try:
        fb, st, ref, rc = tg.render_both(text)
    finally:
        gpu.global_option("flat_groups", 1)
        gpu.global_option("inst_lds", 1)
    assert st.rays.as_dict() == rc.as_dict()
    assert float(tg.rel_err(fb, ref).max()) <= REL_TOL
    assert rc.shadow > 0 and rc.reflect > 0


# ------------------------------------------------------------------------------------------------ 3. tiny primitive sets
@pytest.mark.parametrize("how", THREE_BUILDERS)
@pytest.mark.parametrize("k", [1, 2, 4, 5, 8])
def test_tiny_primitive_sets(k, how, tmp_path, asset_dir, monkeypatch):
    """1 .. 8 triangles (FJ_TINY_PRIMS = FJ_MAX_LEAF_PRIMS = 4: up to 4 the set is a leaf root, tested in the instance loop of the
    phased walk; 5 is the first real tree): alone and as 3 instances beside a normal object, through trace and through a frame"""
    name = "tiny%d" % k
    path, rays, to, io = family_case(name, tmp_path)
    normal = synth.ensure_assets(asset_dir, ("tiny",))["tiny"]
    three = ((0, 0, 0), (.5, 1.5, -.5), (-.5, -1.0, .25))
    crowd = pm.trace_scene(path, instances=three, normal_mesh=normal)
    soup = np.concatenate([rays, pm.soup_rays(np.array([[-3, -4, -3], [3, 3, 3]], dtype=np.float32), n=4000)], axis=0)
    key = ("crowd", k)
    if key not in _cache:
        _cache[key] = pm.oracle_trace(crowd, soup)
    with builder(how, monkeypatch):
        t, ids, facts = gpu_trace(pm.trace_scene(path), rays)
        t3, ids3, _ = gpu_trace(crowd, soup)
        fb, st, ref, rc = tg.render_both(pm.frame_scene(asset_dir, path, lights=((2, 6, 4), (-3, 5, 2)), normal_mesh=normal,
                                                        instances=(((0, .6, 0), (0, 0, 0)), ((1.2, 1.0, -.8), (0, 40, 0)), ((-.9, 1.4, .5), (20, 0, 10)))))
    assert np.array_equal(t, to) and np.array_equal(ids, io)
    assert np.array_equal(t3, _cache[key][0]) and np.array_equal(ids3, _cache[key][1])
    assert len(np.unique(_cache[key][1][:, 0])) >= 4                  # the normal object and the instances are all hit
    assert st.rays.as_dict() == rc.as_dict()
    assert float(tg.rel_err(fb, ref).max()) <= REL_TOL
    _cache[("facts", k, how)] = facts
    print("tiny", k, how, facts)
    # the boundary pair: up to FJ_MAX_LEAF_PRIMS = 4 triangles the device builders make the root a leaf (one dummy node, nothing to push);
    # 5 triangles are the first real tree -- ONE 4-wide node again, so blas_nodes is 1 on both sides and stack_need tells them apart.
    # (The host's SAH builder may split 3 or 4 triangles where that pays, and reports its node storage in chunks of 1024.)
    assert facts["blas_nodes"] >= 1
    if how != "host_sah":
        assert facts["blas_nodes"] == 1 or k > 5
        assert (facts["stack_need"] == 0) == (k <= 4)
    if k <= 2:
        assert facts["stack_need"] == 0
    if k >= 5:
        assert facts["stack_need"] >= 1


# ------------------------------------------------------------------------------------------- 4. the stack overflow area
TEL_SIZE = 64.0                               # the telescope in scenes: 64 units along each axis, so that many octaves lie beyond the
TEL_SCALE = TEL_SIZE / pm.TELESCOPE_SCALE     # camera's near distance
TEL_APEX = np.array([-1.0, 1.5, -1.0])
DIAG = np.ones(3) / np.sqrt(3.0)


def telescope_frame(asset_dir, path, shader, n_inst=1, res=(48, 32)):
    """the camera sits at the telescope's apex and looks out along its axis (yaw 225, pitch 35.26: the direction (1, 1, 1)),
    so camera rays enter the small boxes first and pass all of them.  Two point lights on the axis: one behind the apex -- the shadow
    rays of everything the camera sees run back down the telescope, large boxes first, which is deep for the any-hit walks (no order
    among a node's children) -- and one beyond the large end: shadow rays from the small triangles near the apex leave through every
    larger box, nearest first, which is deep for the walks that sort the children"""
    f3 = lambda p: tuple(float(x) for x in p)
    inst = [(f3(TEL_APEX), (0, 0, 0))] + [(f3(TEL_APEX + np.array(d)), (0, 0, 0)) for d in ((.7, -.2, .1), (.1, .3, .8), (-.4, .5, -.3))][:n_inst - 1]
    lights = (f3(TEL_APEX - 1.0 * DIAG), f3(TEL_APEX + 1.2 * TEL_SIZE * np.ones(3)))
    text = pm.frame_scene(asset_dir, path, lights=lights, res=res, spp=(2, 2), shader=shader, instances=inst, scale=TEL_SCALE)
    cam = TEL_APEX                  # (the apex itself: the cone of camera rays is similar to itself at every octave)
    text = text.replace("SetProperty3 cam1 translate 0.5 2.0 6", "SetProperty3 cam1 translate %.17g %.17g %.17g" % tuple(cam))
    text = text.replace("SetProperty3 cam1 rotate -12 4 0", "SetProperty3 cam1 rotate 35.264389682754654 225 0")
    text = text.replace("SetProperty1 cam1 fov 40", "SetProperty1 cam1 fov 14")
    assert "35.264389682754654 225" in text and "fov 14" in text
    return text


def render_counted(text, batch_tiles=0):
    """counting render (the stack peaks of its launches), production render (same pixels), oracle: ray counts equal, pixels within
    REL_TOL.  Returns the facts of the scene and the peaks."""
    sp, rd = tg.prepare(text)
    gs = gpu.Scene(sp)
    if batch_tiles:
        gs.set_option("batch_tiles", batch_tiles)
    gs.set_option("count_nodes", 1)
    fb, st = gs.render_frame(rd)
    facts = {k: int(gs.query(k)) for k in ("stack_need", "stack_peak", "stack_peak_closest", "stack_peak_shadow", "closest_kernel", "lean_anyhit", "curve_anyhit")}
    facts["batches"] = st.batches
    gs.set_option("count_nodes", 0)
    fb2, st2 = gs.render_frame(rd)
    assert int(gs.query("stack_peak")) == 0                # the production instantiations do not count
    gs.close()
    osc = oracle_ffi.OracleScene(sp)
    ref, rc = osc.render(rd)
    osc.close()
    assert np.array_equal(fb, fb2) or float(tg.rel_err(fb, fb2).max()) <= 1e-6
    assert st.rays.as_dict() == rc.as_dict() == st2.rays.as_dict(), (st.rays.as_dict(), rc.as_dict())
    facts["max_rel_err"] = float(tg.rel_err(fb, ref).max())
    assert facts["max_rel_err"] <= REL_TOL, facts["max_rel_err"]
    facts["rays"] = rc.as_dict()
    return facts


# stack_peak of k_trace_closest on the axis rays, measured on the MI355X with the default build (stack_need in brackets).  Only the radix
# tree is walked past the 32 LDS entries: the other builders put two or three triangles of an octave into one leaf, so a level of
# their trees pushes one sibling where the radix tree pushes three.
PEAKS_TRACE = {"host_sah": 20, "ploc_default": 20, "ploc_hybrid64": 18, "ploc_root_r1": 20, "ploc_root_r16": 20, "ploc_root_r128": 20,   # [42 43 46 49 49 49]
               "radix": 54}                                                                                                              # [76]


@pytest.mark.parametrize("how", sorted(BUILDERS))
def test_telescope_trace_overflows_the_lds_stack(how, tmp_path, monkeypatch):
    """k_trace_closest on the axis rays: the tree needs more than the 32 LDS entries on every builder, on the radix tree the walk
    really holds more than 32 (54: 22 rows of the overflow area written and read back), and the hits are the oracle's bit for bit.
    On the other builders the walk stays in LDS (PEAKS_TRACE: measured 18 .. 20 of a need of 42 .. 49) -- asserted as measured."""
    path, rays, to, io = family_case("telescope", tmp_path)
    with builder(how, monkeypatch):
        t, ids, facts = gpu_trace(pm.trace_scene(path), rays, count=True)
    print("telescope trace", how, facts)
    assert np.array_equal(t, to) and np.array_equal(ids, io)
    assert facts["stack_need"] > STACK_LDS
    if how == "radix":
        assert facts["stack_peak_closest"] > STACK_LDS
    assert facts["stack_peak_closest"] >= PEAKS_TRACE[how]
    assert facts["stack_peak"] <= facts["stack_need"]


FRAME_WALKS = {
    # name: (shader, instances, global options, closest_kernel expected, lean_anyhit expected)
    "closest_general_and_lean_anyhit": ("plastic", 1, {}, 0, 1),
    "closest_phased": ("glass", 1, {"flat_groups": 0}, 1, 1),
    "closest_flat": ("glass", 1, {}, 4, 1),
    "shadow_general_translucent": ("translucent", 1, {}, 0, 0),
    "shadow_split_per_instance": ("plastic", 4, {}, 0, 1),
}
OPTION_DEFAULTS = {"flat_groups": 1}
# (stack_peak_closest, stack_peak_shadow) measured on the MI355X with the default build, whole frame and tile by tile alike;
# stack_need is 42 with the host's tree and 76 with the radix tree.  (The glass scenes have no shadow rays.)
PEAKS_FRAMES = {
    ("host_sah", "closest_general_and_lean_anyhit"): (13, 21), ("radix", "closest_general_and_lean_anyhit"): (41, 26),
    ("host_sah", "closest_phased"): (13, 0), ("radix", "closest_phased"): (41, 0),
    ("host_sah", "closest_flat"): (15, 0),                       # (flat groups are built from host trees only)
    ("host_sah", "shadow_general_translucent"): (13, 3), ("radix", "shadow_general_translucent"): (41, 6),
    ("host_sah", "shadow_split_per_instance"): (13, 25), ("radix", "shadow_split_per_instance"): (41, 40),
}


@pytest.mark.parametrize("batch_tiles", [0, 1], ids=["whole_frame", "tile_by_tile"])
@pytest.mark.parametrize("how,walk", sorted(PEAKS_FRAMES))
def test_telescope_frames_overflow_the_lds_stack(how, walk, batch_tiles, tmp_path, asset_dir, monkeypatch):
    """48 x 32 frames, 2 x 2 samples, camera at the telescope's apex, as a whole frame and tile by tile (the overflow rows are per
    persistent thread and serve many small launches); every frame is the oracle's (ray counts equal, pixels within REL_TOL, counting
    and production renders alike).  What goes through the overflow area in the DEFAULT build (PEAKS_FRAMES):
      k_trace_closest (32 in LDS)         41 on the radix tree
      k_trace_closest_phased (32)         41 on the radix tree
      k_shadow_anyhit (12), one instance  21 on the host's tree, 26 on the radix tree
      k_shadow_anyhit (12), rays split per candidate instance (4 telescopes)   25 / 40
    and what does not:
      k_trace_closest_flat (32)           15: flat groups take host trees only, whose leaves hold an octave's triangles together
      k_shadow_trace (32)                 3 / 6: it visits the nearest child first and a translucent hit shortens the ray
    Those two are asserted at the measured depth here; their overflow rows are written and read back by the same frames in the stack4
    variant build (4 entries in LDS in every walk), which tests/test_gpu_variant_builds.py runs."""
    shader, n_inst, opts, kernel, lean = FRAME_WALKS[walk]
    v, t = pm.telescope()
    path = pm.write_mesh(tmp_path, "telescope", v, t)
    for k, val in opts.items():
        gpu.global_option(k, val)
    try:
        with builder(how, monkeypatch):
            facts = render_counted(telescope_frame(asset_dir, path, shader, n_inst), batch_tiles)
    finally:
        for k in opts:
            gpu.global_option(k, OPTION_DEFAULTS[k])
    print("telescope frame", how, walk, batch_tiles, facts)
    want_closest, want_shadow = PEAKS_FRAMES[(how, walk)]
    assert facts["closest_kernel"] == kernel and facts["lean_anyhit"] == lean
    assert facts["stack_need"] > STACK_LDS
    assert (facts["batches"] > 1) == (batch_tiles == 1)
    assert (facts["rays"]["shadow"] > 0) == (shader != "glass")
    assert facts["stack_peak_closest"] >= want_closest              # (closest-hit walks: a function of the ray and the tree alone)
    if how == "radix" and walk in ("closest_general_and_lean_anyhit", "closest_phased"):
        assert facts["stack_peak_closest"] > STACK_LDS
    if lean and shader != "glass":
        # (the any-hit walk postpones leaves depending on what its wave does: the measured 21 .. 40 may move by an entry or two)
        assert facts["stack_peak_shadow"] > STACK_LDS_ANYHIT
    else:
        assert facts["stack_peak_shadow"] >= want_shadow
    assert facts["stack_peak"] <= facts["stack_need"]


def fur_telescope_text(directory, asset_dir):
    """the fur scene of the workloads (48 x 32, 2 x 2 samples, two lights) with the ten largest octaves of the telescope, at a size of
    0.5, in place of its mesh"""
    from fujiyama_renderer_amd import workloads
    v, t = pm.telescope(n=30)
    v = (v.astype(np.float64) * (0.5 / pm.TELESCOPE_SCALE)).astype(np.float32)
    path = pm.write_mesh(directory, "telescope_fur", v, t)
    text = workloads.furry(asset_dir, res=(48, 32), spp=(2, 2), mesh="furball", nlights=2)
    old = synth.ensure_assets(asset_dir, ("furball",))["furball"]
    assert old in text
    return text.replace(old, path)


def test_fur_on_the_telescope(tmp_path, asset_dir):
    """the curve walks (k_shadow_anyhit_curves: 16 entries in LDS, the curve instantiation of k_trace_closest: 20): fur can only be
    grown on a mesh by CurveGeneratorProcedure, here on the ten largest octaves of the telescope at a size of 0.5 (the oracle's grid
    over the curves takes 2 s to build at this size and 14 s at 2.0).  Parity with the oracle, and the depth the walks reach:
    measured stack_need 38, closest-hit walk 16, any-hit walk 16 -- the last LDS entry, not beyond (at size 2.0: need 49, 15 and 19,
    three rows of the overflow area).  So the DEFAULT build's curve walks stay inside LDS here; their overflow rows are covered by this
    scene in the stack4 variant build (4 entries in LDS), run by tests/test_gpu_variant_builds.py."""
    facts = render_counted(fur_telescope_text(tmp_path, asset_dir))
    print("telescope fur", facts)
    assert facts["closest_kernel"] == 2 and facts["curve_anyhit"] == 1 and facts["rays"]["shadow"] > 0
    assert facts["stack_need"] > STACK_LDS_CURVES
    assert facts["stack_peak_closest"] >= 16 and facts["stack_peak_shadow"] >= STACK_LDS_CANYHIT
    assert facts["stack_peak"] <= facts["stack_need"]
