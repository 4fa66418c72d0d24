"""GPU suite, the two variant builds of the product libraries (-m gpu): what the default build cannot reach.

stack4    -DFJ_STACK_LDS*=4: the production code with four traversal-stack entries per lane in LDS in EVERY walk, so that the rows of the
          global overflow area (TravStack, AH_OVF, CA_OVF; sized (stack_need - FJ_STACK_LDS_MIN) x persistent threads at scene creation) are
          written and read back by every kernel family -- also by the four that stay inside LDS in the default build (k_trace_closest_flat,
          k_shadow_trace, k_shadow_anyhit_curves, the curve and motion instantiations; tests/test_gpu_pathological.py).
validate  -DFJ_TRI_FILTER_VALIDATE -DFJ_LIGHT_CONE_VALIDATE -DFJ_LIGHT_HULL_VALIDATE: the exact test behind every verdict of the f32 triangle
          filter, the per-light box cones and the per-light hull cones, counted on the device.  The one-sided contracts are pinned on the CPU
          through host twins; here they are held on the device's own records, uploads and wave-level logic: 0 contradictions.

ffi.LIB_DIR is read at import, so each variant runs in ONE child process (tests/variant_child.py) per session, started by a session fixture;
the child measures and writes one record per case, the tests below read their record and assert.  A child that dies -- return code, time limit
or a HIP error in its output -- fails every test of its variant with the tail of its output; nothing is retried.

Time limits: three times the wall time of the same case list in a child that uses the DEFAULT library (whole process, asset directory empty
at the start), measured on the MI355X: profiles/variant_builds.txt.
"""
import json
import os
import re
import subprocess
import sys

import pytest

import test_gpu_parity as tg
import test_gpu_pathological as tp
import variant_child as vc
from test_variant_builds_cpu import EXPECTED, ensure_variant

pytestmark = pytest.mark.gpu

# seconds: 3 x the default library's wall time for the list, the largest of the runs on two boxes (stack4 7.95, 7.44, 7.61 s; validate 1.19, 1.21,
# 1.36, 1.35, 1.38 s: profiles/variant_builds.txt)
CHILD_TIMEOUT = {"stack4": 3 * 7.95, "validate": 3 * 1.38}
HIP_ERROR = re.compile(r"hipError|HIP error|illegal memory access|Memory access fault|fjgpu error -1\b|Aborted|Segmentation fault")

STACK4_ROWS = 4          # LDS entries of every walk in the stack4 build


class Dead(object):
    def __init__(self, why):
        self.why = why


def run_child(variant, directory):
    """-> the child's result (dict), or Dead.  The variant is built first if its directory is missing."""
    lib_dir = ensure_variant(variant)
    out = os.path.join(str(directory), variant + ".json")
    env = dict(os.environ, FJGPU_LIBDIR=lib_dir)
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "variant_child.py"), variant, out]
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT[variant])
    except subprocess.TimeoutExpired as e:
        tail = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode("utf-8", "replace")
        return Dead("the %s child ran into its time limit of %.0f s\n%s" % (variant, CHILD_TIMEOUT[variant], tail[-3000:]))
    print(r.stdout[-6000:])
    if r.returncode != 0:
        return Dead("the %s child ended with status %d\n%s" % (variant, r.returncode, r.stdout[-3000:]))
    if HIP_ERROR.search(r.stdout):
        return Dead("the %s child's output names a HIP error\n%s" % (variant, r.stdout[-3000:]))
    with open(out) as f:
        result = json.load(f)
    if not result.get("complete"):
        return Dead("the %s child left an incomplete result\n%s" % (variant, r.stdout[-3000:]))
    return result


@pytest.fixture(scope="session")
def stack4_run(tmp_path_factory):
    return run_child("stack4", tmp_path_factory.mktemp("variant_stack4"))


@pytest.fixture(scope="session")
def validate_run(tmp_path_factory):
    return run_child("validate", tmp_path_factory.mktemp("variant_validate"))


def record(run, name):
    if isinstance(run, Dead):
        pytest.fail(run.why)
    rec = run["records"][name]
    assert rec["error"] is None, rec["error"]
    return rec


def delta(rec, counter):
    return rec["counters_after"][counter] - rec["counters_before"][counter]


@pytest.mark.parametrize("variant", ["stack4", "validate"])
def test_the_child_ran_the_variant_it_was_asked_for(variant, stack4_run, validate_run):
    run = {"stack4": stack4_run, "validate": validate_run}[variant]
    if isinstance(run, Dead):
        pytest.fail(run.why)
    assert run["build_config"] == EXPECTED[variant]
    assert sorted(run["records"]) == sorted(n for n, _, _ in vc.CASE_LISTS[variant]())


# ------------------------------------------------------------------------------------------------------------ stack4
# kernel families of the coverage condition: each needs a passing case whose peak is strictly above the family's LDS rows (4)
CLOSEST, PHASED, FLAT, C_CURVES, C_MOTION = ("k_trace_closest", "k_trace_closest_phased", "k_trace_closest_flat", "k_trace_closest<curves>",
                                              "k_trace_closest<motion>")
AH_SINGLE, AH_SPLIT, AH_CURVES, SH_TRANSLUCENT, SH_MOTION_CURVES = ("k_shadow_anyhit, single instance", "k_shadow_anyhit, split", "k_shadow_anyhit_curves",
                                                                    "k_shadow_trace, translucent", "k_shadow_trace, motion or curves")
AH_OTHER = "k_shadow_anyhit"      # (recorded; not a family of the condition)
FAMILIES = (CLOSEST, PHASED, FLAT, C_CURVES, C_MOTION, AH_SINGLE, AH_SPLIT, AH_CURVES, SH_TRANSLUCENT, SH_MOTION_CURVES)
SHADOW_FAMILIES = (AH_SINGLE, AH_SPLIT, AH_CURVES, SH_TRANSLUCENT, SH_MOTION_CURVES, AH_OTHER)
# the any-hit walks postpone leaves depending on what their wave does, so their peaks may move by an entry or two from run to run (as in
# test_telescope_frames_overflow_the_lds_stack); the other walks' peaks are a function of the ray and the tree alone
MOVING = (AH_SINGLE, AH_SPLIT, AH_CURVES, AH_OTHER)
WALK_FAMILIES = {"closest_general_and_lean_anyhit": (CLOSEST, AH_SINGLE), "closest_phased": (PHASED, None), "closest_flat": (FLAT, None),
                 "shadow_general_translucent": (CLOSEST, SH_TRANSLUCENT), "shadow_split_per_instance": (CLOSEST, AH_SPLIT)}


def _stack4_expect():
    """case -> (closest_kernel, lean_anyhit, curve_anyhit, {family: peak measured on the MI355X in the stack4 build}); the peaks equal the
    default build's (PEAKS_TRACE, PEAKS_FRAMES of test_gpu_pathological): a peak is a property of the walk, not of where its rows live"""
    out = {}
    for how in vc.TRACE_BUILDERS:
        out["trace_%s" % how] = (0, None, None, {CLOSEST: tp.PEAKS_TRACE[how]})
    for how, walk in vc.TELESCOPE_FRAMES:
        _, _, _, kernel, lean = tp.FRAME_WALKS[walk]
        pc, ps = tp.PEAKS_FRAMES[(how, walk)]
        fc, fs = WALK_FAMILIES[walk]
        for bt in (0, 1):
            out["telescope_%s_%s_%s" % (walk, how, vc.BATCH_IDS[bt])] = (kernel, lean, 0, dict({fc: pc}, **({fs: ps} if fs else {})))
    out["fur_telescope"] = (2, 0, 1, {C_CURVES: 16, AH_CURVES: 16})
    out["c5_hair_vertex_velocity_64x48_2spp"] = (3, 0, 0, {C_MOTION: 18, SH_MOTION_CURVES: 16})
    out["motion_velocity_and_object_64x48_2spp"] = (3, 0, 0, {C_MOTION: 5, SH_MOTION_CURVES: 7})
    out["motion_camera_64x48_3spp"] = (0, 1, 0, {CLOSEST: 7, AH_SINGLE: 5})          # (a moving camera alone takes the static kernels)
    out["c2_buddhas_96x54_2spp_bunny"] = (0, 1, 0, {CLOSEST: 12, AH_SPLIT: 14})
    out["crowd_150_instances_64x48_2spp"] = (0, 1, 0, {CLOSEST: 7, AH_SPLIT: 6})
    out["c6_ibl_dome_light_64x48_2spp"] = (0, 1, 0, {CLOSEST: 7, AH_OTHER: 11})
    out["teapot_64_2spp"] = (4, 1, 0, {FLAT: 13, AH_OTHER: 10})
    return out


STACK4_EXPECT = _stack4_expect()
# a (case, family) pair COVERS the family where its measured peak clears the four LDS rows -- by at least two rows for the walks whose peak moves
COVERING = {(case, fam) for case, e in STACK4_EXPECT.items() for fam, peak in e[3].items()
            if fam in FAMILIES and peak > STACK4_ROWS + (2 if fam in MOVING else 0)}


def test_every_kernel_family_has_a_covering_case():
    """the condition itself, on the table: every family is covered, the translucent k_shadow_trace by the radix tree only (6; the host's
    tree stays at 3 and covers nothing)"""
    assert sorted(STACK4_EXPECT) == sorted(n for n, _, _ in vc.stack4_cases())
    for fam in FAMILIES:
        assert any(f == fam for _, f in COVERING), fam
    assert {c for c, f in COVERING if f == SH_TRANSLUCENT} == {"telescope_shadow_general_translucent_radix_whole_frame", "telescope_shadow_general_translucent_radix_tile_by_tile"}


@pytest.mark.parametrize("case", sorted(STACK4_EXPECT))
def test_stack4_walks_through_the_overflow_rows(case, stack4_run):
    """every case in the build with four LDS rows: ray counts equal to the oracle's, pixels within REL_TOL, counting and production renders
    alike (render_counted's assertions, which ran in the child: an error is in the record), fjgpu_trace hits bit for bit; the kernel that ran
    is the one named; stack_peak <= stack_need (a walk that held more would have written past its rows); and the peaks: strictly above the
    four rows where the case covers a family -- the overflow rows were written and read back --, at the measured value elsewhere"""
    rec = record(stack4_run, case)
    kernel, lean, curve, peaks = STACK4_EXPECT[case]
    facts = rec["facts"]
    print(case, facts)
    assert facts["closest_kernel"] == kernel
    if rec["kind"] == "trace":
        assert rec["bit_exact"] is True and rec["hits"] > 0
    else:
        assert (facts["lean_anyhit"], facts["curve_anyhit"]) == (lean, curve)
        assert rec["rays"] == rec["rays_oracle"] == facts["rays"]
        assert rec["max_rel_err"] <= tg.REL_TOL
    assert facts["stack_need"] > STACK4_ROWS
    assert facts["stack_peak"] <= facts["stack_need"]
    for fam, want in peaks.items():
        got = facts["stack_peak_shadow" if fam in SHADOW_FAMILIES else "stack_peak_closest"]
        if (case, fam) in COVERING:
            assert got > STACK4_ROWS, (fam, got)
        if fam not in MOVING:
            assert got >= want, (fam, got, want)
        else:
            assert got > 0, (fam, got)
    # (the validation counters do not exist in this build)
    assert rec["counters_after"]["tri_filter_contradictions"] == -1 and rec["counters_after"]["light_cone_contradictions"] == -1


# ---------------------------------------------------------------------------------------------------------- validate
VALIDATE_CASES = sorted(n for n, _, _ in vc.validate_cases())
CONE_CASES = {"headline": True, "light_inside": False, "light_level_with_a_box_face": False, "light_far_away": False, "two_groups": True,
              "dome_ibl": False}                        # True: the cones must have given verdicts
HULL_CASES = {"headline": True, "mirrored_instance": True, "light_level_with_the_mesh": False, "light_inside": False, "two_groups": True}
FILTER_CASES = ("dome_ibl", "dragon_small_96x54", "buddhas_bunny_96x54", "telescope_host_sah", "telescope_radix")


@pytest.mark.parametrize("case", VALIDATE_CASES)
def test_validate_frames_are_the_oracles(case, validate_run):
    """the validate build queues the hull-settled pairs all the same and adds their colour whatever the walk finds, so its frames are the
    oracle's too -- with the hulls on and off: ray counts equal, pixels within REL_TOL; and no counter of any of the three contracts moved
    the wrong way on any scene"""
    rec = record(validate_run, case)
    print(case, rec["facts"], rec["counters_by_hulls"])
    assert rec["rays"] == rec["rays_oracle"] == rec["rays_hulls_off"]
    assert rec["max_rel_err"] <= tg.REL_TOL
    assert rec["counting_equals_production"] is True
    for c in ("light_cone_contradictions", "light_hull_contradictions", "tri_filter_contradictions"):
        assert delta(rec, c) == 0, c
    for c in vc.COUNTERS:
        assert rec["counters_before"][c] >= 0 and delta(rec, c) >= 0, c           # (-1: a build without the switch)


@pytest.mark.parametrize("case", sorted(CONE_CASES))
def test_no_box_cone_verdict_is_contradicted_on_the_device(case, validate_run):
    """a cone verdict implies that the reference's BoxRayIntersect returns false: the exact box test behind every verdict of the light loop.
    The loop puts a pair to the hull cone first, and a hull lies inside its box cone: the verdicts come from the frames with light_hulls 0."""
    rec = record(validate_run, case)
    assert delta(rec, "light_cone_contradictions") == 0
    print(case, "light_cone_verdicts", delta(rec, "light_cone_verdicts"), rec["counters_by_hulls"])
    if CONE_CASES[case]:
        assert delta(rec, "light_cone_verdicts") > 0
        assert rec["counters_by_hulls"]["0"]["light_cone_verdicts"] > 0
    if rec["facts"]["light_cone_records"] == 0:
        assert delta(rec, "light_cone_verdicts") == 0


@pytest.mark.parametrize("case", sorted(HULL_CASES))
def test_no_hull_verdict_is_contradicted_on_the_device(case, validate_run):
    """a hull verdict implies no hit: every settled pair (queued compact for the lean any-hit walk) is walked, none finds a triangle"""
    rec = record(validate_run, case)
    assert rec["facts"]["lean_anyhit"] == 1
    assert delta(rec, "light_hull_contradictions") == 0
    print(case, "light_hull_verdicts", delta(rec, "light_hull_verdicts"), rec["counters_by_hulls"])
    if HULL_CASES[case]:
        assert delta(rec, "light_hull_verdicts") > 0
    assert rec["counters_by_hulls"]["0"]["light_hull_verdicts"] == 0            # (option light_hulls 0: nothing settled, nothing flagged)


@pytest.mark.parametrize("case", FILTER_CASES)
def test_the_triangle_filter_never_contradicts_the_exact_test_on_the_device(case, validate_run):
    """the f32 filter of the lean any-hit walk with the exact test behind every verdict: MISS and HIT are never contradicted, and both are
    given (`maybe` and `exact_hits` are printed: undecided tests are about 0.1 % on big frames and may be none on a small one)"""
    rec = record(validate_run, case)
    assert rec["facts"]["lean_anyhit"] == 1
    d = {c: delta(rec, c) for c in vc.COUNTERS if c.startswith("tri_filter")}
    print(case, d)
    assert d["tri_filter_contradictions"] == 0
    assert d["tri_filter_miss"] > 0 and d["tri_filter_hit"] > 0
    assert d["tri_filter_hit"] <= d["tri_filter_exact_hits"] <= d["tri_filter_hit"] + d["tri_filter_maybe"]
