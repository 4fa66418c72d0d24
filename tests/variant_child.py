"""Child process of tests/test_gpu_variant_builds.py: `python variant_child.py CASE_LIST OUT.json` runs one case list -- "stack4" or
"validate" -- with whatever build of the product libraries FJGPU_LIBDIR names (ffi.LIB_DIR is read at import, so a build is a process) and
writes one JSON record per case: facts of the scene, ray counts, the largest relative error against the oracle, whether the hits were bit-exact,
the process-wide validation counters before and after the case, the seconds it took.  The file is rewritten after every case.

A failed comparison (AssertionError) is written into the case's record and the list goes on; anything else -- a HIP error first of all --
ends the process at once with status 1: nothing more is started on a device after a fault.  The parent asserts; this file only measures.

The cases are the suite's own small shapes, built by the helpers of test_gpu_pathological, test_gpu_light_cone, frame_cases and workloads.
"""
import json
import os
import sys
import tempfile
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CONFIG_NAMES = ("stack_lds", "stack_lds_curves", "stack_lds_anyhit", "stack_lds_canyhit", "stack_lds_min",
                "tri_filter_validate", "light_cone_validate", "light_hull_validate")
COUNTERS = ("light_cone_verdicts", "light_cone_contradictions", "light_hull_verdicts", "light_hull_contradictions",
            "tri_filter_miss", "tri_filter_hit", "tri_filter_maybe", "tri_filter_exact_hits", "tri_filter_contradictions")

TRACE_BUILDERS = ("host_sah", "radix", "ploc_root_r16")
MOTION_FRAMES = ("c5_hair_vertex_velocity_64x48_2spp", "motion_velocity_and_object_64x48_2spp", "motion_camera_64x48_3spp")
OTHER_FRAMES = ("c2_buddhas_96x54_2spp_bunny", "crowd_150_instances_64x48_2spp", "c6_ibl_dome_light_64x48_2spp", "teapot_64_2spp")
TELESCOPE_FRAMES = (       # (builder, walk) as in test_gpu_pathological.PEAKS_FRAMES: flat groups are built from host trees only
    ("host_sah", "closest_general_and_lean_anyhit"), ("radix", "closest_general_and_lean_anyhit"),
    ("host_sah", "closest_phased"), ("radix", "closest_phased"),
    ("host_sah", "closest_flat"),
    ("host_sah", "shadow_general_translucent"), ("radix", "shadow_general_translucent"),
    ("host_sah", "shadow_split_per_instance"), ("radix", "shadow_split_per_instance"),
)
BATCH_IDS = {0: "whole_frame", 1: "tile_by_tile"}


def stack4_cases():
    """[(name, kind, arguments)]: the walks of DESIGN 5 with 4 stack entries in LDS"""
    out = [("trace_%s" % how, "trace", dict(how=how)) for how in TRACE_BUILDERS]
    for how, walk in TELESCOPE_FRAMES:
        for bt in (0, 1):
            out.append(("telescope_%s_%s_%s" % (walk, how, BATCH_IDS[bt]), "telescope", dict(how=how, walk=walk, batch_tiles=bt)))
    out.append(("fur_telescope", "fur", {}))
    out += [(name, "frame", dict(name=name)) for name in MOTION_FRAMES + OTHER_FRAMES]
    return out


def validate_cases():
    """[(name, kind, arguments)]: the scenes whose light loop and any-hit walk the validate build checks verdict by verdict"""
    return [(name, "scene", dict(scene=name)) for name in (
        "headline", "light_inside", "light_level_with_a_box_face", "light_far_away", "two_groups", "dome_ibl",      # box cones (and hulls)
        "mirrored_instance", "light_level_with_the_mesh",                                                          # hull cones
        "dragon_small_96x54", "buddhas_bunny_96x54")] + [                                                          # triangle filter (with dome_ibl)
        ("telescope_%s" % how, "telescope_parity", dict(how=how)) for how in ("host_sah", "radix")]


CASE_LISTS = {"stack4": stack4_cases, "validate": validate_cases}


class Env(object):
    """what test_gpu_pathological.builder needs of a monkeypatch"""
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=True):
        os.environ.pop(k, None)


def read_counters(asset_dir):
    """the validation counters of the process (a query needs a scene handle: a small one, which renders nothing); -1 in builds without the switch"""
    import test_gpu_parity as tg
    from fujiyama_renderer_amd import gpu
    sp, _ = tg.prepare(tg._custom_scene(asset_dir, lights=1))
    gs = gpu.Scene(sp)
    out = {k: int(gs.query(k)) for k in COUNTERS}
    gs.close()
    return out


def validate_scene_text(name, asset_dir):
    import test_gpu_light_cone as lc
    import test_gpu_parity as tg
    from fujiyama_renderer_amd import gpu, workloads
    if name == "headline":
        return lc.headline(asset_dir)
    if name == "light_inside":                    # the centre of the dragon's box: inside the box and inside the hull
        b = lc.group_box(lc.headline(asset_dir))
        c = .5 * (b[:3] + b[3:])
        return lc.headline(asset_dir, "SetProperty3 light1 translate %r %r %r" % (float(c[0]), float(c[1]), float(c[2])))
    if name == "light_level_with_a_box_face":
        b = lc.group_box(lc.headline(asset_dir))
        return lc.headline(asset_dir, "SetProperty3 light2 translate %r %r %r" % (float(b[3] + 2.5), float(b[4]), float(b[5] + 1.5)))
    if name == "light_far_away":
        return lc.headline(asset_dir, "SetProperty3 light3 translate 10000 12 3000")
    if name == "two_groups":
        return lc.headline(asset_dir, *lc.TWO_GROUPS)
    if name == "dome_ibl":
        return workloads.ibl(asset_dir, mesh="small", sample_count=48, **lc.SHAPE)
    if name == "mirrored_instance":
        return lc.headline(asset_dir, "SetProperty3 dragon_shader0 diffuse 0.6 0.3 0.2", "SetProperty3 dragon1 scale -0.5 0.7 0.4")
    if name == "light_level_with_the_mesh":
        b = lc.group_box(lc.headline(asset_dir))
        text = lc.headline(asset_dir, "SetProperty3 light2 translate %r %r %r" % (float(.5 * (b[0] + b[3])), float(b[4]), float(.5 * (b[2] + b[5]))))
        sp, _ = tg.prepare(text)
        rec, _, _ = gpu.host_light_hulls(sp, 0)
        assert list(rec["count"]) == [6, 6, 0, 6]
        return text
    if name == "dragon_small_96x54":
        return workloads.dragon(asset_dir, res=(96, 54), spp=(2, 2), mesh="small")
    if name == "buddhas_bunny_96x54":
        return workloads.buddhas(asset_dir, res=(96, 54), spp=(2, 2), mesh="bunny")
    raise KeyError(name)


def render_parity(text, rec):
    """counting and production frame with the scene option light_hulls 1 and 0 on one resident scene, against the oracle (rendered once);
    the figures first, then the comparison.  The light loop puts a pair to the hull cone first and a hull lies inside its box cone, so with
    the hulls on no pair of a group that has both reaches the box cone: the frames with light_hulls 0 are the ones that count cone verdicts.
    rec["counters_by_hulls"]: the counters' deltas of each setting's two frames."""
    import numpy as np
    import oracle_ffi
    import test_gpu_parity as tg
    from fujiyama_renderer_amd import gpu
    sp, rd = tg.prepare(text)
    gs = gpu.Scene(sp)
    rec["facts"] = {k: int(gs.query(k)) for k in ("lean_anyhit", "closest_kernel", "light_cone_rows", "light_cone_records", "light_hull_rows", "light_hull_records")}
    got, rec["counters_by_hulls"] = {}, {}
    for hulls in (1, 0):
        before = {k: int(gs.query(k)) for k in COUNTERS}
        gs.set_option("light_hulls", hulls)
        gs.set_option("count_nodes", 1)
        fb, st = gs.render_frame(rd)
        gs.set_option("count_nodes", 0)
        fb2, _ = gs.render_frame(rd)
        after = {k: int(gs.query(k)) for k in COUNTERS}
        rec["counters_by_hulls"][str(hulls)] = {k: after[k] - before[k] for k in COUNTERS}
        got[hulls] = (fb, fb2, st.rays.as_dict())
    gs.close()
    osc = oracle_ffi.OracleScene(sp)
    ref, rc = osc.render(rd)
    osc.close()
    rec["rays_oracle"] = rc.as_dict()
    rec["rays"] = got[1][2]
    rec["rays_hulls_off"] = got[0][2]
    rec["max_rel_err"] = max(float(tg.rel_err(fb, ref).max()) for hulls in got for fb in got[hulls][:2])
    rec["counting_equals_production"] = all(bool(np.array_equal(a, b)) or float(tg.rel_err(a, b).max()) <= 1e-6 for a, b, _ in got.values())
    assert rec["rays"] == rec["rays_oracle"] == rec["rays_hulls_off"], (rec["rays"], rec["rays_hulls_off"], rec["rays_oracle"])
    assert rec["max_rel_err"] <= tg.REL_TOL, rec["max_rel_err"]
    assert rec["counting_equals_production"]


def run_case(kind, args, asset_dir, directory, rec):
    import numpy as np
    import pathological_meshes as pm
    import test_gpu_pathological as tp
    from fujiyama_renderer_amd import gpu, workloads
    from frame_cases import FRAMES
    if kind == "trace":
        path, rays, to, io = tp.family_case("telescope", directory)
        with tp.builder(args["how"], Env()):
            t, ids, facts = tp.gpu_trace(pm.trace_scene(path), rays, count=True)
        rec["facts"] = facts
        rec["bit_exact"] = bool(np.array_equal(t, to) and np.array_equal(ids, io))
        rec["hits"] = int((io[:, 0] >= 0).sum())
        assert rec["bit_exact"]
    elif kind in ("telescope", "telescope_parity"):
        walk = args.get("walk", "closest_general_and_lean_anyhit")
        shader, n_inst, opts, _, _ = tp.FRAME_WALKS[walk]
        v, t = pm.telescope()
        path = pm.write_mesh(directory, "telescope", v, t)
        for k, val in opts.items():
            gpu.global_option(k, val)
        try:
            with tp.builder(args["how"], Env()):
                text = tp.telescope_frame(asset_dir, path, shader, n_inst)
                if kind == "telescope":
                    rec["facts"] = tp.render_counted(text, args["batch_tiles"])
                else:
                    render_parity(text, rec)
        finally:
            for k in opts:
                gpu.global_option(k, tp.OPTION_DEFAULTS[k])
    elif kind == "fur":
        rec["facts"] = tp.render_counted(tp.fur_telescope_text(directory, asset_dir))
    elif kind == "frame":
        b, kw = FRAMES[args["name"]]
        rec["facts"] = tp.render_counted(workloads.BUILDERS[b](asset_dir, **kw))
    elif kind == "scene":
        render_parity(validate_scene_text(args["scene"], asset_dir), rec)
    else:
        raise KeyError(kind)
    if "facts" in rec and "rays" in rec["facts"]:          # (render_counted: equal to the oracle's, or it raised)
        rec["rays"] = rec["rays_oracle"] = rec["facts"]["rays"]
        rec["max_rel_err"] = rec["facts"]["max_rel_err"]


def main(argv):
    which, out_path = argv[1], argv[2]
    cases = CASE_LISTS[which]()
    from fujiyama_renderer_amd import ffi, gpu, workloads
    result = {"case_list": which, "lib_dir": ffi.LIB_DIR, "build_config": {k: int(gpu.build_config(k)) for k in CONFIG_NAMES},
              "records": {}, "complete": False}

    def dump():
        with open(out_path + ".tmp", "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
        os.replace(out_path + ".tmp", out_path)

    dump()
    if gpu.device_count() < 1:
        print("variant_child: no device", flush=True)
        return 1
    asset_dir = workloads.default_asset_dir()
    os.makedirs(asset_dir, exist_ok=True)
    directory = tempfile.mkdtemp(prefix="variant_child_")
    t_all = time.time()
    for name, kind, args in cases:
        rec = {"kind": kind, "args": args, "error": None}
        result["records"][name] = rec
        t0 = time.time()
        try:
            rec["counters_before"] = read_counters(asset_dir)
            try:
                run_case(kind, args, asset_dir, directory, rec)
            except AssertionError:
                rec["error"] = traceback.format_exc()[-3000:]
            rec["counters_after"] = read_counters(asset_dir)
        except BaseException:
            rec["error"] = "DIED: " + traceback.format_exc()[-3000:]
            result["total_seconds"] = time.time() - t_all
            dump()
            print("variant_child: %s died\n%s" % (name, rec["error"]), flush=True)
            return 1
        rec["seconds"] = time.time() - t0
        result["total_seconds"] = time.time() - t_all
        dump()
        print("variant_child %s: %-60s %6.2f s  %s" % (which, name, rec["seconds"], "FAILED" if rec["error"] else "ok"), flush=True)
    result["complete"] = True
    dump()
    print("variant_child %s: %d cases in %.1f s" % (which, len(cases), result["total_seconds"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
