"""The wavefront frame loop (csrc/device/fjgpu_frame.hip: fjgpu_render_tiles, fjgpu_render_tiles_variance) pinned to a ledger that was
recorded BEFORE the loop was moved out of fjgpu_api.hip and cut into stages: one small frame per path through the loop, each as one
batch (batch_tiles 0) and as a batch per tile (batch_tiles 1), and per frame

  - the integer fields of fjgpu_stats that do not depend on the order in which blocks run: the ray counts per context, batches,
    closest_launches, light_loop_launches, shadow_walk_launches, trace_launches, rays_sorted;
  - the query accum_memsets;
  - for the frame that is reproducible to the bit (one light, no bounces: tests/test_gpu_shade_stores.py), the SHA-256 of the 32-bit words
    of the framebuffer -- and of the variance buffer, for fjgpu_render_tiles_variance on that frame.

The refusals of the two entry points are pinned as return code plus the whole text of fjgpu_last_error(), for every single defect and for
a few pairs of defects, which pin the order of the checks.  They need a resident scene, so they run on the device too; every buffer they
pass is a real device buffer of the frame's size (the "overlap" defects point into one larger buffer), so a call that slipped through its
refusal would render a frame and not follow a wild address.

tests/frame_ledger.json is the expected table; `python tests/test_gpu_frame_ledger.py --record` writes it: it observes every case in two
child processes, one after the other, and keeps a field only where the two agree (it prints the fields it drops).  The table is not
recorded again when the loop changes: a difference is a change of behaviour.

Frames are at most 96 x 64 with 32 x 32 tiles and a ragged last tile.  Two paths of the loop cannot be provoked at these sizes and have
no case: the halving of the batch after a failed allocation, and the second render after the split shadow rays overflowed their queue."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "frame_ledger.json")

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("batches", "closest_launches", "light_loop_launches", "shadow_walk_launches", "trace_launches", "rays_sorted")
BATCH_TILES = (0, 1)


def _mods():
    import test_gpu_parity as tp
    import test_gpu_shade_stores as ss
    from edge_scenes import custom_scene
    from fujiyama_renderer_amd import ffi, gpu, workloads
    return tp, ss, custom_scene, ffi, gpu, workloads


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint32).tobytes()).hexdigest()


def ledger(st, gs, prefix=""):
    out = {prefix + "rays." + k: v for k, v in st.rays.as_dict().items()}
    for k in STAT_FIELDS:
        out[prefix + k] = int(getattr(st, k))
    out[prefix + "accum_memsets"] = int(gs.query("accum_memsets"))
    return out


def _frame(text, batch_tiles, options=(), hashed=False):
    """one frame of `text` on a new scene -> its ledger"""
    tp, _, _, _, gpu, _ = _mods()
    sp, rd = tp.prepare(text)
    assert rd.xres <= 96 and rd.yres <= 64 and (rd.tile_w, rd.tile_h) == (32, 32) and (rd.xres % 32 or rd.yres % 32)
    gs = gpu.Scene(sp)
    try:
        gs.set_option("batch_tiles", batch_tiles)
        for name, value in options:
            gs.set_option(name, value)
        fb, st = gs.render_frame(rd)
        out = ledger(st, gs)
    finally:
        gs.close()
    assert st.batches == (gpu.tile_count(rd) if batch_tiles else 1)
    if hashed:
        out["sha256"] = sha(fb)
    return out


def _glass(asset_dir):
    _, ss, custom_scene, _, _, _ = _mods()
    return custom_scene(asset_dir, res=(90, 60), obj_shader="glass_shader", ren_props=ss.TILES)


def case_fixed_grid_three_lights(asset_dir, bt):
    _, ss, _, _, _, _ = _mods()
    out = _frame(ss.lone_object(asset_dir), bt)
    assert out["rays.shadow"] > 0 and out["accum_memsets"] == 0
    return out


def case_reproducible(asset_dir, bt):
    _, ss, _, _, _, _ = _mods()
    out = _frame(ss._reproducible(asset_dir, False), bt, hashed=True)
    assert out["rays.reflect"] == out["rays.refract"] == 0
    return out


def _glass_frame(asset_dir, bt, speculate, options=()):
    _, _, _, _, gpu, _ = _mods()
    gpu.global_option("speculative_walk", speculate)
    try:
        out = _frame(_glass(asset_dir), bt, options)
    finally:
        gpu.global_option("speculative_walk", 1)
    assert out["rays.reflect"] > 0 and out["rays.refract"] > 0          # two children per hit, levels beyond the first
    return out


def case_glass_host_waits_at_every_level(asset_dir, bt):
    return _glass_frame(asset_dir, bt, 0)


def case_glass_speculative_walk(asset_dir, bt):
    return _glass_frame(asset_dir, bt, 1)


def case_glass_overlap_shadow(asset_dir, bt):
    return _glass_frame(asset_dir, bt, 1, (("overlap_shadow", 1),))


def case_glass_sorted_rays(asset_dir, bt):
    _, _, _, _, gpu, _ = _mods()
    gpu.global_option("ray_sort", 4)
    gpu.global_option("ray_sort_min", 1)
    try:
        out = _frame(_glass(asset_dir), bt)
    finally:
        gpu.global_option("ray_sort", -1)
        gpu.global_option("ray_sort_min", 1 << 16)
    assert out["rays_sorted"] == out["rays.reflect"] + out["rays.refract"] > 0
    return out


def case_pathtracing_uid_keyed_streams(asset_dir, bt):
    _, ss, _, _, _, workloads = _mods()
    out = _frame(workloads.cornell(asset_dir, res=(48, 32), spp=(2, 2), mesh="tiny", extra=ss.TILES), bt)
    assert out["rays.diffuse"] > 0
    return out


def case_time_sampled_camera(asset_dir, bt):
    _, ss, _, _, _, workloads = _mods()
    return _frame(workloads.motion(asset_dir, res=(64, 48), spp=(2, 2), mesh="tiny", kind="camera", extra=ss.TILES), bt)


def case_object_motion(asset_dir, bt):
    _, ss, _, _, _, workloads = _mods()
    return _frame(workloads.motion(asset_dir, res=(64, 48), spp=(2, 2), mesh="tiny", kind="object", extra=ss.TILES), bt)


def case_adaptive_sampler(asset_dir, bt):
    tp, ss, _, _, gpu, workloads = _mods()
    # (64 x 64 is two whole tiles each way: the issue's frame for this sampler, the one frame here without a ragged tile)
    sp, rd = tp.prepare(workloads.teapot(asset_dir, res=(64, 64), spp=(1, 1), mesh="tiny", extra=ss.TILES + tp.ADAPTIVE))
    assert rd.sampler_type == 1
    gs = gpu.Scene(sp)
    try:
        gs.set_option("batch_tiles", bt)
        _, st = gs.render_frame(rd)
        out = ledger(st, gs)
    finally:
        gs.close()
    assert out["accum_memsets"] == out["batches"] == (4 if bt else 1)
    return out


def case_variance_entry_point(asset_dir, bt):
    tp, ss, _, _, gpu, _ = _mods()
    sp, rd = tp.prepare(ss._reproducible(asset_dir, False))
    gs = gpu.Scene(sp)
    try:
        gs.set_option("batch_tiles", bt)
        fb, var, st = gs.render_frame_variance(rd)
        out = ledger(st, gs)
    finally:
        gs.close()
    out["sha256"] = sha(fb)
    out["sha256_variance"] = sha(var)
    assert var.any()
    return out


def case_listed_tiles_out_of_order(asset_dir, bt):
    import torch
    tp, ss, _, _, gpu, _ = _mods()
    sp, rd = tp.prepare(ss.lone_object(asset_dir))
    assert gpu.tile_count(rd) == 6
    gs = gpu.Scene(sp)
    try:
        gs.set_option("batch_tiles", bt)
        fb = torch.zeros((rd.yres, rd.xres, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        st = gs.render_tiles(rd, [4, 0, 1], fb.data_ptr())          # (the object is in the middle column: tiles 1 and 4)
        out = ledger(st, gs)
    finally:
        gs.close()
    assert out["batches"] == (3 if bt else 1) and out["rays.shadow"] > 0
    return out


def case_second_call_grows_the_arena(asset_dir, bt):
    """the first call of a scene renders in cold-start batches (two tiles' worth of samples here), the second sizes its batch by memory"""
    tp, ss, _, _, gpu, _ = _mods()
    sp, rd = tp.prepare(ss.lone_object(asset_dir))
    per_tile = (2 * rd.tile_w + 2 * 2) * (2 * rd.tile_h + 2 * 2)          # (upper bound of a tile's samples: rate 2, filter margin <= 2)
    gpu.global_option("cold_batch_samples", 2 * per_tile)
    try:
        gs = gpu.Scene(sp)
        try:
            gs.set_option("batch_tiles", bt)
            _, st1 = gs.render_frame(rd)
            out = ledger(st1, gs, "first.")
            out["first.work_bytes"] = int(gs.query("work_bytes"))
            _, st2 = gs.render_frame(rd)
            out.update(ledger(st2, gs, "second."))
            out["second.work_bytes"] = int(gs.query("work_bytes"))
        finally:
            gs.close()
    finally:
        gpu.global_option("cold_batch_samples", 0)
    if bt == 0:
        assert out["first.batches"] > 1 and out["second.batches"] == 1 and out["second.work_bytes"] >= out["first.work_bytes"]
    return out


CASES = {name[5:]: fn for name, fn in sorted(globals().items()) if name.startswith("case_")}


# ------------------------------------------------------------------------------------------------------------------------------- refusals

NAN, INF = float("nan"), float("inf")
_RENDER_DEFECTS = dict(
    xres_0=dict(xres=0), yres_negative=dict(yres=-60), tile_w_0=dict(tile_w=0), tile_h_negative=dict(tile_h=-32),
    region_negative=dict(region=(-1, 0, 90, 60)), region_outside=dict(region=(0, 0, 91, 60)), region_empty=dict(region=(4, 2, 4, 6)),
    region_inverted=dict(region=(0, 40, 90, 20)), rate_x_0=dict(rate_x=0), rate_y_negative=dict(rate_y=-2))
_SAMPLER_DEFECTS = dict(
    sampler_type_2=dict(sampler_type=2), sampler_type_negative=dict(sampler_type=-1),
    adaptive_subdivision_negative=dict(sampler_type=1, adaptive_max_subdivision=-1),
    adaptive_subdivision_9=dict(sampler_type=1, adaptive_max_subdivision=9),
    adaptive_threshold_negative=dict(sampler_type=1, adaptive_max_subdivision=2, adaptive_subdivision_threshold=-.5),
    adaptive_threshold_nan=dict(sampler_type=1, adaptive_max_subdivision=2, adaptive_subdivision_threshold=NAN))
_TILE_DEFECTS = dict(tile_id_negative=dict(tiles=(0, -1)), tile_id_past_the_end=dict(tiles=(6, 0)), tile_id_far=dict(tiles=(1 << 30,)))

REFUSALS = {
    "fjgpu_render_tiles": dict(
        defects=dict(_RENDER_DEFECTS, **dict(_SAMPLER_DEFECTS, **dict(
            _TILE_DEFECTS, null_scene=dict(scene=None), null_render=dict(render=None), null_framebuffer=dict(fb=None)))),
        pairs=[("sampler_type_2", "xres_0"), ("adaptive_subdivision_9", "rate_x_0"), ("xres_0", "tile_id_negative"),
               ("null_framebuffer", "sampler_type_2"), ("xres_0", "rate_x_0"), ("tile_w_0", "region_outside")]),
    "fjgpu_render_tiles_variance": dict(
        defects=dict(_RENDER_DEFECTS, **dict(_TILE_DEFECTS, **dict(
            sampler_type_2=dict(sampler_type=2), adaptive_sampler=dict(sampler_type=1, adaptive_max_subdivision=2),
            adaptive_subdivision_9=dict(sampler_type=1, adaptive_max_subdivision=9),
            null_scene=dict(scene=None), null_render=dict(render=None), null_framebuffer=dict(fb=None), null_variance=dict(variance=None),
            albedo_floor_0=dict(albedo="own", floor=0.), albedo_floor_negative=dict(albedo="own", floor=-1.),
            albedo_floor_nan=dict(albedo="own", floor=NAN), albedo_floor_inf=dict(albedo="own", floor=INF),
            variance_inside_framebuffer=dict(variance="in_fb"), variance_is_albedo=dict(albedo="own", variance="albedo")))),
        pairs=[("null_variance", "xres_0"), ("albedo_floor_0", "xres_0"), ("xres_0", "variance_inside_framebuffer"),
               ("variance_inside_framebuffer", "adaptive_sampler"), ("adaptive_sampler", "tile_id_negative"),
               ("albedo_floor_nan", "null_framebuffer"), ("sampler_type_2", "rate_x_0")]),
}


def refusal_cases(entry):
    e = REFUSALS[entry]
    out = {name: dict(d) for name, d in e["defects"].items()}
    for a, b in e["pairs"]:
        assert not set(e["defects"][a]) & set(e["defects"][b]), (a, b)
        out[a + "+" + b] = dict(e["defects"][a], **e["defects"][b])
    return out


_refusals = None


def observe_refusals(asset_dir):
    """{entry point: {case: [rc, message]}} on one resident scene"""
    global _refusals
    if _refusals is not None:
        return _refusals
    import torch
    tp, ss, _, ffi, gpu, _ = _mods()
    L = gpu.lib()
    sp, rd = tp.prepare(ss.lone_object(asset_dir))
    assert (rd.xres, rd.yres) == (90, 60) and gpu.tile_count(rd) == 6
    px = rd.xres * rd.yres
    fb = torch.zeros(5 * px, dtype=torch.float32, device="cuda")          # the framebuffer, and behind it room for a variance "inside" it
    var = torch.zeros(px, dtype=torch.float32, device="cuda")
    alb = torch.ones(3 * px, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gs = gpu.Scene(sp)
    out = {}
    try:
        for entry in sorted(REFUSALS):
            out[entry] = {}
            for name, d in sorted(refusal_cases(entry).items()):
                r = rd.copy()
                for k, v in d.items():
                    if k == "region":
                        r.region[:] = v
                    elif hasattr(r, k):
                        setattr(r, k, v)
                scene = None if "scene" in d else gs._h
                render = None if "render" in d else C.byref(r)
                fb_p = None if "fb" in d else C.c_void_p(fb.data_ptr())
                ids = np.array(d.get("tiles", (0,)), dtype=np.int32)
                ids_p = ids.ctypes.data_as(C.c_void_p)
                if entry == "fjgpu_render_tiles":
                    rc = L.fjgpu_render_tiles(scene, render, ids_p, len(ids), fb_p, None, None)
                else:
                    alb_p = C.c_void_p(alb.data_ptr()) if d.get("albedo") == "own" else None
                    where = d.get("variance", "own")
                    var_p = {"own": C.c_void_p(var.data_ptr()), None: None, "in_fb": C.c_void_p(fb.data_ptr() + 4 * (4 * px - 8)),
                             "albedo": C.c_void_p(alb.data_ptr())}[where]
                    rc = L.fjgpu_render_tiles_variance(scene, render, ids_p, len(ids), fb_p, alb_p, C.c_float(d.get("floor", 1e-4)), var_p,
                                                       None, None)
                out[entry][name] = [int(rc), L.fjgpu_last_error().decode()]
    finally:
        gs.close()
    _refusals = out
    return out


# ---------------------------------------------------------------------------------------------------------------------------------- tests

def expected():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.parametrize("batch_tiles", BATCH_TILES, ids=["one_batch", "a_batch_per_tile"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_frame_ledger(case, batch_tiles, asset_dir):
    want = expected()["frames"][case][str(batch_tiles)]
    got = CASES[case](asset_dir, batch_tiles)
    print("%s, batch_tiles %d: %s" % (case, batch_tiles, json.dumps(got, sort_keys=True)))
    assert want and set(want) <= set(got)
    wrong = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not wrong, "\n".join("%s: recorded %r, now %r" % (k, w, g) for k, (w, g) in sorted(wrong.items()))


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_refusals_to_the_letter(entry, asset_dir):
    want, got = expected()["refusals"][entry], observe_refusals(asset_dir)[entry]
    assert sorted(want) == sorted(refusal_cases(entry)), "the table's cases are not the generator's"
    wrong = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    print("%s: %d cases, %d differ" % (entry, len(want), len(wrong)))
    assert not wrong, "\n".join("%s: recorded %r, now %r" % (k, w, g) for k, (w, g) in sorted(wrong.items()))


def test_the_table_holds_every_case_and_only_refusals():
    table = expected()
    assert sorted(table["frames"]) == sorted(CASES)
    for case, by_bt in table["frames"].items():
        assert sorted(by_bt) == [str(b) for b in BATCH_TILES], case
    assert "sha256" in table["frames"]["reproducible"]["0"] and "sha256" in table["frames"]["reproducible"]["1"]
    for entry, t in table["refusals"].items():
        for name, (rc, msg) in t.items():
            assert rc < 0 and msg, (entry, name)


# --------------------------------------------------------------------------------------------------------------------------------- record

def observe_all():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from fujiyama_renderer_amd import workloads
    asset_dir = workloads.default_asset_dir()
    os.makedirs(asset_dir, exist_ok=True)
    frames = {case: {str(bt): CASES[case](asset_dir, bt) for bt in BATCH_TILES} for case in sorted(CASES)}
    return dict(frames=frames, refusals=observe_refusals(asset_dir))


def _child():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--observe"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def record():
    a = _child()
    b = _child()
    dropped = []
    for case, by_bt in a["frames"].items():
        for bt, fields in by_bt.items():
            for k in sorted(fields):
                if b["frames"][case][bt].get(k) != fields[k]:
                    dropped.append("%s[%s].%s: %r / %r" % (case, bt, k, fields[k], b["frames"][case][bt].get(k)))
                    del fields[k]
    assert a["refusals"] == b["refusals"], "the refusals differ between two recordings"
    with open(TABLE, "w") as f:
        json.dump(a, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d frames, %d refusals" % (sum(len(v) for v in a["frames"].values()), sum(len(v) for v in a["refusals"].values())))
    print("fields dropped because two recordings differ: %s" % (dropped or "none"))


if __name__ == "__main__":
    if sys.argv[1:] == ["--observe"]:
        print("RESULT " + json.dumps(observe_all()))
    elif sys.argv[1:] == ["--record"]:
        record()
    else:
        sys.exit("usage: %s --record" % sys.argv[0])
