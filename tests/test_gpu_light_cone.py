"""GPU suite, per-light shadow cones (-m gpu): the light loop (k_shadow_cull) of whole-ray launches settles the box misses of its
(point, light) pairs with a cone built once per (single-instance shadow group, light sample) at scene creation
(fujiyama-renderer_amd/csrc/device/fjgpu_light_cone.h), and runs the reciprocals and the six-plane box test for what the cone leaves open.

Every case renders with the scene option `light_cones` 1 and 0 (0: the instantiation without cones, the parent's code).  What has to
hold on both: the oracle's pixels and ray counts per context, and between the two settings equal `insts_tested` and `rays.shadow` in the
counting frame -- a cone verdict counts the event the box test counted.  (`shadow_traversed` is whole 512-slot chunks per wave and moves
by a chunk from run to run: not compared.)  The queries `light_cone_rows` / `light_cone_records` say what the scene's table holds.
"""
import numpy as np
import pytest

import oracle_ffi
import test_gpu_parity as tg
from fujiyama_renderer_amd import gpu, workloads

SHAPE = dict(res=(64, 48), spp=(2, 2))


def with_props(text, *lines):
    """the scene text with commands inserted before the frame buffer is made (a later SetProperty replaces an earlier one)"""
    head, sep, tail = text.rpartition("NewFrameBuffer ")
    assert sep
    return head + "".join(l + "\n" for l in lines) + sep + tail


def both_settings(text):
    """-> ({1: (fb, stats), 0: (fb, stats)}, rows, records): counting and production frame per setting on ONE resident scene, the oracle once"""
    sp, rd = tg.prepare(text)
    tg._last["adaptive"] = rd.sampler_type == 1
    gs = gpu.Scene(sp)
    got = {}
    for cones in (1, 0):
        gs.set_option("light_cones", cones)
        gs.set_option("count_nodes", 1)
        fb, st = gs.render_frame(rd)
        gs.set_option("count_nodes", 0)
        fb2, _ = gs.render_frame(rd)
        assert float(tg.rel_err(fb, fb2).max()) <= 1e-6
        got[cones] = (fb, st)
    rows, records = int(gs.query("light_cone_rows")), int(gs.query("light_cone_records"))
    gs.close()
    osc = oracle_ffi.OracleScene(sp)
    ref, rc = osc.render(rd)
    osc.close()
    for cones in (1, 0):
        tg.assert_parity(got[cones][0], got[cones][1], ref, rc)
    on, off = got[1][1], got[0][1]
    print("rows %d records %d | insts_tested %d / %d, shadow rays %d / %d, shadow_traversed %d / %d" % (
        rows, records, on.insts_tested, off.insts_tested, on.rays.shadow, off.rays.shadow, on.shadow_traversed, off.shadow_traversed))
    assert on.insts_tested == off.insts_tested
    assert on.rays.shadow == off.rays.shadow == rc.shadow
    return got, rows, records


def headline(asset_dir, *lines):
    return with_props(workloads.dragon(asset_dir, mesh="tiny", nlights=4, **SHAPE), *lines)


# the headline with a second, smaller dragon in a group of its own: the floor's and the small dragon's shadow rays go to group1 (the dragon), the dragon's to group2
TWO_GROUPS = ("SetProperty3 dragon_shader0 diffuse 0.6 0.3 0.2",
              "NewObjectInstance dragon2 dragon_mesh",
              "SetProperty3 dragon2 scale 0.3 0.3 0.3",
              "SetProperty3 dragon2 translate -1.3 0 1.2",
              "AssignShader dragon2 DEFAULT_SHADING_GROUP dragon_shader0",
              "NewObjectGroup group2",
              "AddObjectToGroup group2 dragon2",
              "AssignObjectGroup dragon1 shadow_target group2",
              "AssignObjectGroup dragon2 shadow_target group1")


def group_box(text, group=0):
    """the reference box of the single-instance group (DGroup.sbounds: the instance's bounds + 1e-4, the statement of the scene builder)"""
    sp, rd = tg.prepare(text)
    inst, skip, box = gpu.host_instance_level(sp, group)
    assert len(inst) == 1
    return np.concatenate([box[0, :3] - .0001, box[0, 3:] + .0001])


@pytest.mark.gpu
def test_headline_scene_small(asset_dir):
    """the floor's pairs miss the dragon's box (the cone's verdict) but for the shadow's neighbourhood, which is queued"""
    got, rows, records = both_settings(headline(asset_dir))
    assert (rows, records) == (1, 4)
    assert got[1][1].rays.shadow > 0 and got[1][1].shadow_traversed > 0


@pytest.mark.gpu
def test_a_light_inside_the_box(asset_dir):
    """no cone for that light: its pairs take the box test, the other three lights' the cones"""
    b = group_box(headline(asset_dir))
    c = .5 * (b[:3] + b[3:])
    got, rows, records = both_settings(headline(asset_dir, "SetProperty3 light1 translate %r %r %r" % (float(c[0]), float(c[1]), float(c[2]))))
    assert (rows, records) == (1, 3)


@pytest.mark.gpu
def test_a_light_level_with_a_box_face(asset_dir):
    """a light in the plane of the box's top face, beside the box: the classification is ambiguous on that axis, no cone"""
    b = group_box(headline(asset_dir))
    got, rows, records = both_settings(headline(asset_dir, "SetProperty3 light2 translate %r %r %r" % (float(b[3] + 2.5), float(b[4]), float(b[5] + 1.5))))
    assert (rows, records) == (1, 3)


@pytest.mark.gpu
def test_a_light_far_away(asset_dir):
    got, rows, records = both_settings(headline(asset_dir, "SetProperty3 light3 translate 10000 12 3000"))
    assert (rows, records) == (1, 4)


@pytest.mark.gpu
def test_dome_light_scene_small(asset_dir):
    """many fixed light samples, all of them 1e38 away: the 1e-9 margin of a cone from there is wider than any box, so none is built
    and the launches take the instantiation without cones; the option changes nothing"""
    got, rows, records = both_settings(workloads.ibl(asset_dir, mesh="small", sample_count=48, **SHAPE))
    assert records == 0 and rows == 0


@pytest.mark.gpu
def test_two_single_instance_groups_in_one_frame(asset_dir):
    """the floor's records name group1 (the dragon), the dragon's name group2 (a second, smaller dragon) and the small dragon's group1 again:
    waves whose 64 records straddle an outline hold records of different groups and take the box test, the others their group's cones"""
    text = headline(asset_dir, *TWO_GROUPS)
    got, rows, records = both_settings(text)
    assert (rows, records) == (2, 8)
    assert got[1][1].shadow_traversed > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name, build", [
    ("crowd_split_loop", lambda a: workloads.crowd(a, mesh="tiny", n=4, nlights=3, **SHAPE)),
    ("area_lights", lambda a: workloads.arealights(a, mesh="tiny", kind="both", **SHAPE)),
    ("fur", lambda a: workloads.furry(a, mesh="furball", nlights=2, **SHAPE)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_scenes_the_cones_leave_alone(name, build, asset_dir):
    """groups of several instances (the split loop), area lights (positions drawn per event) and fur (the hair instantiation) take the
    parent's kernels whatever the option says"""
    both_settings(build(asset_dir))
