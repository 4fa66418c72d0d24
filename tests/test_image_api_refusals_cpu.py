"""The refusals of the six image-space entry points (csrc/device/fjgpu_image_api.hip), pinned to the letter: return code and the whole
text of fjgpu_last_error() for a valid call, for every single defect of its arguments and for every pair of defects that can be applied
together.  The pairs pin the ORDER of the checks, which differs between the entry points and is part of their behaviour.

tests/image_api_refusals.json is the expected table {entry point: {case: [rc, message]}}; `python tests/test_image_api_refusals_cpu.py
--record` writes it, with the child code the test runs.  It was recorded before the entry points were moved out of fjgpu_api.hip and is
not recorded again when they change: a difference is a change of behaviour.

A call is a dict of values (BASE); a defect is a dict of the values it replaces, and two defects can be applied together when they
replace different values.  Addresses are fake: non-NULL, 16-byte aligned, 4 KiB apart (frames are 16 x 8, the largest buffer is 2 KiB).
Every case runs in ONE child process that sees no device and checks that first, so a case that slipped through its refusal stops at
"no HIP device is visible" (-1) and never follows an address.  A pair that answers -1 shows that its two defects cancel; such pairs are
listed in DROPPED, with the reason, and nothing else is.

The entry "fjgpu_denoise_estimate_variance_albedo(albedo=NULL)" is that entry point called without an albedo: it answers with the plain
entry point's name.
"""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "image_api_refusals.json")
F = [4096 * k for k in range(1, 24)]
NAN, INF = float("nan"), float("inf")
FILTER_ROWS, TEMPORAL_ROWS = 65535 * 4, 65535 * 16          # the row limits: one row over each is a defect


def _merge(*ds):
    out = {}
    for d in ds:
        out.update(d)
    return out


# ---- the denoise family: fjgpu_denoise_desc and the buffers of each entry point
_DN_DESC = dict(null_desc=False, xres=16, yres=8, region=(0, 0, 16, 8), iterations=3, sigma_color=1.0, sigma_normal=1.0, sigma_position=1.0)
_DN_DEFECTS = dict(
    null_desc=dict(null_desc=True), xres_0=dict(xres=0), yres_negative=dict(yres=-8),
    region_empty=dict(region=(4, 2, 4, 6)), region_outside=dict(region=(0, 0, 17, 8)), region_negative=dict(region=(-1, 0, 16, 8)),
    region_inverted=dict(region=(0, 6, 16, 2)), rows_over=dict(yres=FILTER_ROWS + 1, region=(0, 0, 16, FILTER_ROWS + 1)),
    nan_color=dict(sigma_color=NAN), nan_normal=dict(sigma_normal=NAN), nan_position=dict(sigma_position=NAN))
_ITERATIONS = dict(iterations_0=dict(iterations=0), iterations_9=dict(iterations=9), iterations_negative=dict(iterations=-1))
_FLOORS = dict(floor_0=dict(floor=0.0), floor_negative=dict(floor=-1.0), floor_nan=dict(floor=NAN), floor_inf=dict(floor=INF))

ENTRIES = {
    "fjgpu_denoise": dict(
        base=_merge(_DN_DESC, dict(cin=F[0], cout=F[1])),
        defects=_merge(_DN_DEFECTS, _ITERATIONS, dict(
            null_in=dict(cin=None), null_out=dict(cout=None), misaligned_in=dict(cin=F[0] + 4), misaligned_out=dict(cout=F[1] + 8)))),
    "fjgpu_denoise_albedo": dict(
        base=_merge(_DN_DESC, dict(cin=F[0], cout=F[1], albedo=F[2], floor=0.05)),
        defects=_merge(_DN_DEFECTS, _ITERATIONS, _FLOORS, dict(
            null_in=dict(cin=None), null_out=dict(cout=None), misaligned_in=dict(cin=F[0] + 4), misaligned_out=dict(cout=F[1] + 8)))),
    "fjgpu_denoise_estimate_variance": dict(
        base=_merge(_DN_DESC, dict(iterations=0, color=F[0], vout=F[1])),          # iterations is not the estimate's business
        defects=_merge(_DN_DEFECTS, dict(
            null_color=dict(color=None), null_out=dict(vout=None), misaligned_color=dict(color=F[0] + 4),
            out_is_color=dict(color=F[3], vout=F[3])))),
    "fjgpu_denoise_estimate_variance_albedo": dict(
        base=_merge(_DN_DESC, dict(iterations=0, color=F[0], vout=F[1], albedo=F[2], floor=0.05)),
        defects=_merge(_DN_DEFECTS, _FLOORS, dict(
            null_color=dict(color=None), null_out=dict(vout=None), misaligned_color=dict(color=F[0] + 4),
            out_is_color=dict(color=F[3], vout=F[3]), out_is_albedo=dict(albedo=F[4], vout=F[4])))),
    "fjgpu_denoise_estimate_variance_albedo(albedo=NULL)": dict(
        base=_merge(_DN_DESC, dict(iterations=0, color=F[0], vout=F[1], albedo=None, floor=0.0)),
        defects=_merge(_DN_DEFECTS, dict(
            null_color=dict(color=None), null_out=dict(vout=None), misaligned_color=dict(color=F[0] + 4),
            out_is_color=dict(color=F[3], vout=F[3])))),
    "fjgpu_denoise_variance": dict(
        base=_merge(_DN_DESC, dict(sl=4.0, cin=F[0], cout=F[1], albedo=F[2], floor=0.05, vin=F[3], vout=F[4])),
        defects=_merge(_DN_DEFECTS, _ITERATIONS, _FLOORS, dict(
            null_in=dict(cin=None), null_out=dict(cout=None), misaligned_in=dict(cin=F[0] + 4), misaligned_out=dict(cout=F[1] + 8),
            nan_luminance=dict(sl=NAN), vout_is_vin=dict(vin=F[5], vout=F[5]), vout_is_cin=dict(cin=F[6], vout=F[6]),
            vout_is_cout=dict(cout=F[7], vout=F[7]), vin_is_cout=dict(vin=F[8], cout=F[8])))),
    # ---- the temporal pass: fjgpu_temporal_desc, the two frames' guides, the view of the previous frame and the two histories
    "fjgpu_denoise_temporal": dict(
        base=dict(null_desc=False, xres=16, yres=8, region=(0, 0, 16, 8), alpha_min=0.1, max_history=8.0, tol_position=0.5, cos_normal=0.9,
                  min_history_variance=4.0, albedo_floor=1e-4, color=F[0], position=F[1], normal=F[2], ids=F[3], albedo=None, vs=None,
                  null_view=False, view_xres=16, view_yres=8, pp=F[4], pn=F[5], pi=F[6], vout=F[7], null_prev=False, prev_color=F[8],
                  prev_moments=F[9], prev_length=F[10], null_next=False, next_color=F[11], next_moments=F[12], next_length=F[13]),
        defects=dict(
            null_desc=dict(null_desc=True), null_color=dict(color=None), null_position=dict(position=None), null_normal=dict(normal=None),
            null_ids=dict(ids=None), null_next=dict(null_next=True), null_next_member=dict(next_moments=None),
            null_prev_member=dict(prev_length=None), null_prev_view=dict(null_view=True), null_prev_ids=dict(pi=None),
            null_prev_position=dict(pp=None), xres_0=dict(xres=0), yres_negative=dict(yres=-8),
            region_empty=dict(region=(4, 2, 4, 6)), region_outside=dict(region=(0, 0, 17, 8)), region_negative=dict(region=(0, -1, 16, 8)),
            rows_over=dict(yres=TEMPORAL_ROWS + 1, region=(0, 0, 16, TEMPORAL_ROWS + 1)),
            alpha_0=dict(alpha_min=0.0), alpha_above_1=dict(alpha_min=1.5), alpha_negative=dict(alpha_min=-0.5),
            max_history_0=dict(max_history=0.5), nan_alpha=dict(alpha_min=NAN), nan_max_history=dict(max_history=NAN),
            nan_tol=dict(tol_position=NAN), nan_cos=dict(cos_normal=NAN), nan_min_history=dict(min_history_variance=NAN),
            nan_floor=dict(albedo_floor=NAN), bad_floor=dict(albedo=F[14], albedo_floor=0.0), floor_inf=dict(albedo=F[14], albedo_floor=INF),
            next_is_prev=dict(next_color=F[8], next_moments=F[9], next_length=F[10]), next_color_is_color=dict(next_color=F[0]),
            next_overlaps_prev=dict(next_color=F[8] + 16), variance_out_is_spatial=dict(vs=F[15], vout=F[15]),
            next_members_equal=dict(next_moments=F[13]), misaligned_color=dict(color=F[0] + 4), misaligned_next=dict(next_color=F[11] + 8),
            misaligned_prev=dict(prev_color=F[8] + 4), bad_view=dict(view_xres=0))),
}

# pairs whose two defects cancel, so that the call reaches the device check: {entry point: [(defect, defect, why)]}
DROPPED = {}


def cases(entry):
    """{case name: the values of the call}: the base call, each defect, each pair of defects that replace different values"""
    e = ENTRIES[entry]
    out = {"valid": dict(e["base"])}
    for name, d in sorted(e["defects"].items()):
        out[name] = _merge(e["base"], d)
    dropped = {(a, b) for a, b, _ in DROPPED.get(entry, [])}
    for a, b in itertools.combinations(sorted(e["defects"]), 2):
        da, db = e["defects"][a], e["defects"][b]
        if set(da) & set(db) or (a, b) in dropped:
            continue
        out[a + "+" + b] = _merge(e["base"], da, db)
    return out


def _denoise_desc(ffi, v):
    d = ffi.DenoiseDesc()
    d.xres, d.yres, d.iterations, d.stop_at_ids = v["xres"], v["yres"], v["iterations"], 1
    d.region[:] = v["region"]
    d.sigma_color, d.sigma_normal, d.sigma_position = v["sigma_color"], v["sigma_normal"], v["sigma_position"]
    return None if v["null_desc"] else C.byref(d)


def call(L, ffi, entry, v):
    """one call of `entry` with the values `v` -> [rc, message]"""
    name = entry.split("(")[0]
    if name == "fjgpu_denoise":
        rc = L.fjgpu_denoise(0, _denoise_desc(ffi, v), v["cin"], None, None, None, v["cout"], None, None)
    elif name == "fjgpu_denoise_albedo":
        rc = L.fjgpu_denoise_albedo(0, _denoise_desc(ffi, v), v["cin"], None, None, None, v["albedo"], v["floor"], v["cout"], None, None)
    elif name == "fjgpu_denoise_estimate_variance":
        rc = L.fjgpu_denoise_estimate_variance(0, _denoise_desc(ffi, v), v["color"], None, None, None, v["vout"], None, None)
    elif name == "fjgpu_denoise_estimate_variance_albedo":
        rc = L.fjgpu_denoise_estimate_variance_albedo(0, _denoise_desc(ffi, v), v["color"], None, None, None, v["albedo"], v["floor"], v["vout"],
                                                      None, None)
    elif name == "fjgpu_denoise_variance":
        rc = L.fjgpu_denoise_variance(0, _denoise_desc(ffi, v), v["sl"], v["cin"], None, None, None, v["albedo"], v["floor"], v["vin"], v["cout"],
                                      v["vout"], None, None)
    else:
        d = ffi.TemporalDesc()
        d.xres, d.yres = v["xres"], v["yres"]
        d.region[:] = v["region"]
        for k in ("alpha_min", "max_history", "tol_position", "cos_normal", "min_history_variance", "albedo_floor"):
            setattr(d, k, v[k])
        view = ffi.View()
        view.xres, view.yres = v["view_xres"], v["view_yres"]
        view.uv_size[:] = (1.0, 0.5)
        prev, nxt = ffi.TemporalHistory(), ffi.TemporalHistory()
        prev.color, prev.moments, prev.length = v["prev_color"], v["prev_moments"], v["prev_length"]
        nxt.color, nxt.moments, nxt.length = v["next_color"], v["next_moments"], v["next_length"]
        rc = L.fjgpu_denoise_temporal(0, None if v["null_desc"] else C.byref(d), v["color"], v["position"], v["normal"], v["ids"], v["albedo"],
                                      v["vs"], None if v["null_view"] else C.byref(view), v["pp"], v["pn"], v["pi"],
                                      None if v["null_prev"] else C.byref(prev), None if v["null_next"] else C.byref(nxt), v["vout"], None, None)
    return [rc, L.fjgpu_last_error().decode()]


def child():
    """every case of every entry point, in a process that sees no device"""
    sys.path.insert(0, ROOT)
    from fujiyama_renderer_amd import ffi, gpu
    assert gpu.device_count() == 0, "a device is visible"
    L = gpu.lib()
    out = {entry: {name: call(L, ffi, entry, v) for name, v in cases(entry).items()} for entry in sorted(ENTRIES)}
    print("RESULT " + json.dumps(out))


_observed = None


def observed():
    global _observed
    if _observed is None:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stdout
        _observed = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    return _observed


def expected():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_to_the_letter(entry):
    want, got = expected()[entry], observed()[entry]
    assert sorted(want) == sorted(cases(entry)), "the table's cases are not the generator's"
    wrong = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    print("%s: %d cases, %d differ" % (entry, len(want), len(wrong)))
    assert not wrong, "\n".join("%s: expected %r, got %r" % (k, w, g) for k, (w, g) in sorted(wrong.items())[:20])


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_only_the_valid_call_reaches_the_device_check(entry):
    """the table itself: -1 and "<name>: no HIP device is visible" for the valid call, -2 under the entry point's prefix for every other
    case (fjgpu_denoise's prefix for both of its entry points, but for the albedo floor's refusal)"""
    want = expected()[entry]
    name = entry.split("(")[0]
    said = {"fjgpu_denoise_albedo": "fjgpu_denoise", "fjgpu_denoise_estimate_variance_albedo(albedo=NULL)": "fjgpu_denoise_estimate_variance"}.get(entry, name)
    assert want["valid"] == [-1, said + ": no HIP device is visible"]
    for k, (rc, msg) in want.items():
        if k != "valid":
            assert rc == -2 and (msg.startswith(said + ": ") or msg.startswith(name + ": albedo_floor")), (k, rc, msg)


def test_dropped_pairs_are_few():
    """at most one pair in ten per entry point, each of two defects that exist and could have been applied together"""
    for entry, pairs in DROPPED.items():
        defects = ENTRIES[entry]["defects"]
        possible = [1 for a, b in itertools.combinations(sorted(defects), 2) if not set(defects[a]) & set(defects[b])]
        assert 10 * len(pairs) <= len(possible), entry
        for a, b, why in pairs:
            assert a < b and not set(defects[a]) & set(defects[b]) and why, (entry, a, b)


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()
    elif sys.argv[1:] == ["--record"]:
        table = observed()
        with open(TABLE, "w") as f:
            # one case per line
            f.write("{\n" + ",\n".join("%s: {\n%s\n}" % (json.dumps(e), ",\n".join("%s: %s" % (json.dumps(k), json.dumps(t[k])) for k in sorted(t)))
                                       for e, t in sorted(table.items())) + "\n}\n")
        print("recorded %s" % ", ".join("%s: %d" % (k, len(v)) for k, v in sorted(table.items())))
        print("cases that reach the device check:", [(e, k) for e, t in table.items() for k, (rc, _) in t.items() if rc != -2 and k != "valid"])
    else:
        sys.exit("usage: %s --record" % sys.argv[0])
