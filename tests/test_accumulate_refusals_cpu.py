"""The refusals of fjgpu_accumulate and fjgpu_accumulate_tile_error (include/fjgpu.h; csrc/device/fjgpu_image_api.hip), to the letter, and
their order.

As in tests/test_image_api_refusals_cpu.py the calls run in ONE child process that sees no device and checks that first: addresses are
fake (non-NULL, 16-byte aligned, 64 KiB apart; the frame is 16 x 8, the largest buffer 2 KiB), every refusal is decided before any device
call, and a case that slipped through its refusal stops at "no HIP device is visible" (-1) and never follows an address.  Only the
rectangle list is real host memory: the entries read it.

ORDER lists the defects of each entry from the first check to the last; every pair of defects that can be applied together must answer
with the message of the one that comes first.
"""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = [65536 * k for k in range(1, 12)]
NAN, INF = float("nan"), float("inf")
PX = 16 * 8 * 4                         # bytes of one f32 plane

A, E = "fjgpu_accumulate: ", "fjgpu_accumulate_tile_error: "
_NULL_A = A + "null argument (color, state and its mean, m2 and count are required)"
_NULL_E = E + "null argument (state, its mean, m2 and count, and errors_out are required)"
_RECT = "rect %d must be a non-empty rectangle inside the frame"

ENTRIES = {
    "fjgpu_accumulate": dict(
        base=dict(xres=16, yres=8, rects=[(0, 0, 16, 8)], n_rects=None, color=F[0], null_state=False, mean=F[1], m2=F[2], count=F[3], vout=F[4]),
        valid_variants=dict(whole_frame=dict(rects=None, n_rects=0), no_variance=dict(vout=None), reset=dict(reset=1),
                            whole_frame_ignores_n=dict(rects=None, n_rects=-3)),
        # (defect, the values it replaces, the message), first check first
        order=[
            ("null_color", dict(color=None), _NULL_A), ("null_state", dict(null_state=True), _NULL_A), ("null_mean", dict(mean=None), _NULL_A),
            ("null_m2", dict(m2=None), _NULL_A), ("null_count", dict(count=None), _NULL_A),
            ("xres_0", dict(xres=0), A + "resolution must be positive"), ("yres_negative", dict(yres=-8), A + "resolution must be positive"),
            ("n_rects_negative", dict(n_rects=-1), A + "n_rects is negative"),
            ("rect_empty", dict(rects=[(0, 0, 16, 8), (4, 2, 4, 6)]), A + _RECT % 1), ("rect_outside", dict(rects=[(0, 0, 17, 8)]), A + _RECT % 0),
            ("rect_negative", dict(rects=[(0, -1, 16, 8)]), A + _RECT % 0), ("rect_inverted", dict(rects=[(0, 6, 16, 2)]), A + _RECT % 0),
            ("color_is_mean", dict(color=F[5], mean=F[5]), A + "color overlaps a plane of the state"),
            ("color_overlaps_m2", dict(m2=F[0] + 4 * PX - 16), A + "color overlaps a plane of the state"),
            ("vout_is_count", dict(vout=F[6], count=F[6]), A + "variance_out overlaps a plane of the state"),
            ("vout_overlaps_mean", dict(vout=F[1] + 4 * PX - 4), A + "variance_out overlaps a plane of the state"),
            ("misaligned_color", dict(color=F[0] + 4), A + "color and the state's mean must be 16-byte aligned"),
            ("misaligned_mean", dict(mean=F[1] + 8), A + "color and the state's mean must be 16-byte aligned"),
        ]),
    "fjgpu_accumulate_tile_error": dict(
        base=dict(xres=16, yres=8, rects=[(0, 0, 16, 8)], n_rects=None, null_state=False, mean=F[1], m2=F[2], count=F[3], floor=1e-3, errors=F[7]),
        valid_variants=dict(whole_frame=dict(rects=None, n_rects=0)),
        order=[
            ("null_state", dict(null_state=True), _NULL_E), ("null_mean", dict(mean=None), _NULL_E), ("null_m2", dict(m2=None), _NULL_E),
            ("null_count", dict(count=None), _NULL_E), ("null_errors", dict(errors=None), _NULL_E),
            ("xres_0", dict(xres=0), E + "resolution must be positive"), ("yres_negative", dict(yres=-8), E + "resolution must be positive"),
            ("n_rects_negative", dict(n_rects=-1), E + "n_rects is negative"),
            ("rect_empty", dict(rects=[(4, 2, 4, 6)]), E + _RECT % 0), ("rect_outside", dict(rects=[(0, 0, 16, 8), (0, 0, 16, 9)]), E + _RECT % 1),
            ("floor_0", dict(floor=0.0), E + "lum_floor must be finite and > 0"), ("floor_negative", dict(floor=-1.0), E + "lum_floor must be finite and > 0"),
            ("floor_nan", dict(floor=NAN), E + "lum_floor must be finite and > 0"), ("floor_inf", dict(floor=INF), E + "lum_floor must be finite and > 0"),
            ("misaligned_mean", dict(mean=F[1] + 4), E + "the state's mean must be 16-byte aligned"),
        ]),
}


def cases(entry):
    """{case: (values, expected [rc, message])}: the valid calls, each defect, each pair of defects that replace different values"""
    e = ENTRIES[entry]
    gone = [-1, entry + ": no HIP device is visible"]
    out = {"valid": (dict(e["base"]), gone)}
    for name, d in e["valid_variants"].items():
        out["valid:" + name] = (dict(e["base"], **d), gone)
    for name, d, msg in e["order"]:
        out[name] = (dict(e["base"], **d), [-2, msg])
    for (na, da, ma), (nb, db, _) in itertools.combinations(e["order"], 2):
        if not set(da) & set(db):
            out[na + "+" + nb] = (dict(e["base"], **dict(da, **db)), [-2, ma])
    return out


def call(L, ffi, entry, v):
    import numpy as np
    st = ffi.AccumState()
    st.mean, st.m2, st.count = v["mean"], v["m2"], v["count"]
    stp = None if v["null_state"] else C.byref(st)
    if v["rects"] is None:
        keep, rp, n = None, None, 0
    else:
        keep = np.ascontiguousarray(v["rects"], dtype=np.int32).reshape(-1, 4)
        rp, n = keep.ctypes.data_as(C.c_void_p), len(keep)
    if v["n_rects"] is not None:
        n = v["n_rects"]
    if entry == "fjgpu_accumulate":
        rc = L.fjgpu_accumulate(0, v["xres"], v["yres"], rp, n, v["color"], stp, v.get("reset", 0), v["vout"], None, None)
    else:
        rc = L.fjgpu_accumulate_tile_error(0, v["xres"], v["yres"], rp, n, stp, v["floor"], v["errors"], None, None)
    return [rc, L.fjgpu_last_error().decode()]


def child():
    sys.path.insert(0, ROOT)
    from fujiyama_renderer_amd import ffi, gpu
    assert gpu.device_count() == 0, "a device is visible"
    L = gpu.lib()
    out = {entry: {name: call(L, ffi, entry, v) for name, (v, _) in cases(entry).items()} for entry in sorted(ENTRIES)}
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


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusals_and_their_order(entry):
    got = observed()[entry]
    want = {k: w for k, (_, w) in cases(entry).items()}
    assert sorted(got) == sorted(want)
    wrong = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    print("%s: %d cases, %d differ" % (entry, len(want), len(wrong)))
    assert not wrong, "\n".join("%s: expected %r, got %r" % (k, w, g) for k, (w, g) in sorted(wrong.items())[:20])


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_message_starts_with_the_entrys_name(entry):
    for k, (rc, msg) in observed()[entry].items():
        assert msg.startswith(entry + ": "), (k, msg)
        assert rc == (-1 if k.startswith("valid") else -2), (k, rc, msg)


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        child()
    else:
        sys.exit("usage: run under pytest")
