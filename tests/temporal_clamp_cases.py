"""The cases of fjgpu_denoise_temporal_clamped that both suites run (tests/test_temporal_clamp_cpu.py through the host twin,
tests/test_gpu_temporal_clamp.py on the device), on the analytic scene of tests/temporal_scene.py: 37 x 29 with region (3, 2, 34, 27).

`run(cur, prev, prev_hist, albedo, vs, out=None, var_out=None, clamp=None, amount=None, **params) -> (history, variance, amount)`;
clamp is None or (radius, gamma, stop_at_ids), amount an [H, W] float32 array to write into or None.
"""
import numpy as np

import temporal_clamp_model as tcm
import temporal_model as tm
import temporal_scene as ts

W, H, REGION = ts.W, ts.H, ts.REGION
CASES = [(radius, albedo, stop) for radius in (1, 2, 3) for albedo in (False, True) for stop in (0, 1)]
CASE_IDS = ["r%d-%s-%s" % (r, "albedo" if a else "plain", "stop" if s else "nostop") for r, a, s in CASES]
GAMMA = 1.0


def model_run(cur, prev, prev_hist, albedo, vs, out=None, var_out=None, clamp=None, amount=None, details=None, **params):
    return tcm.accumulate(cur["color"], cur["position"], cur["normal"], cur["ids"], albedo=cur["albedo"] if albedo else None, variance_spatial=vs,
                          prev_view=prev["view"] if prev else None, prev_position=prev["position"] if prev else None,
                          prev_normal=prev["normal"] if prev else None, prev_ids=prev["ids"] if prev else None, prev=prev_hist, region=REGION,
                          out=out, variance_out=var_out, clamp=clamp, amount_out=amount, details=details, **params)


def check_equal_to_model(run, radius, albedo, stop, what):
    """the 4-frame pan through `run`, each frame from run's own history, against the model on the same inputs: history length exactly,
    colour, moments, variance and amount within ts.REL_TOL; the clamp must have moved something"""
    clamp = (radius, GAMMA, stop)
    hist, prev, moved = None, None, 0
    for k, cur in enumerate(ts.pan_sequence()):
        vs = ts.spatial_variance(k)
        got, gvar, gamt = run(cur, prev, hist, albedo, vs, clamp=clamp, **ts.PARAMS)
        ref, rvar, ramt = model_run(cur, prev, hist, albedo, vs, clamp=clamp, **ts.PARAMS)
        assert np.array_equal(got["length"], ref["length"]), (what, k)
        for name, a, b in (("color", got["color"], ref["color"]), ("moments", got["moments"], ref["moments"]), ("variance", gvar, rvar),
                           ("amount", gamt, ramt)):
            assert np.isfinite(a).all()
            err = float(tm.rel_err(a, b).max())
            print("clamp %-26s frame %d %-8s max rel err %.3e" % (what, k, name, err))
            assert err <= ts.REL_TOL, (what, k, name, err)
        assert (gamt[~ts.inside()] == 0).all() and (gamt[got["length"] == 1] == 0).all()
        moved += int((gamt > 0).sum())
        hist, prev = got, cur
    assert moved > 100, moved


def ghost_frames():
    """six frames of the 0.4-pixel pan, noise 0.1, seeds 100 + k; from frame 4 on the sphere's clean rgb is multiplied by 0.3 (every guide
    stays put) and the noise is added afterwards"""
    out = []
    for k in range(6):
        f = ts.frame(dx=k * 0.4 * ts.PIXEL_AT_SPHERE)
        clean = f["clean"].astype(np.float64)
        if k >= 4:
            clean[..., :3] = np.where((f["ids"][..., 0] == 1)[..., None], 0.3 * clean[..., :3], clean[..., :3])
        hit = f["ids"][..., 0] >= 0
        color = clean.copy()
        color[..., :3] += 0.1 * np.random.default_rng(100 + k).standard_normal((H, W, 3)) * hit[..., None]
        out.append(dict(f, color=color.astype(np.float32), clean=clean.astype(np.float32)))
    return out


def ghost(run):
    """-> (sphere ratio, ground ratio, share of the sphere's pixels with amount > 0) at frame 4: the mean absolute rgb error against the
    frame's clean image of the pass clamped with radius 1, gamma 1, no id stop, over that of the unclamped pass"""
    frames = ghost_frames()
    err = {}
    for name, clamp in (("plain", None), ("clamped", (1, 1.0, 0))):
        hist, prev = None, None
        for k in range(5):
            hist, _, amt = run(frames[k], prev, hist, False, None, clamp=clamp, **ts.PARAMS)
            prev = frames[k]
        f = frames[4]
        m = ts.inside()
        sphere, ground = m & (f["ids"][..., 0] == 1), m & (f["ids"][..., 0] == 0)
        d = np.abs(hist["color"][..., :3].astype(np.float64) - f["clean"][..., :3])
        err[name] = (float(d[sphere].mean()), float(d[ground].mean()), float((amt[sphere] > 0).mean()))
    noisy = float(np.abs(frames[4]["color"][..., :3].astype(np.float64) - frames[4]["clean"][..., :3])[sphere].mean())
    print("ghost, frame 4: sphere %.4f -> %.4f (noisy frame %.4f), ground %.4f -> %.4f, amount > 0 on %.3f of the sphere"
          % (err["plain"][0], err["clamped"][0], noisy, err["plain"][1], err["clamped"][1], err["clamped"][2]))
    return err["clamped"][0] / err["plain"][0], err["clamped"][1] / err["plain"][1], err["clamped"][2]


def check_untouched_and_unread(run, clamp=(2, GAMMA, 1)):
    """ts.check_untouched_and_unread with a clamped run -- garbage outside the region changes nothing inside: the skipped taps -- and an
    amount prefilled with -7.5 keeps that value outside the region"""
    amounts = []

    def clamped(cur, prev, prev_hist, albedo, vs, out=None, var_out=None, **params):
        amount = np.full((H, W), -7.5, dtype=np.float32)
        hist, var, amt = run(cur, prev, prev_hist, albedo, vs, out=out, var_out=var_out, clamp=clamp, amount=amount, **params)
        amounts.append(amt)
        return hist, var

    ts.check_untouched_and_unread(clamped)
    m = ts.inside()
    assert len(amounts) == 4
    for a in amounts:
        assert (a[~m] == np.float32(-7.5)).all() and (a[m] >= 0).all()
    assert np.array_equal(amounts[1], amounts[3]) and (amounts[1] > 0).sum() > 50
