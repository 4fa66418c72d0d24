"""An analytic scene for the temporal accumulation's tests (tests/test_temporal_cpu.py, tests/test_gpu_temporal.py): a square of ground and
a sphere standing on it, seen by a pinhole camera with the conventions of include/fjgpu.h (fjgpu_scene_view): rays through pixel centres,
u = (x + .5) / W, v = 1 - (y + .5) / H, target ((u - .5) uv_x, (v - .5) uv_y, -1) in camera space.  Position, normal and ids are exact
(f64, rounded to f32 once); the colour is a smooth function of the world position, so that the same surface point has the same colour from
every camera, plus -- where asked for -- per-frame noise from a seeded generator.

W x H = 37 x 29 with region (3, 2, 34, 27): odd, ragged, and more than one 16 x 16 block of the kernel in both directions.
"""
import numpy as np

import temporal_model as tm

W, H = 37, 29
REGION = (3, 2, 34, 27)
SPHERE_C = np.array([0.3, 1.0, -6.0])
SPHERE_R = 1.0
GROUND_HALF = 6.0                      # the ground is the rectangle |x| <= 6, -12 <= z <= 4 of the plane y = 0; beyond it: background
FOV_Y = 40.0
EYE = np.array([0.0, 2.2, 1.5])
TILT = -0.22                           # radians about x: the camera looks slightly down
# a sideways move of the camera that shifts the sphere's centre by one pixel: distance / focal length in pixels
PIXEL_AT_SPHERE = float(np.linalg.norm(SPHERE_C - EYE) * 2 * np.tan(np.radians(FOV_Y) / 2) / H)


def camera(dx=0.0, pan=0.0, tilt=TILT):
    """(camera-to-world 4 x 4, view): the eye moved sideways by dx world units and turned by `pan` radians about y"""
    cy, sy, cx, sx = np.cos(pan), np.sin(pan), np.cos(tilt), np.sin(tilt)
    Ry = np.array([[cy, 0, sy, 0], [0, 1, 0, 0], [-sy, 0, cy, 0], [0, 0, 0, 1.0]])
    Rx = np.array([[1, 0, 0, 0], [0, cx, -sx, 0], [0, sx, cx, 0], [0, 0, 0, 1.0]])
    T = np.eye(4)
    T[:3, 3] = EYE + np.array([dx, 0.0, 0.0])
    M = T @ Ry @ Rx
    uvy = 2 * np.tan(np.radians(FOV_Y) / 2)
    return M, tm.View(np.linalg.inv(M)[:3].reshape(-1), (uvy * W / H, uvy), W, H)


def rays(M, view, u=None, v=None):
    """origin [3] and unit directions [..., 3] of the rays through (u, v) (default: the pixel centres), as Camera::GetRay forms them"""
    if u is None:
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        u, v = (x + .5) / W, 1 - (y + .5) / H
    target = np.stack([(u - .5) * view.uv_size[0], (v - .5) * view.uv_size[1], -np.ones_like(u), np.ones_like(u)], axis=-1)
    tw = target @ M.T
    eye = M[:3, 3]
    d = tw[..., :3] - eye
    return eye, d / np.linalg.norm(d, axis=-1, keepdims=True)


def world_colour(P):
    """the noise-free RGBA of a surface point: smooth in the world position, between 0.2 and 1.4"""
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    c = np.stack([0.8 + 0.5 * np.sin(0.9 * x + 0.4 * z), 0.7 + 0.4 * np.cos(0.6 * z - 0.5 * y), 0.8 + 0.3 * np.sin(0.7 * x * 0.5 + 1.1 * y),
                  np.ones_like(x)], axis=-1)
    return c


def world_albedo(P):
    x, z = P[..., 0], P[..., 2]
    return np.stack([0.5 + 0.3 * np.sin(1.7 * x), 0.5 + 0.3 * np.cos(1.3 * z), 0.4 + 0.2 * np.sin(x + z)], axis=-1)


def frame(dx=0.0, pan=0.0, noise=0.0, seed=0, tilt=TILT, sphere=True):
    """one frame -> dict(view, color [H, W, 4], position, normal [H, W, 3], ids [H, W, 4] int32, albedo [H, W, 3], clean [H, W, 4]): ids[0] is 0 on
    the ground, 1 on the sphere, -1 on the background (position and normal 0, colour 0 there, as the AOV pass leaves a pixel without a hit).
    sphere=False with tilt=-0.9: nothing but ground in every pixel."""
    M, view = camera(dx, pan, tilt)
    eye, d = rays(M, view)
    # sphere
    oc = eye - SPHERE_C
    b = d @ oc
    disc = b * b - (oc @ oc - SPHERE_R ** 2)
    with np.errstate(all="ignore"):
        ts = np.where((disc > 0) & sphere, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
        ts = np.where(ts > 0, ts, np.inf)
        tg = np.where(d[..., 1] < 0, -eye[1] / d[..., 1], np.inf)
    Pg = eye + np.where(np.isfinite(tg), tg, 0.0)[..., None] * d
    tg = np.where(np.isfinite(tg) & (np.abs(Pg[..., 0]) <= GROUND_HALF) & (Pg[..., 2] >= -2 * GROUND_HALF) & (Pg[..., 2] <= 4.0), tg, np.inf)
    t = np.minimum(ts, tg)
    hit = np.isfinite(t)
    P = eye + np.where(hit, t, 0)[..., None] * d
    on_sphere = hit & (ts <= tg)
    N = np.where(on_sphere[..., None], (P - SPHERE_C) / SPHERE_R, np.array([0.0, 1.0, 0.0]))
    ids = np.full((H, W, 4), -1, dtype=np.int32)
    ids[..., 0] = np.where(hit, np.where(on_sphere, 1, 0), -1)
    ids[..., 1] = np.where(hit, 7, -1)
    clean = np.where(hit[..., None], world_colour(P), 0.0)
    color = clean.copy()
    if noise:
        color[..., :3] += noise * np.random.default_rng(seed).standard_normal((H, W, 3)) * hit[..., None]
    return dict(view=view, M=M, color=color.astype(np.float32), clean=clean.astype(np.float32),
                position=np.where(hit[..., None], P, 0.0).astype(np.float32), normal=np.where(hit[..., None], N, 0.0).astype(np.float32),
                ids=ids, albedo=np.where(hit[..., None], world_albedo(P), 0.0).astype(np.float32))


def inside():
    m = np.zeros((H, W), dtype=bool)
    m[REGION[1]:REGION[3], REGION[0]:REGION[2]] = True
    return m


# ---- the cases both suites run: `run(cur, prev, prev_hist, albedo, vs, out, var_out, **params) -> (history, variance)` is the host twin
# (tests/test_temporal_cpu.py) or the device (tests/test_gpu_temporal.py); cur / prev are frames as above, prev_hist a history or None
PARAMS = dict(alpha_min=0.05, max_history=8.0, tol_position=0.5, cos_normal=0.8, min_history_variance=3.0, albedo_floor=0.05)
REL_TOL = 1e-4


def model_run(cur, prev, prev_hist, albedo, vs, out=None, var_out=None, **params):
    return tm.accumulate(cur["color"], cur["position"], cur["normal"], cur["ids"], albedo=cur["albedo"] if albedo else None, variance_spatial=vs,
                         prev_view=prev["view"] if prev else None, prev_position=prev["position"] if prev else None,
                         prev_normal=prev["normal"] if prev else None, prev_ids=prev["ids"] if prev else None, prev=prev_hist, region=REGION,
                         out=out, variance_out=var_out, **params)


def pan_sequence(n=4, step=0.4, noise=0.1):
    """n frames of a sideways move of `step` pixels (at the sphere's distance) per frame, each with its own noise"""
    return [frame(dx=k * step * PIXEL_AT_SPHERE, noise=noise, seed=100 + k) for k in range(n)]


def spatial_variance(k):
    return (np.random.default_rng(40 + k).random((H, W)) * 0.2).astype(np.float32)


def check_equal_to_model(run, albedo, spatial, what, frames=None):
    """a 4-frame pan through `run`, each frame from run's own history of the frame before, against the model on the same inputs: every
    output within REL_TOL (denominator floored at 1e-3), the history length exactly (the taps both chose are the same)"""
    frames = pan_sequence() if frames is None else frames
    hist, prev = None, None
    for k, cur in enumerate(frames):
        vs = spatial_variance(k) if spatial else None
        got, gvar = run(cur, prev, hist, albedo, vs, **PARAMS)
        ref, rvar = model_run(cur, prev, hist, albedo, vs, **PARAMS)
        assert np.array_equal(got["length"], ref["length"]), (what, k)
        for name, a, b in (("color", got["color"], ref["color"]), ("moments", got["moments"], ref["moments"]), ("variance", gvar, rvar)):
            assert np.isfinite(a).all()
            err = float(tm.rel_err(a, b).max())
            print("temporal %-28s frame %d %-8s max rel err %.3e" % (what, k, name, err))
            assert err <= REL_TOL, (what, k, name, err)
        hist, prev = got, cur
    m = inside()
    fg = m & (frames[-1]["ids"][..., 0] >= 0)
    # (a weighted mean of equal lengths is that length up to an f32 rounding per tap)
    assert abs(float(hist["length"][fg].max()) - len(frames)) <= 1e-5 and (hist["length"][m & ~fg] == 1).all()
    assert (hist["length"][fg] >= 2).mean() > 0.8
    return hist


def check_untouched_and_unread(run):
    """pixels outside the region are untouched in every output, and nothing outside it is read: garbage there changes nothing inside"""
    f0, f1 = pan_sequence(2)
    m = inside()

    def go(a, b):
        h0, _ = run(a, None, None, True, None, **PARAMS)
        out = tm.new_history(H, W, -7.5)
        var = np.full((H, W), -7.5, dtype=np.float32)
        return run(b, a, h0, True, spatial_variance(1), out=out, var_out=var, **PARAMS)

    hist, var = go(f0, f1)
    for a in (hist["color"], hist["moments"], hist["length"], var):
        assert (a[~m] == np.float32(-7.5)).all() and (a[m] != np.float32(-7.5)).all()
    g0, g1 = ({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()} for f in (f0, f1))
    for f in (g0, g1):
        for k in ("color", "position", "normal", "albedo"):
            f[k][~m] = np.float32(1e30)
        f["ids"][~m] = 0                   # the ground's id: a tap out there would be taken if it were read
    hist2, var2 = go(g0, g1)
    for k in hist:
        assert np.array_equal(hist[k], hist2[k])
    assert np.array_equal(var, var2)
