"""numpy restatement of fjgpu_denoise_temporal (include/fjgpu.h), f32 throughout, the projection in f64.

Written from the header's text, not from the kernel.  Projection of a world point P through a view (world_to_camera M, rows of a 3 x 4
matrix; uv_size; xres, yres): c_k = ((M[4k] P.x + M[4k+1] P.y) + M[4k+2] P.z) + M[4k+3], visible if c.z < 0,
fx = (c.x / -c.z / uv_size[0] + .5) xres - .5, fy = (.5 - c.y / -c.z / uv_size[1]) yres - .5.  Per region pixel: L = l(C.rgb / max(albedo,
floor)) or l(C.rgb); the four taps around (fx, fy), j outer and i inner, weigh (i ? a : 1 - a) (j ? b : 1 - b) and count where they lie in
the region, carry the pixel's id, pass the position and normal tests and have a history length >= 1; H = weighted sums / valid weight;
n = min(H_len + 1, max_history), alpha = max(1 / n, alpha_min), X' = H + alpha (X - H); no history (valid weight <= 1e-4, background,
non-finite position or projection, no previous frame): C' = C, m = (L, L L), len = 1.  v = max(0, m2' - m1' m1'), or the spatial variance
where len' < min_history_variance.  Vectorised over the pixels, a loop over the four taps; skipping a tap is adding a +0 term.
"""
import numpy as np

from denoise_model import _dist2, rel_err          # noqa: F401  (rel_err: the error measure of every comparison with this model)
from denoise_variance_model import luminance

F = np.float32
MIN_WEIGHT = np.float32(1e-4)


class View(object):
    """fjgpu_view as plain Python: anything with these four attributes is a view to this module (ffi.View is)"""

    def __init__(self, world_to_camera, uv_size, xres, yres):
        self.world_to_camera = [float(v) for v in np.asarray(world_to_camera, dtype=np.float64).reshape(-1)[:12]]
        self.uv_size = [float(uv_size[0]), float(uv_size[1])]
        self.xres, self.yres = int(xres), int(yres)


def project(view, P):
    """P [..., 3] (f32 or f64) -> (fx, fy, ok): f64 pixel coordinates and whether the point is in front of the camera and both are finite"""
    M = [float(v) for v in view.world_to_camera]
    P = np.asarray(P)
    X, Y, Z = (P[..., k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        c = [((M[4 * k] * X + M[4 * k + 1] * Y) + M[4 * k + 2] * Z) + M[4 * k + 3] for k in range(3)]
        d = -c[2]
        fx = (c[0] / d / float(view.uv_size[0]) + .5) * float(view.xres) - .5
        fy = (.5 - c[1] / d / float(view.uv_size[1])) * float(view.yres) - .5
        ok = (c[2] < 0) & np.isfinite(fx) & np.isfinite(fy)
    return fx, fy, ok


def new_history(H, W, fill=0.0):
    return {"color": np.full((H, W, 4), fill, dtype=np.float32), "moments": np.full((H, W, 2), fill, dtype=np.float32),
            "length": np.full((H, W), fill, dtype=np.float32)}


def accumulate(color, position, normal, ids, albedo=None, variance_spatial=None, prev_view=None, prev_position=None, prev_normal=None,
               prev_ids=None, prev=None, region=None, alpha_min=0.1, max_history=32.0, tol_position=None, cos_normal=0.9,
               min_history_variance=4.0, albedo_floor=1e-4, out=None, variance_out=None):
    """-> (history {"color", "moments", "length"}, variance [H, W]): `out` / `variance_out` (or new zeroed arrays) with the region written"""
    C = np.ascontiguousarray(color, dtype=np.float32)
    Hh, Ww = C.shape[:2]
    x0, y0, x1, y1 = (0, 0, Ww, Hh) if region is None else region
    R = (slice(y0, y1), slice(x0, x1))
    out = new_history(Hh, Ww) if out is None else out
    variance_out = np.zeros((Hh, Ww), dtype=np.float32) if variance_out is None else variance_out
    c = C[R]
    with np.errstate(all="ignore"):
        if albedo is not None:
            a = np.ascontiguousarray(albedo, dtype=np.float32)[R]
            a = np.where(a > F(albedo_floor), a, F(albedo_floor))
            L = luminance(c[..., :3] / a)
        else:
            L = luminance(c[..., :3])
        L2 = L * L
        P = np.ascontiguousarray(position, dtype=np.float32)[R]
        N = np.ascontiguousarray(normal, dtype=np.float32)[R]
        I = np.asarray(ids)[R][..., 0]
        h, w = L.shape
        wsum = np.zeros((h, w), dtype=np.float32)
        hsum = np.zeros((h, w, 7), dtype=np.float32)
        if prev is not None:
            fx, fy, ok = project(prev_view, P)
            ok = ok & (I >= 0) & np.isfinite(P).all(axis=-1)
            fx = np.where(ok, fx, 0.0)
            fy = np.where(ok, fy, 0.0)
            xf, yf = np.floor(fx), np.floor(fy)
            ok = ok & (xf >= x0 - 1) & (xf < x1) & (yf >= y0 - 1) & (yf < y1)
            xf = np.where(ok, xf, 0.0)
            yf = np.where(ok, yf, 0.0)
            ta, tb = (fx - xf).astype(np.float32), (fy - yf).astype(np.float32)
            qx0, qy0 = xf.astype(np.int64), yf.astype(np.int64)
            pP = np.ascontiguousarray(prev_position, dtype=np.float32)
            pN = np.ascontiguousarray(prev_normal, dtype=np.float32)
            pI = np.asarray(prev_ids)[..., 0]
            hist = np.concatenate([np.ascontiguousarray(prev["color"], dtype=np.float32), np.ascontiguousarray(prev["moments"], dtype=np.float32),
                                   np.ascontiguousarray(prev["length"], dtype=np.float32)[..., None]], axis=-1)
            tol = float(np.float32(0.0 if tol_position is None else tol_position))
            position_on = tol > 0 and tol != float("inf")
            tol2 = F(tol) * F(tol)
            normal_on = float(np.float32(cos_normal)) > -1
            for j in range(2):
                for i in range(2):
                    qx, qy = qx0 + i, qy0 + j
                    valid = ok & (qx >= x0) & (qx < x1) & (qy >= y0) & (qy < y1)
                    gx, gy = np.where(valid, qx, x0), np.where(valid, qy, y0)
                    valid &= pI[gy, gx] == I
                    if position_on:
                        valid &= _dist2(P, pP[gy, gx]) <= tol2
                    if normal_on:
                        q = pN[gy, gx]
                        valid &= (q[..., 0] * N[..., 0] + q[..., 1] * N[..., 1]) + q[..., 2] * N[..., 2] >= F(cos_normal)
                    Hq = hist[gy, gx]
                    valid &= Hq[..., 6] >= F(1)
                    wt = (ta if i else F(1) - ta) * (tb if j else F(1) - tb)
                    wsum = wsum + np.where(valid, wt, F(0))
                    hsum = hsum + np.where(valid[..., None], wt[..., None] * Hq, F(0))
        have = wsum > MIN_WEIGHT
        Hm = hsum / np.where(have, wsum, F(1))[..., None]
        n1 = Hm[..., 6] + F(1)
        n = np.where(n1 < F(max_history), n1, F(max_history))
        r = F(1) / n
        alpha = np.where(r > F(alpha_min), r, F(alpha_min))
        X = np.concatenate([c, L[..., None], L2[..., None]], axis=-1)
        blended = Hm[..., :6] + alpha[..., None] * (X - Hm[..., :6])
        Xn = np.where(have[..., None], blended, X).astype(np.float32)
        n = np.where(have, n, F(1)).astype(np.float32)
        v = Xn[..., 5] - Xn[..., 4] * Xn[..., 4]
        v = np.where(v > 0, v, F(0))
        if variance_spatial is not None:
            v = np.where(n < F(min_history_variance), np.ascontiguousarray(variance_spatial, dtype=np.float32)[R], v)
    out["color"][R] = Xn[..., :4]
    out["moments"][R] = Xn[..., 4:6]
    out["length"][R] = n
    variance_out[R] = v.astype(np.float32)
    return out, variance_out
