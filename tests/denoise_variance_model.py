"""numpy restatement of fjgpu_denoise_estimate_variance and fjgpu_denoise_variance (include/fjgpu.h), f32 throughout.

Written from the header's text, not from the kernels.  l(C) = 0.2126f C.r + 0.7152f C.g + 0.0722f C.b.  Estimate: over the 7 x 7 taps
(dy outer, dx inner; outside the region or, with stop_at_ids, of another instance id: skipped) w = expf(-(d2n k_n + d2x k_x)); pass 1
s0 += w, s1 += w l_q, m = s1 / s0; pass 2 d = l_q - m, s2 += w (d d); V = max(s2 / s0, 0).  Iteration i, spacing 2^i: g = the 3 x 3
average of V at spacing 1 with weights (1/4, 1/2, 1/4)^2 over the taps inside the region, divided by their weight sum;
k_l = 1 / (sigma_luminance sqrtf(g) + 1e-6), 0 where sigma_luminance is <= 0 or +inf; e = |l_q - l_p| k_l + d2n k_n + d2x k_x;
w = (h[dy+2] h[dx+2]) expf(-e); sum += w C_q, wsum += w, vsum += (w w) V_q; C' = sum / wsum, V' = vsum / (wsum wsum).
Vectorised over the pixels, loops over the taps; skipping a tap is adding a +0 term.  Helpers and rel_err are denoise_model's.
"""
import numpy as np

import albedo_model as am
import denoise_model as dm
from denoise_model import rel_err          # noqa: F401  (the error measure of every comparison with this model)

VAR_EPS = np.float32(1e-6)
K3 = np.array([0.25, 0.5, 0.25], dtype=np.float32)
F = np.float32


def luminance(C):
    return (F(0.2126) * C[..., 0] + F(0.7152) * C[..., 1]) + F(0.0722) * C[..., 2]


def _views(h, w, oy, ox):
    """slices P (pixels whose tap at offset (ox, oy) is inside the h x w region) and Q (those taps), or None"""
    py0, py1 = max(0, -oy), min(h, h - oy)
    px0, px1 = max(0, -ox), min(w, w - ox)
    if py0 >= py1 or px0 >= px1:
        return None
    return (slice(py0, py1), slice(px0, px1)), (slice(py0 + oy, py1 + oy), slice(px0 + ox, px1 + ox))


def _crop(color, normal, position, ids, stop_at_ids, region):
    color = np.ascontiguousarray(color, dtype=np.float32)
    H, W = color.shape[:2]
    x0, y0, x1, y1 = (0, 0, W, H) if region is None else region
    h, w = y1 - y0, x1 - x0
    zero3 = np.zeros((h, w, 3), dtype=np.float32)
    N = zero3 if normal is None else np.ascontiguousarray(normal, dtype=np.float32)[y0:y1, x0:x1, :3]
    X = zero3 if position is None else np.ascontiguousarray(position, dtype=np.float32)[y0:y1, x0:x1, :3]
    I = None if (ids is None or not stop_at_ids) else np.asarray(ids)[y0:y1, x0:x1, 0]
    return color, (x0, y0, x1, y1), N, X, I


def _estimate(L, N, X, I, kn, kx):
    h, w = L.shape
    taps = []
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            v = _views(h, w, dy, dx)
            if v is None:
                continue
            P, Q = v
            wt = np.exp(-(dm._dist2(N[P], N[Q]) * kn + dm._dist2(X[P], X[Q]) * kx), dtype=np.float32)
            if I is not None:
                wt = np.where(I[Q] == I[P], wt, F(0))
            taps.append((P, Q, wt))
    s0 = np.zeros((h, w), dtype=np.float32)
    s1 = np.zeros((h, w), dtype=np.float32)
    for P, Q, wt in taps:
        s0[P] += wt
        s1[P] += wt * L[Q]
    m = s1 / s0
    s2 = np.zeros((h, w), dtype=np.float32)
    for P, Q, wt in taps:
        d = L[Q] - m[P]
        s2[P] += wt * (d * d)
    V = s2 / s0
    return np.where(V > 0, V, F(0)).astype(np.float32)


def estimate_variance(color, normal=None, position=None, ids=None, sigma_normal=1.0, sigma_position=1.0, stop_at_ids=True, region=None):
    """-> [H, W] f32: the estimate inside the region, 0 outside"""
    color, (x0, y0, x1, y1), N, X, I = _crop(color, normal, position, ids, stop_at_ids, region)
    _, kn, kx = dm.constants(0.0, sigma_normal if normal is not None else 0.0, sigma_position if position is not None else 0.0, 0)
    out = np.zeros(color.shape[:2], dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        out[y0:y1, x0:x1] = _estimate(luminance(color[y0:y1, x0:x1]), N, X, I, kn, kx)
    return out


def k_l(sigma_luminance, g):
    s = float(np.float32(sigma_luminance))
    if not s > 0 or s == float("inf"):
        return np.zeros_like(g)
    return (F(1) / (F(s) * np.sqrt(g, dtype=np.float32) + VAR_EPS)).astype(np.float32)


def denoise_variance(color, normal=None, position=None, ids=None, albedo=None, albedo_floor=1e-4, variance=None, iterations=5,
                     sigma_luminance=4.0, sigma_normal=1.0, sigma_position=1.0, stop_at_ids=True, region=None):
    """-> (a copy of color whose region is filtered, [H, W] f32 variance of the last iteration inside the region and 0 outside)"""
    color0 = np.ascontiguousarray(color, dtype=np.float32)
    a = None
    if albedo is not None:
        color, a = am.demodulate(color0, albedo, albedo_floor, region)
    color, (x0, y0, x1, y1), N, X, I = _crop(color, normal, position, ids, stop_at_ids, region)
    h, w = y1 - y0, x1 - x0
    _, kn, kx = dm.constants(0.0, sigma_normal if normal is not None else 0.0, sigma_position if position is not None else 0.0, 0)
    C = color[y0:y1, x0:x1].copy()
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        if variance is None:
            V = _estimate(luminance(C), N, X, I, kn, kx)
        else:
            V = np.ascontiguousarray(variance, dtype=np.float32)[y0:y1, x0:x1].copy()
        for i in range(iterations):
            s = 1 << i
            gs = np.zeros((h, w), dtype=np.float32)
            gw = np.zeros((h, w), dtype=np.float32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    v = _views(h, w, dy, dx)
                    if v is None:
                        continue
                    P, Q = v
                    wt = K3[dy + 1] * K3[dx + 1]
                    gs[P] += wt * V[Q]
                    gw[P] += wt
            kl = k_l(sigma_luminance, gs / gw)
            L = luminance(C)
            acc = np.zeros((h, w, 4), dtype=np.float32)
            wsum = np.zeros((h, w), dtype=np.float32)
            vsum = np.zeros((h, w), dtype=np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    v = _views(h, w, s * dy, s * dx)
                    if v is None:
                        continue
                    P, Q = v
                    e = (np.abs(L[Q] - L[P]) * kl[P] + dm._dist2(N[P], N[Q]) * kn) + dm._dist2(X[P], X[Q]) * kx
                    wt = (dm.H5[dy + 2] * dm.H5[dx + 2]) * np.exp(-e, dtype=np.float32)
                    if I is not None:
                        wt = np.where(I[Q] == I[P], wt, F(0))
                    acc[P] += wt[..., None] * C[Q]
                    wsum[P] += wt
                    vsum[P] += (wt * wt) * V[Q]
            C = acc / wsum[..., None]
            V = vsum / (wsum * wsum)
    out = color0.copy()
    out[y0:y1, x0:x1] = C
    if a is not None:
        out[y0:y1, x0:x1, :3] = C[..., :3] * a[y0:y1, x0:x1]
    var = np.zeros(color0.shape[:2], dtype=np.float32)
    var[y0:y1, x0:x1] = V
    return out, var
