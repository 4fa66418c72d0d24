"""numpy restatement of fjgpu_denoise (include/fjgpu.h): the edge-avoiding a-trous filter, f32 throughout.

Written from the header's text, not from the kernel: h = (1/16, 1/4, 3/8, 1/4, 1/16); iteration i has tap spacing 2^i; the taps are
visited dy = -2..2 (outer), dx = -2..2 (inner); a tap outside the region, or (stop_at_ids) of another instance id, is skipped;
w = (h[dy+2] h[dx+2]) expf(-(d2c k_c + d2n k_n + d2x k_x)), every sum left to right in f32; out = sum / wsum.  The constants are f64
quotients rounded once to f32 (capped at the largest finite f32), 0 for a term that is off (sigma <= 0 or +inf, or its guide missing).
Vectorised over the pixels, a loop over the 25 taps.
"""
import numpy as np

H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=np.float32)
FLT_MAX = float(np.finfo(np.float32).max)


def k_of(sigma):
    """1 / sigma^2 as f32 (sigma: a python float holding the descriptor's f32 value, possibly scaled by 2^-i, which is exact)"""
    sigma = float(sigma)
    if not sigma > 0 or sigma == float("inf"):
        return np.float32(0)
    with np.errstate(over="ignore", divide="ignore"):
        k = np.float64(1.0) / (np.float64(sigma) * np.float64(sigma))
    return np.float32(min(float(k), FLT_MAX))


def constants(sigma_color, sigma_normal, sigma_position, i):
    sc, sn, sx = (float(np.float32(s)) for s in (sigma_color, sigma_normal, sigma_position))
    return k_of(sc * 2.0 ** -i), k_of(sn), k_of(sx)


def _dist2(a, b):
    d = b - a                                                        # f32 arrays [..., 3]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def denoise(color, normal=None, position=None, ids=None, iterations=5, sigma_color=1.0, sigma_normal=1.0, sigma_position=1.0,
            stop_at_ids=True, region=None):
    """color [H, W, 4] f32, normal / position [H, W, 3] f32 or None, ids [H, W, 4] int32 or None -> a copy of color whose region
    (xmin, ymin, xmax, ymax; None = the frame) is filtered"""
    color = np.ascontiguousarray(color, dtype=np.float32)
    H, W = color.shape[:2]
    x0, y0, x1, y1 = (0, 0, W, H) if region is None else region
    h, w = y1 - y0, x1 - x0
    C = color[y0:y1, x0:x1].copy()
    zero3 = np.zeros((h, w, 3), dtype=np.float32)
    N = zero3 if normal is None else np.ascontiguousarray(normal, dtype=np.float32)[y0:y1, x0:x1, :3]
    X = zero3 if position is None else np.ascontiguousarray(position, dtype=np.float32)[y0:y1, x0:x1, :3]
    I = None if (ids is None or not stop_at_ids) else np.asarray(ids)[y0:y1, x0:x1, 0]
    with np.errstate(over="ignore", under="ignore"):
        for i in range(iterations):
            s = 1 << i
            kc, kn, kx = constants(sigma_color, sigma_normal if normal is not None else 0.0,
                                   sigma_position if position is not None else 0.0, i)
            acc = np.zeros((h, w, 4), dtype=np.float32)
            wsum = np.zeros((h, w), dtype=np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    # pixels p = (py, px) whose tap q = p + s (dx, dy) is inside the region
                    py0, py1 = max(0, -s * dy), min(h, h - s * dy)
                    px0, px1 = max(0, -s * dx), min(w, w - s * dx)
                    if py0 >= py1 or px0 >= px1:
                        continue
                    P = (slice(py0, py1), slice(px0, px1))
                    Q = (slice(py0 + s * dy, py1 + s * dy), slice(px0 + s * dx, px1 + s * dx))
                    e = (_dist2(C[P][..., :3], C[Q][..., :3]) * kc + _dist2(N[P], N[Q]) * kn) + _dist2(X[P], X[Q]) * kx
                    wt = (H5[dy + 2] * H5[dx + 2]) * np.exp(-e, dtype=np.float32)
                    if I is not None:
                        wt = np.where(I[Q] == I[P], wt, np.float32(0))    # adding +0 terms is what skipping the tap does
                    acc[P] += wt[..., None] * C[Q]
                    wsum[P] += wt
            C = acc / wsum[..., None]
    out = color.copy()
    out[y0:y1, x0:x1] = C
    return out


def rel_err(a, ref):
    """the project's pixel error (tests/test_gpu_parity.py): the denominator floored at 1e-3"""
    return np.abs(a - ref) / np.maximum(np.abs(ref), 1e-3)
