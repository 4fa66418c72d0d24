"""numpy restatement of fjgpu_denoise_temporal_clamped (include/fjgpu.h), f32 throughout, the projection in f64.

Written from the header's text, not from the kernel.  The pass is fjgpu_denoise_temporal's (tests/temporal_model.py, which has no hook
between fetch and blend, so the whole pass is restated here) up to and including H /= valid weight.  Then, for a pixel p with history and
a clamp (radius, gamma, stop_at_ids): the taps q = p + (dx, dy), dy = -radius..radius outer, dx inner, of the CURRENT frame count where they
lie in the region and (stop_at_ids) ids[q][0] == ids[p][0]; cnt = sum of 1.f; for X in the four channels of C_q and L_q (the pass's luminance
of pixel q): s1 += X_q, m = s1 / cnt, then d = X_q - m, s2 += d d, sd = sqrt(s2 / cnt), lo = m - gamma sd, hi = m + gamma sd.
H' = H < lo ? lo : (H > hi ? hi : H) for the colour, h1 likewise against L's box, h2' = h2 where h1' == h1 else (h2 - h1 h1) + h1' h1'.
amount = max |H' - H| over r, g, b; 0 without history.  Blend and variance from H'.  Skipping a tap is adding a +0 term.
"""
import numpy as np

from denoise_variance_model import luminance
from temporal_model import _dist2, new_history, project, rel_err          # noqa: F401

F = np.float32
MIN_WEIGHT = np.float32(1e-4)


def window_box(X, ids0, region, radius, gamma, stop_at_ids):
    """X [h, w, 5] and ids0 [h, w] of the region -> (m, sd, lo, hi), each [h, w, 5]: the box of every region pixel's window"""
    h, w = ids0.shape
    r = int(radius)
    Xp = np.zeros((h + 2 * r, w + 2 * r, 5), dtype=np.float32)
    Xp[r:r + h, r:r + w] = X
    Ip = np.zeros((h + 2 * r, w + 2 * r), dtype=ids0.dtype)
    Ip[r:r + h, r:r + w] = ids0
    inside = np.zeros((h + 2 * r, w + 2 * r), dtype=bool)
    inside[r:r + h, r:r + w] = True
    taps = []
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sl = (slice(r + dy, r + dy + h), slice(r + dx, r + dx + w))
            counts = inside[sl].copy()
            if stop_at_ids:
                counts &= Ip[sl] == ids0
            taps.append((counts, Xp[sl]))
    with np.errstate(all="ignore"):
        cnt = np.zeros((h, w), dtype=np.float32)
        s1 = np.zeros((h, w, 5), dtype=np.float32)
        for counts, Xq in taps:
            cnt = cnt + np.where(counts, F(1), F(0))
            s1 = s1 + np.where(counts[..., None], Xq, F(0))
        m = s1 / cnt[..., None]
        s2 = np.zeros((h, w, 5), dtype=np.float32)
        for counts, Xq in taps:
            d = Xq - m
            s2 = s2 + np.where(counts[..., None], d * d, F(0))
        sd = np.sqrt(s2 / cnt[..., None])
        lo = m - F(gamma) * sd
        hi = m + F(gamma) * sd
    return m, sd, lo, hi


def _clip(H, lo, hi):
    return np.where(H < lo, lo, np.where(H > hi, hi, H))


def accumulate(color, position, normal, ids, albedo=None, variance_spatial=None, prev_view=None, prev_position=None, prev_normal=None,
               prev_ids=None, prev=None, region=None, alpha_min=0.1, max_history=32.0, tol_position=None, cos_normal=0.9,
               min_history_variance=4.0, albedo_floor=1e-4, out=None, variance_out=None, clamp=None, amount_out=None, details=None):
    """-> (history {"color", "moments", "length"}, variance [H, W], amount [H, W]).  clamp: None or (radius, gamma, stop_at_ids).
    details: a dict that receives "m", "sd" [h, w, 5] of the region's boxes and "have" [h, w]"""
    C = np.ascontiguousarray(color, dtype=np.float32)
    Hh, Ww = C.shape[:2]
    x0, y0, x1, y1 = (0, 0, Ww, Hh) if region is None else region
    R = (slice(y0, y1), slice(x0, x1))
    out = new_history(Hh, Ww) if out is None else out
    variance_out = np.zeros((Hh, Ww), dtype=np.float32) if variance_out is None else variance_out
    amount_out = np.zeros((Hh, Ww), dtype=np.float32) if amount_out is None else amount_out
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
        Hm = (hsum / np.where(have, wsum, F(1))[..., None]).astype(np.float32)
        amount = np.zeros((h, w), dtype=np.float32)
        if clamp is not None:
            radius, gamma, stop = clamp
            X5 = np.concatenate([c, L[..., None]], axis=-1)
            m, sd, lo, hi = window_box(X5, I, None, radius, gamma, stop)
            if details is not None:
                details.update(m=m, sd=sd, have=have)
            Hc = _clip(Hm[..., :4], lo[..., :4], hi[..., :4])
            h1, h2 = Hm[..., 4], Hm[..., 5]
            h1c = _clip(h1, lo[..., 4], hi[..., 4])
            h2c = np.where(h1c == h1, h2, (h2 - h1 * h1) + h1c * h1c)
            amount = np.where(have, np.abs(Hc[..., :3] - Hm[..., :3]).max(axis=-1), F(0)).astype(np.float32)
            Hm = np.concatenate([Hc, h1c[..., None], h2c[..., None], Hm[..., 6:]], axis=-1).astype(np.float32)
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
    amount_out[R] = amount
    return out, variance_out, amount_out
