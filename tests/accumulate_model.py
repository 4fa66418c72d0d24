"""numpy restatement of fjgpu_accumulate and fjgpu_accumulate_tile_error (include/fjgpu.h), f32 throughout.

Written from the header's text, not from the kernels.  State per pixel: mean [4], m2, count.  With `reset` the state read is zero.  A new
pixel with a channel that is not finite changes nothing (under reset the zero state is stored).  Otherwise n = count + 1;
mean_k' = mean_k + (x_k - mean_k) / n; l = l(x.rgb), m = l(mean.rgb) BEFORE the update, l(C) = 0.2126f C.r + 0.7152f C.g + 0.0722f C.b
left to right; d = l - m; m' = m + d / n; m2' = m2 + d * (l - m'); count' = n.  variance = count' >= 2 ? m2' / (count' * (count' - 1)) : 0.
Tile error: e_p = sqrtf(variance) / max(l(mean.rgb), lum_floor); the f64 sum over the rectangle (here: row by row, the serial sum) over
the pixel count, rounded to f32; +inf where a pixel has count < 2.

Every operation is a numpy f32 operation on whole arrays, so nothing is contracted and nothing is computed wider.
"""
import numpy as np

f32 = np.float32


def luminance(r, g, b):
    return f32(0.2126) * r + f32(0.7152) * g + f32(0.0722) * b


def new_state(yres, xres, fill=0.0):
    return dict(mean=np.full((yres, xres, 4), fill, f32), m2=np.full((yres, xres), fill, f32), count=np.full((yres, xres), fill, f32))


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def variance_of_mean(m2, count):
    with np.errstate(all="ignore"):
        v = m2 / (count * (count - f32(1)))
    return np.where(count >= f32(2), v, f32(0)).astype(f32)


def accumulate(color, state, rects=None, reset=False, variance_out=None):
    """fjgpu_accumulate on numpy arrays, in place: color [H, W, 4] f32, state = dict(mean [H, W, 4], m2 [H, W], count [H, W]), rects a list of
    (xmin, ymin, xmax, ymax) or None (the whole frame), variance_out [H, W] or None"""
    H, W = color.shape[:2]
    for x0, y0, x1, y1 in ([(0, 0, W, H)] if rects is None else rects):
        sl = (slice(y0, y1), slice(x0, x1))
        x = color[sl].astype(f32)
        if reset:
            mean, m2, count = np.zeros_like(x), np.zeros(x.shape[:2], f32), np.zeros(x.shape[:2], f32)
        else:
            mean, m2, count = state["mean"][sl].copy(), state["m2"][sl].copy(), state["count"][sl].copy()
        ok = np.isfinite(x).all(axis=2)
        with np.errstate(all="ignore"):
            n = count + f32(1)
            l = luminance(x[..., 0], x[..., 1], x[..., 2])
            m = luminance(mean[..., 0], mean[..., 1], mean[..., 2])
            mean_new = mean + (x - mean) / n[..., None]
            d = l - m
            m1 = m + d / n
            m2_new = m2 + d * (l - m1)
        mean = np.where(ok[..., None], mean_new, mean).astype(f32)
        m2 = np.where(ok, m2_new, m2).astype(f32)
        count = np.where(ok, n, count).astype(f32)
        write = ok | bool(reset)
        state["mean"][sl] = np.where(write[..., None], mean, state["mean"][sl])
        state["m2"][sl] = np.where(write, m2, state["m2"][sl])
        state["count"][sl] = np.where(write, count, state["count"][sl])
        if variance_out is not None:
            variance_out[sl] = variance_of_mean(m2, count)
    return state


def tile_errors(state, rects=None, lum_floor=1e-3):
    """fjgpu_accumulate_tile_error on numpy arrays -> f32 [n_rects]"""
    H, W = state["count"].shape
    out = []
    for x0, y0, x1, y1 in ([(0, 0, W, H)] if rects is None else rects):
        sl = (slice(y0, y1), slice(x0, x1))
        mean, m2, count = state["mean"][sl], state["m2"][sl], state["count"][sl]
        if not bool((count >= f32(2)).all()):
            out.append(f32(np.inf))
            continue
        with np.errstate(all="ignore"):
            v = variance_of_mean(m2, count)
            l = luminance(mean[..., 0], mean[..., 1], mean[..., 2])
            e = np.sqrt(v, dtype=f32) / np.where(l > f32(lum_floor), l, f32(lum_floor)).astype(f32)
        s = 0.0
        for val in e.astype(np.float64).reshape(-1):      # the serial f64 sum, row by row
            s += float(val)
        out.append(f32(s / float(e.size)))
    return np.array(out, f32)
