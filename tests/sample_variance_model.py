"""numpy restatement of fjgpu_render_tiles_variance's arithmetic (include/fjgpu.h; csrc/device/fjgpu_sample_var_math.h), f64 sums.

Written from the header's text.  For pixel p = (px, py) and the npx_x * npx_y samples s of its filter window, each with its film position
(u, v) and its radiance:
  w_s = exp(-2 (xx xx + yy yy)),  xx = 2 (xres u - (px + .5)) / fw,  yy = 2 (yres (1 - v) - (py + .5)) / fh          (f64)
  l_s = (f64) l(d) with l(d) = 0.2126f d.r + 0.7152f d.g + 0.0722f d.b in f32; d = the sample's rgb, or rgb / max(albedo[p], albedo_floor)
        per channel in f32 -- the pixel's albedo
  S0 = sum w, S1 = sum w l, m = S1 / S0;  then S2 = sum w (l - m)^2, Q = sum w^2;  e = Q / S0^2;  V = (S2 / S0) e / (1 - e), 0 where e >= 1;
  rounded to f32 once; negative or not finite -> 0.
The sums here are numpy's (pairwise), the twin's are row-major and the kernel's a butterfly: they differ by f64 roundings.
"""
import math

import numpy as np

import denoise_variance_model as dvm

F = np.float32


def weight(xres, yres, fw, fh, px, py, u, v):
    """px, py, u, v broadcast against each other -> f64"""
    filtx = xres * np.asarray(u, dtype=np.float64) - (np.asarray(px) + .5)
    filty = yres * (1 - np.asarray(v, dtype=np.float64)) - (np.asarray(py) + .5)
    xx = 2 * filtx / float(fw)
    yy = 2 * filty / float(fh)
    return np.exp(-2 * (xx * xx + yy * yy))


def luminance(rgb, albedo=None, albedo_floor=1e-4):
    """rgb [..., 3] f32 and the PIXEL's albedo (broadcast against it) -> f64 of the f32 luminance"""
    d = np.asarray(rgb, dtype=np.float32)[..., :3]
    with np.errstate(all="ignore"):
        if albedo is not None:
            a = np.asarray(albedo, dtype=np.float32)
            d = (d / np.where(a > F(albedo_floor), a, F(albedo_floor))).astype(np.float32)
        return dvm.luminance(d).astype(np.float64)


def variance(w, l):
    """w, l [..., n] f64: the samples of a window along the last axis -> V [...] f32"""
    w = np.asarray(w, dtype=np.float64)
    l = np.asarray(l, dtype=np.float64)
    with np.errstate(all="ignore"):
        S0 = w.sum(axis=-1)
        m = (w * l).sum(axis=-1) / S0
        d = l - m[..., None]
        S2 = (w * (d * d)).sum(axis=-1)
        Q = (w * w).sum(axis=-1)
        e = Q / (S0 * S0)
        V = ((S2 / S0) * e / (1 - e)).astype(np.float32)
        V = np.where(e >= 1, F(0), V)
        return np.where(np.isfinite(V) & (V >= 0), V, F(0)).astype(np.float32)


def mean_and_e(w, l):
    """-> (m, e) of a window, f64: what a tolerance on V is floored with (V's scale is m^2 e where the spread is of the mean's size)"""
    w = np.asarray(w, dtype=np.float64)
    S0 = w.sum(axis=-1)
    return (w * np.asarray(l, dtype=np.float64)).sum(axis=-1) / S0, (w * w).sum(axis=-1) / (S0 * S0)


def tiles_variance(frame, tiles, s_uv, s_accum, albedo=None, albedo_floor=1e-4, out=None, moments=None):
    """the pass over sample arrays as the beauty pass holds them: frame = dict(xres, yres, rate_x, rate_y, npx_x, npx_y, fw, fh); tiles =
    dicts of xmin, ymin, xmax, ymax, nx, sample_offset; s_uv [n, 2] f64, s_accum [n, 4] f32; albedo [yres, xres, 3] or None
    -> [yres, xres] f32 (out's pixels outside the tiles are kept); moments: a [yres, xres, 2] f64 array that takes (m, e) of every pixel"""
    fr = frame
    V = np.zeros((fr["yres"], fr["xres"]), dtype=np.float32) if out is None else out
    sy, sx = np.mgrid[0:fr["npx_y"], 0:fr["npx_x"]]
    for T in tiles:
        for py in range(T["ymin"], T["ymax"]):
            for px in range(T["xmin"], T["xmax"]):
                base = T["sample_offset"] + (py - T["ymin"]) * fr["rate_y"] * T["nx"] + (px - T["xmin"]) * fr["rate_x"]
                s = (base + sy * T["nx"] + sx).reshape(-1)
                w = weight(fr["xres"], fr["yres"], fr["fw"], fr["fh"], px, py, s_uv[s, 0], s_uv[s, 1])
                l = luminance(s_accum[s], None if albedo is None else albedo[py, px], albedo_floor)
                V[py, px] = variance(w, l)
                if moments is not None:
                    with np.errstate(all="ignore"):
                        moments[py, px] = mean_and_e(w, l)
    return V


def sampler_margin(rate, filter_width):
    """FixedGridSampler's margin in samples per side"""
    return int(math.ceil((float(F(filter_width)) - 1) * rate * .5))


def from_fine_frame(fine, res, rate, filt, albedo=None, albedo_floor=1e-4):
    """The coarse frame's windows cut out of a FINE frame: `fine` [yres ry, xres rx, 4] f32 is the frame at rate times the resolution,
    1 x 1 sample per pixel, filter width 1, no jitter -- fine pixel (X, Y) is the radiance of the coarse frame's unjittered sample (X, Y),
    whose film position is u = (X + .5) / (rx xres), v = 1 - (Y + .5) / (ry yres).  res = (xres, yres), rate = (rx, ry), filt = (fw, fh).
    -> (V [yres, xres] f32, beauty [yres, xres, 4] f32 -- the filter's weighted mean of the window, f64 sums rounded once --,
        inside [yres, xres] bool: the pixels whose whole window lies in the fine frame; V and beauty are 0 elsewhere)"""
    (xres, yres), (rx, ry), (fw, fh) = res, rate, filt
    fine = np.asarray(fine, dtype=np.float32)
    assert fine.shape[:2] == (yres * ry, xres * rx), fine.shape
    mx, my = sampler_margin(rx, fw), sampler_margin(ry, fh)
    nx, ny = rx + 2 * mx, ry + 2 * my
    bx, by = -(-mx // rx), -(-my // ry)                 # ceil(margin / rate): pixels from the border
    V = np.zeros((yres, xres), dtype=np.float32)
    beauty = np.zeros((yres, xres, 4), dtype=np.float32)
    inside = np.zeros((yres, xres), dtype=bool)
    inside[by:yres - by, bx:xres - bx] = True
    py, px = np.nonzero(inside)
    sy, sx = np.mgrid[0:ny, 0:nx]
    Y = (py[:, None] * ry - my) + sy.reshape(-1)[None, :]          # [pixels, window]
    X = (px[:, None] * rx - mx) + sx.reshape(-1)[None, :]
    u = (X + .5) * (1. / (rx * xres))
    v = 1 - (Y + .5) * (1. / (ry * yres))
    w = weight(xres, yres, float(F(fw)), float(F(fh)), px[:, None], py[:, None], u, v)
    d = fine[Y, X]                                                  # [pixels, window, 4]
    a = None if albedo is None else np.asarray(albedo, dtype=np.float32)[py, px][:, None, :]
    V[py, px] = variance(w, luminance(d, a, albedo_floor))
    beauty[py, px] = ((w[..., None] * d.astype(np.float64)).sum(axis=1) / w.sum(axis=1)[:, None]).astype(np.float32)
    return V, beauty, inside
