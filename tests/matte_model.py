"""numpy restatement of fjgpu_render_aov_matte's definition (include/fjgpu.h; csrc/device/fjgpu_matte_math.h), f64 sums.

Written from the header's text.  For pixel p = (px, py), its samples s with a key k_s (-1: a miss or an unassigned shader, never ranked)
and a weight w_s:
  filtered   the npx_x * npx_y samples of the filter window, first sample = tile's slot + (py - ymin) rate_y nx + (px - xmin) rate_x,
             row-major with nx samples per tile row; w_s = exp(-2 (xx xx + yy yy)), xx = 2 (xres u - (px + .5)) / fw,
             yy = 2 (yres (1 - v) - (py + .5)) / fh (sample_variance_model.weight: the same statement)
  own        the rate_x * rate_y samples margin_x, margin_y further in; w_s = 1
  W = sum w_s over all samples.  Keys in ascending order: A = sum of w_s with that key; (key, A) goes into a list of `ranks` entries before
  the first entry whose weight is strictly smaller (so equal weights stay in ascending key order); what falls off the end, or never gets
  into a full list, adds its weight to R.
  ids[r], coverage[r] = f32(A_r / W) (-1, 0 for an empty rank), rest = f32(R / W), distinct = number of keys.  Own mode: the quotients are
  f32(count) / f32(samples).
The sums here are numpy's (pairwise), the twin's are row-major and the kernel's a butterfly: in filtered mode they differ by f64
roundings; in own mode every sum is a count and everything is exact.

The second half computes what the pass reads from a scene without the pass: the film positions of a tile's samples from the sampler's
formula (FixedGridSampler::generate_samples with the per-tile XorShift stream: fjgpu_host_xorshift_f01, fjgpu_host_sampler_margin) and
the key of every sample from the oracle's trace of the tile's camera rays, with the face groups and GetShader's slot rules.
"""
import ctypes as C

import numpy as np

import sample_variance_model as svm

F = np.float32
KEY_INSTANCE, KEY_SHADER = 0, 1


def rank(keys, w, ranks, filtered):
    """one pixel: keys [n] int, w [n] f64 -> (ids [ranks] int32, coverage [ranks] f32, rest f32, distinct int, A [ranks] f64 (-1: empty), W)"""
    keys = np.asarray(keys)
    w = np.asarray(w, dtype=np.float64)
    W = w.sum()
    entries = []                      # (key, A), ranked
    R = 0.0
    visited = np.unique(keys[keys >= 0])          # ascending
    for k in visited:
        A = w[keys == k].sum()
        at = len(entries)
        for r, (_, a) in enumerate(entries):
            if a < A:
                at = r
                break
        entries.insert(at, (int(k), A))
        if len(entries) > ranks:
            R += entries.pop()[1]
    ids = np.full(ranks, -1, dtype=np.int32)
    cov = np.zeros(ranks, dtype=np.float32)
    Aout = np.full(ranks, -1.0)
    n = len(keys)

    def share(a):
        return F(a / W) if filtered else F(F(a) / F(n))
    for r, (k, a) in enumerate(entries):
        ids[r], cov[r], Aout[r] = k, share(a), a
    return ids, cov, share(R), len(visited), Aout, W


def tiles_matte(frame, tiles, s_uv, keys, filtered, ranks, out=None):
    """the pass over sample arrays as the AOV pass holds them: frame = dict(xres, yres, rate_x, rate_y, npx_x, npx_y, fw, fh, margin_x,
    margin_y); tiles = dicts of xmin, ymin, xmax, ymax, nx, sample_offset; s_uv [n, 2] f64 (None in own mode), keys [n] int32
    -> dict(ids, coverage [yres, xres, ranks], rest, distinct [yres, xres, 1], A [yres, xres, ranks] f64, W [yres, xres] f64); `out`: such
    a dict whose pixels outside the tiles are kept"""
    fr = frame
    H, Wd = fr["yres"], fr["xres"]
    if out is None:
        out = dict(ids=np.zeros((H, Wd, ranks), np.int32), coverage=np.zeros((H, Wd, ranks), np.float32), rest=np.zeros((H, Wd, 1), np.float32),
                   distinct=np.zeros((H, Wd, 1), np.int32))
    out.setdefault("A", np.full((H, Wd, ranks), -1.0))
    out.setdefault("W", np.zeros((H, Wd)))
    nwx, nwy = (fr["npx_x"], fr["npx_y"]) if filtered else (fr["rate_x"], fr["rate_y"])
    ox, oy = (0, 0) if filtered else (fr["margin_x"], fr["margin_y"])
    sy, sx = np.mgrid[0:nwy, 0:nwx]
    for T in tiles:
        for py in range(T["ymin"], T["ymax"]):
            for px in range(T["xmin"], T["xmax"]):
                first = T["sample_offset"] + ((py - T["ymin"]) * fr["rate_y"] + oy) * T["nx"] + (px - T["xmin"]) * fr["rate_x"] + ox
                s = (first + sy * T["nx"] + sx).reshape(-1)
                w = svm.weight(fr["xres"], fr["yres"], fr["fw"], fr["fh"], px, py, s_uv[s, 0], s_uv[s, 1]) if filtered else np.ones(s.size)
                ids, cov, rest, n, A, W = rank(keys[s], w, ranks, filtered)
                out["ids"][py, px], out["coverage"][py, px], out["rest"][py, px, 0], out["distinct"][py, px, 0] = ids, cov, rest, n
                out["A"][py, px], out["W"][py, px] = A, W
    return out


# ---- from a scene: sample positions and keys

def frame_of(rd, margin):
    """the frame description of tiles_matte from an ffi.RenderDesc and the sampler's margin (fjgpu_host_sampler_margin)"""
    mx, my = margin
    return dict(xres=rd.xres, yres=rd.yres, rate_x=rd.rate_x, rate_y=rd.rate_y, npx_x=rd.rate_x + 2 * mx, npx_y=rd.rate_y + 2 * my,
                fw=float(rd.filter_w), fh=float(rd.filter_h), margin_x=mx, margin_y=my)


def tile_uv(lib, rd, rect, margin):
    """film positions (u, v) [ny * nx, 2] of the samples of the tile with pixel rectangle rect = (xmin, ymin, xmax, ymax), in sample order
    k = y nx + x: FixedGridSampler::generate_samples (src/fj_fixed_grid_sampler.cc:33-84); the XorShift stream restarts per tile, draws 2k
    and 2k + 1 jitter sample k"""
    xmin, ymin, xmax, ymax = rect
    mx, my = margin
    nx, ny = rd.rate_x * (xmax - xmin) + 2 * mx, rd.rate_y * (ymax - ymin) + 2 * my
    udelta, vdelta = 1. / (rd.rate_x * rd.xres), 1. / (rd.rate_y * rd.yres)
    y, x = np.mgrid[0:ny, 0:nx]
    u = (.5 + x + (xmin * rd.rate_x - mx)) * udelta
    v = 1 - (.5 + y + (ymin * rd.rate_y - my)) * vdelta
    if rd.jitter > 0:
        draws = np.empty(2 * nx * ny)
        lib.fjgpu_host_xorshift_f01(draws.size, draws.ctypes.data_as(C.c_void_p))
        d = draws.reshape(ny, nx, 2)
        u = u + udelta * (d[:, :, 0] * float(rd.jitter) - .5)
        v = v + vdelta * (d[:, :, 1] * float(rd.jitter) - .5)
    return np.stack([u.reshape(-1), v.reshape(-1)], axis=1)


def sample_keys(view, ids, key, shader_slot):
    """the key of every sample from the oracle's trace ids [n, 2] = (instance, primitive; -1: miss): the instance, or the shader slot of
    the hit face's group (a curve: group 0) by GetShader's rules (test_gpu_aov.shader_slot)"""
    inst = ids[:, 0].astype(np.int32)
    if key == KEY_INSTANCE:
        return np.where(inst >= 0, inst, -1).astype(np.int32)
    out = np.full(inst.size, -1, dtype=np.int32)
    for ii in np.unique(inst[inst >= 0]):
        I = view.instances[int(ii)]
        sel = inst == ii
        fg = None if I["curve"] else view.meshes[I["primset"]]["fg"]
        if fg is None:
            out[sel] = shader_slot(I, 0)
        else:
            sg = fg[ids[sel, 1]]
            slots = {int(g): shader_slot(I, int(g)) for g in np.unique(sg)}
            out[sel] = [slots[int(g)] for g in sg]
    return out


def expected_matte(lib, gs, osc, view, rd, tile_rects, margin, key, ranks, filtered, shader_slot, out=None, traces=None):
    """the four buffers (and A, W) as the header defines them, for the tiles with pixel rectangles tile_rects = {tile id: rect}: keys from
    the oracle's trace of Scene.camera_samples, film positions from the sampler's formula.  traces: a dict that keeps the oracle's ids per
    tile between calls (the trace does not depend on key, ranks or mode).  -> (dict, samples traced)"""
    fr = frame_of(rd, margin)
    n_rays = 0
    for tile, rect in tile_rects.items():
        if traces is not None and tile in traces:
            ids = traces[tile]
        else:
            rays = gs.camera_samples(rd, int(tile))
            _, ids, _ = osc.trace(view.target_group, rays)
            if traces is not None:
                traces[tile] = ids
        uv = tile_uv(lib, rd, rect, margin)
        assert uv.shape[0] == ids.shape[0]
        n_rays += ids.shape[0]
        T = dict(xmin=rect[0], ymin=rect[1], xmax=rect[2], ymax=rect[3], nx=rd.rate_x * (rect[2] - rect[0]) + 2 * margin[0], sample_offset=0)
        out = tiles_matte(fr, [T], uv, sample_keys(view, ids, key, shader_slot), filtered, ranks, out=out)
    return out, n_rays
