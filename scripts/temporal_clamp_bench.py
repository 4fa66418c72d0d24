#!/usr/bin/env python3
"""resolve_ms of fjgpu_denoise_temporal_clamped for radius 1, 2, 3 against fjgpu_denoise_temporal on the same device buffers
(profiles/temporal_clamp.txt): a wall facing the camera, seen from an eye that moved by 0.4 pixel, with an albedo, a spatial variance and a
history of length 3 -- every pixel has a history, so every pixel walks its window.  The four passes are interleaved call by call; a round
is the median of its calls, the figure the median of the rounds with their least and greatest.

    python scripts/temporal_clamp_bench.py [--res 1920 1080] [--warmup 20] [--rounds 11] [--calls 30] [--against OTHER/libfjgpu.so]

--against: another build of libfjgpu.so (the parent commit's, say) whose fjgpu_denoise_temporal is timed in the same interleaving.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fujiyama_renderer_amd import ffi, gpu          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--against", default=None)
    a = ap.parse_args()
    import torch
    W, H = a.res
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    px = 1.0 / 256                                         # a pixel at depth 4 in world units: uv_size = (4 W px / 4, ...) below
    eye = 0.4 * px

    def wall(e):
        return np.stack([(x - W / 2) * px + e, (H / 2 - y) * px, np.full_like(x, -4.0)], axis=-1).astype(np.float32)

    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    normal = np.zeros((H, W, 3), dtype=np.float32)
    normal[..., 2] = 1
    ids = np.zeros((H, W, 4), dtype=np.int32)
    ids[:, W // 2:, 0] = 1                                 # two objects, so that the id stop has something to compare
    t = dict(color=up(rng.random((H, W, 4), dtype=np.float32)), position=up(wall(eye)), normal=up(normal), ids=up(ids),
             albedo=up(0.2 + 0.6 * rng.random((H, W, 3), dtype=np.float32)), vs=up(rng.random((H, W), dtype=np.float32)),
             pposition=up(wall(0.0)), pcolor=up(rng.random((H, W, 4), dtype=np.float32)), pmoments=up(rng.random((H, W, 2), dtype=np.float32)),
             plength=up(np.full((H, W), 3, dtype=np.float32)), ncolor=torch.zeros((H, W, 4), device=dev), nmoments=torch.zeros((H, W, 2), device=dev),
             nlength=torch.zeros((H, W), device=dev), var=torch.zeros((H, W), device=dev), amount=torch.zeros((H, W), device=dev))
    torch.cuda.synchronize(dev)
    view = ffi.View()
    view.world_to_camera[:] = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    view.uv_size[:] = (W * px / 4.0, H * px / 4.0)
    view.xres, view.yres = W, H
    d = ffi.TemporalDesc()
    d.xres, d.yres = W, H
    d.region[:] = (0, 0, W, H)
    d.alpha_min, d.max_history, d.tol_position, d.cos_normal = gpu.ALPHA_MIN, gpu.MAX_HISTORY, 0.05, gpu.COS_NORMAL
    d.min_history_variance, d.albedo_floor = gpu.MIN_HISTORY_VARIANCE, gpu.ALBEDO_FLOOR
    hp, hn = ffi.TemporalHistory(), ffi.TemporalHistory()
    hp.color, hp.moments, hp.length = (t[k].data_ptr() for k in ("pcolor", "pmoments", "plength"))
    hn.color, hn.moments, hn.length = (t[k].data_ptr() for k in ("ncolor", "nmoments", "nlength"))
    p = lambda k: C.c_void_p(t[k].data_ptr())
    st = ffi.GpuStats()
    args = (p("color"), p("position"), p("normal"), p("ids"), p("albedo"), p("vs"), C.byref(view), p("pposition"), p("normal"), p("ids"),
            C.byref(hp), C.byref(hn), p("var"), None, C.byref(st))
    L = gpu.lib()
    other = None
    if a.against:
        other = C.CDLL(os.path.abspath(a.against))
        other.fjgpu_denoise_temporal.argtypes = L.fjgpu_denoise_temporal.argtypes

    def call(radius):
        if radius <= 0:
            rc = (L if radius == 0 else other).fjgpu_denoise_temporal(0, C.byref(d), *args)
        else:
            cl = ffi.TemporalClamp()
            cl.radius, cl.gamma, cl.stop_at_ids, cl.amount = radius, gpu.CLAMP_GAMMA, 1, t["amount"].data_ptr()
            rc = L.fjgpu_denoise_temporal_clamped(0, C.byref(d), C.byref(cl), *args)
        assert rc == 0, L.fjgpu_last_error()
        return st.resolve_ms

    kinds = (0, 1, 2, 3) + ((-1,) if other else ())
    names = {0: "unclamped", -1: "unclamped, " + str(a.against)}
    for _ in range(a.warmup):
        for r in kinds:
            call(r)
    assert abs(float(t["nlength"].min()) - 4.0) <= 1e-4, "a pixel without history"
    rounds = {r: [] for r in kinds}
    for _ in range(a.rounds):
        ms = {r: [] for r in kinds}
        for _ in range(a.calls):
            for r in kinds:
                ms[r].append(call(r))
        for r in kinds:
            rounds[r].append(float(np.median(ms[r])))
    print("%d x %d, warm-up %d, %d rounds of %d interleaved calls: resolve_ms, median of the rounds' medians [least .. greatest]"
          % (W, H, a.warmup, a.rounds, a.calls))
    for r in kinds:
        v = rounds[r]
        print("    %-28s %.4f  [%.4f .. %.4f]" % (names.get(r, "clamped, radius %d" % r), float(np.median(v)), min(v), max(v)))


if __name__ == "__main__":
    main()
