#!/usr/bin/env python3
"""Cost of the progressive accumulation (profiles/accumulate_pass.txt): k_ac_accumulate and k_ac_tile_error over a whole-frame tile list,
beside a device-to-device copy that moves the same bytes, and the host cost of a change of the sampler seed.

Kernel times are the HIP-event times of the calls' own launches (fjgpu_stats.total_ms); the copy is timed with torch's events around
Tensor.copy_.  The kinds are interleaved call by call; a round is the median of its calls, the figure the median of the rounds with their
least and greatest.  The seed change is timed on the host around Scene.render_tiles of ONE tile of the headline's size and sampling rate
(a tiny mesh, so the render itself is short): calls that alternate between two seeds against calls that keep one, and the table build
(fjgpu_host_xorshift_f01_seeded) on its own.

    python scripts/accumulate_pass_bench.py [--res 1920 1080] [--tile 64] [--spp 8 8] [--warmup 3] [--rounds 7] [--calls 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fujiyama_renderer_amd import gpu, host, workloads          # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--spp", type=int, nargs=2, default=(8, 8))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    W, H = a.res
    dev = torch.device("cuda", 0)
    rects = np.array([(x, y, min(x + a.tile, W), min(y + a.tile, H)) for y in range(0, H, a.tile) for x in range(0, W, a.tile)], np.int32)
    g = torch.Generator(device=dev).manual_seed(1)
    frames = [torch.rand((H, W, 4), generator=g, device=dev) for _ in range(2)]
    state = gpu.new_accum_state((H, W))
    var = torch.zeros((H, W), device=dev)
    src, dst = torch.rand((H, W, 8), generator=g, device=dev), torch.zeros((H, W, 8), device=dev)      # 32 B read + 32 B written per pixel
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy():
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    n = [0]

    def frame():
        n[0] += 1
        return frames[n[0] & 1]

    kinds = [
        ("device-to-device copy, 64 B / pixel", copy),
        ("k_ac_accumulate, %d tiles of %d" % (len(rects), a.tile), lambda: gpu.accumulate(frame(), state, rects=rects)[2].total_ms),
        ("k_ac_accumulate, the same with variance_out", lambda: gpu.accumulate(frame(), state, rects=rects, variance_out=var)[2].total_ms),
        ("k_ac_accumulate, one whole-frame rect", lambda: gpu.accumulate(frame(), state)[2].total_ms),
        ("k_ac_tile_error, %d tiles of %d" % (len(rects), a.tile), lambda: gpu.tile_errors(state, rects=rects)[1].total_ms),
    ]
    for _ in range(a.warmup):
        for _, call in kinds:
            call()
    rounds = {name: [] for name, _ in kinds}
    for _ in range(a.rounds):
        ms = {name: [] for name, _ in kinds}
        for _ in range(a.calls):
            for name, call in kinds:
                ms[name].append(call())
        for name, _ in kinds:
            rounds[name].append(float(np.median(ms[name])))
    px = W * H
    print("%d x %d, warm-up %d, %d rounds of %d interleaved calls: median of the rounds' medians [least .. greatest], ms; GB/s of the bytes named"
          % (W, H, a.warmup, a.rounds, a.calls))
    bytes_px = [64, 64, 68, 64, 28]
    for (name, _), b in zip(kinds, bytes_px):
        v = np.array(rounds[name])
        m = float(np.median(v))
        print("    %-46s %7.4f [%7.4f .. %7.4f]   %3d B/pixel  %7.1f GB/s" % (name, m, v.min(), v.max(), b, px * b / m / 1e6))

    # ---- the seed change: one tile of the headline's size and rate
    host.run_scene_text(workloads.dragon(workloads.default_asset_dir(), res=(2 * a.tile, 2 * a.tile), spp=tuple(a.spp), mesh="tiny",
                                         extra=(("tilesize", (a.tile, a.tile)),)), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    fb = torch.zeros((rd.yres, rd.xres, 4), device=dev)
    torch.cuda.synchronize(dev)

    def render(seed):
        t0 = time.perf_counter()
        gs.set_option("sampler_seed", seed)
        gs.render_tiles(rd, [0], fb.data_ptr())
        return (time.perf_counter() - t0) * 1e3

    for s in (1, 2, 1, 2):
        render(s)
    keep, change = [], []
    for r in range(a.rounds * a.calls):
        render(1)
        keep.append(render(1))
        change.append(render(2))
    gs.close()
    import ctypes as C
    m = (C.c_int32 * 2)()
    gpu.lib().fjgpu_host_sampler_margin(C.byref(rd), m)
    tab_len = (a.tile * rd.rate_x + 2 * m[0]) * (a.tile * rd.rate_y + 2 * m[1])
    build = []
    for _ in range(a.rounds * a.calls):
        t0 = time.perf_counter()
        gpu.host_xorshift_f01_seeded(3, 2 * tab_len)
        build.append((time.perf_counter() - t0) * 1e3)
    q = lambda v: "%7.3f [%7.3f .. %7.3f]" % (float(np.median(v)), min(v), max(v))
    print("seed change, one tile of %d x %d pixels at %d x %d spp (%d samples with the margin; tables of 3 x %d doubles = %.2f MB):"
          % (a.tile, a.tile, rd.rate_x, rd.rate_y, tab_len, tab_len, 24e-6 * tab_len))
    print("    render_tiles of the tile, host clock, ms: seed kept %s   seed changed %s   difference of the medians %.3f"
          % (q(keep), q(change), float(np.median(change)) - float(np.median(keep))))
    print("    the table build alone (fjgpu_host_xorshift_f01_seeded, 2 x %d draws), host clock, ms: %s" % (tab_len, q(build)))


if __name__ == "__main__":
    main()
