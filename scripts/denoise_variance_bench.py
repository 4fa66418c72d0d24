#!/usr/bin/env python3
"""Timing of the variance-guided denoiser on the synthetic frame of profiles/denoise_pass.txt, section 4 (profiles/denoise_variance.txt,
section 4): 1920 x 1080, random colours, unit normals, positions in a 3-unit box, ids in 97 x 61-pixel patches of 5 values incl. -1;
sigma_normal 1, sigma_position 0.5, stop_at_ids 1, and for the plain filter sigma_color 3.  HIP-event times of the calls' own launches
(fjgpu_stats), three calls each, all in one process: fjgpu_denoise_variance with an estimated and with a supplied variance,
fjgpu_denoise_estimate_variance alone, and fjgpu_denoise on the same inputs.  Per-iteration times are differences of the fastest
resolve_ms at n and n - 1 iterations.  bench.py does not call this.

    python scripts/denoise_variance_bench.py [--width 1920 --height 1080 --iterations 5 --calls 3]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fujiyama_renderer_amd import gpu          # noqa: E402


def frame(W, H, seed=4):
    rng = np.random.default_rng(seed)
    color = (rng.random((H, W, 4), dtype=np.float32) * 2).astype(np.float32)
    normal = rng.standard_normal((H, W, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    position = (rng.random((H, W, 3), dtype=np.float32) * 3).astype(np.float32)
    patch = rng.integers(-1, 4, ((H + 60) // 61, (W + 96) // 97)).astype(np.int32)
    ids = np.zeros((H, W, 4), dtype=np.int32)
    ids[:, :, 0] = np.repeat(np.repeat(patch, 61, axis=0), 97, axis=1)[:H, :W]
    variance = (rng.random((H, W), dtype=np.float32) * 0.5).astype(np.float32)
    return color, normal, position, ids, variance


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    import torch
    if gpu.device_count() < 1:
        raise SystemExit("needs a GPU")
    c, n, p, i, v = (torch.from_numpy(x).to("cuda:0") for x in frame(a.width, a.height))
    out = torch.empty_like(c)
    guides = dict(sigma_normal=1.0, sigma_position=0.5, stop_at_ids=True)
    arms = {
        "plain (fjgpu_denoise)": lambda k: gpu.denoise(c, n, p, i, iterations=k, sigma_color=3.0, out=out, **guides)[-1],
        "variance, estimated": lambda k: gpu.denoise_variance(c, n, p, i, iterations=k, out=out, **guides)[-1],
        "variance, supplied": lambda k: gpu.denoise_variance(c, n, p, i, variance=v, iterations=k, out=out, **guides)[-1],
    }
    for f in arms.values():          # first launches: code load, allocator
        f(1)
    print("%d x %d, %d iterations, %d calls each; ms" % (a.width, a.height, a.iterations, a.calls))
    print("    %-24s %-6s %-10s %-12s %-10s" % ("arm", "call", "gen_ms", "resolve_ms", "total_ms"))
    full = {}
    for name, f in arms.items():
        for k in range(a.calls):
            st = f(a.iterations)
            print("    %-24s %-6d %-10.3f %-12.3f %-10.3f" % (name, k + 1, st.gen_ms, st.resolve_ms, st.total_ms))
            full.setdefault(name, []).append(st.total_ms)
    est = []
    for k in range(a.calls):
        st = gpu.estimate_variance(c, n, p, i, **guides)[-1]
        print("    %-24s %-6d %-10.3f %-12s %-10.3f" % ("estimate alone", k + 1, st.gen_ms, "-", st.total_ms))
        est.append(st.total_ms)
    base = min(full["plain (fjgpu_denoise)"])
    for name in full:
        print("    fastest total, %-24s %.3f  (%.2f x plain)" % (name, min(full[name]), min(full[name]) / base))
    print("    fastest total, %-24s %.3f  (%.2f x plain)" % ("estimate alone", min(est), min(est) / base))
    print("per-iteration ms: fastest resolve_ms of n iterations minus that of n - 1")
    print("    %-24s %s" % ("spacing", "  ".join("%-7d" % (1 << k) for k in range(a.iterations))))
    for name, f in arms.items():
        best = [0.0] + [min(f(k).resolve_ms for _ in range(a.calls)) for k in range(1, a.iterations + 1)]
        print("    %-24s %s" % (name, "  ".join("%-7.3f" % (best[k] - best[k - 1]) for k in range(1, a.iterations + 1))))
    # the arms give the same colours where they must: sigma_luminance 0 is the plain filter at sigma_color 0
    x, _ = gpu.denoise_variance(c, n, p, i, sigma_luminance=0.0, iterations=a.iterations, **guides)
    y, _ = gpu.denoise(c, n, p, i, sigma_color=0.0, iterations=a.iterations, **guides)
    print("sigma_luminance 0 against the plain filter at sigma_color 0: %s" % ("bit-identical" if np.array_equal(x, y) else "DIFFERENT"))
    # checksums of both outputs, for comparing two builds of the library (FJGPU_LIBDIR) on the same frame
    for name, var in (("estimated", None), ("supplied", v)):
        x, xv, _ = gpu.denoise_variance(c, n, p, i, variance=var, iterations=a.iterations, return_variance=True, **guides)
        print("sha256 %-10s colour %s variance %s" % (name, hashlib.sha256(x.tobytes()).hexdigest()[:16], hashlib.sha256(xv.tobytes()).hexdigest()[:16]))


if __name__ == "__main__":
    main()
