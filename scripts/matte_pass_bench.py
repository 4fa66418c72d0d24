#!/usr/bin/env python3
"""Cost of the matte reduction (k_aov_matte, fjgpu_render_aov_matte) beside k_aov_reduce (fjgpu_render_aov, six buffers) and the closest-hit
walk of the same calls (profiles/matte_pass.txt): HIP-event times of the calls' own launches (fjgpu_stats).  The kinds of call are
interleaved call by call; a round is the median of its calls, the figure the median of the rounds with their least and greatest.

    python scripts/matte_pass_bench.py [--workload dragon|buddhas] [--res W H] [--spp X Y] [--ranks 4] [--warmup 2] [--rounds 5] [--calls 3]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fujiyama_renderer_amd import gpu, host, workloads          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="dragon")
    ap.add_argument("--res", type=int, nargs=2, default=None)
    ap.add_argument("--spp", type=int, nargs=2, default=None)
    ap.add_argument("--ranks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    kw = {}
    if a.res:
        kw["res"] = tuple(a.res)
    if a.spp:
        kw["spp"] = tuple(a.spp)
    host.run_scene_text(getattr(workloads, a.workload)(workloads.default_asset_dir(), **kw), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    kinds = [("render_aov, six buffers", lambda: gs._render_aov_device(rd)[1])]
    for key in ("instance", "shader"):
        for filtered in (True, False):
            kinds.append(("matte, %s key, %s" % (key, "filtered" if filtered else "own samples"),
                          lambda key=key, filtered=filtered: gs._render_matte_device(rd, key=key, ranks=a.ranks, filtered=filtered)[1]))
    for _ in range(a.warmup):
        for _, call in kinds:
            call()
    cols = ("total_ms", "gen_ms", "closest_ms", "resolve_ms")
    rounds = {name: [] for name, _ in kinds}
    for _ in range(a.rounds):
        ms = {name: [] for name, _ in kinds}
        for _ in range(a.calls):
            for name, call in kinds:
                st = call()
                ms[name].append([getattr(st, c) for c in cols])
        for name, _ in kinds:
            rounds[name].append(np.median(np.array(ms[name]), axis=0))
    t, st = gs._render_matte_device(rd, key="instance", ranks=a.ranks, filtered=True)
    d = t["distinct"].cpu().numpy()
    print("%s %d x %d, %d x %d spp, filter %g x %g, %d camera rays, %d batches, ranks %d; distinct keys per pixel (filtered, instance): %s"
          % (a.workload, rd.xres, rd.yres, rd.rate_x, rd.rate_y, rd.filter_w, rd.filter_h, st.rays.camera, st.batches, a.ranks,
             " ".join("%d:%d" % (k, n) for k, n in enumerate(np.bincount(d.ravel())) if n)))
    print("warm-up %d, %d rounds of %d interleaved calls: median of the rounds' medians [least .. greatest], ms" % (a.warmup, a.rounds, a.calls))
    print("    %-36s %s" % ("", "  ".join("%-26s" % c for c in cols)))
    for name, _ in kinds:
        v = np.array(rounds[name])
        print("    %-36s %s" % (name, "  ".join("%7.3f [%7.3f .. %7.3f]" % (float(np.median(v[:, k])), v[:, k].min(), v[:, k].max())
                                                for k in range(len(cols)))))
    gs.close()


if __name__ == "__main__":
    main()
