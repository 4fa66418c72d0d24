#!/usr/bin/env python
"""A host-bound frame for the wavefront frame loop (csrc/device/fjgpu_frame.hip): the 90 x 60 glass scene of tests/test_gpu_frame_ledger.py, whose
launches are a few thousand rays each, so that the loop's own cost -- launches, counter round trips, event bookkeeping -- is what a frame takes.
Prints the median of fjgpu_stats.total_ms and of the call's wall time over `--calls` calls after `--warmup` calls.  To compare two builds of the
library, run it once per build with FJGPU_LIBDIR set (profiles/frame_loop_split.txt).

usage: python scripts/frame_loop_bench.py [--calls 20] [--warmup 5] [--label NAME]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    from edge_scenes import custom_scene
    from fujiyama_renderer_amd import gpu, host, workloads
    text = custom_scene(workloads.default_asset_dir(), res=(90, 60), obj_shader="glass_shader", ren_props=(("tilesize", (32, 32)),))
    host.run_scene_text(text, deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    try:
        for _ in range(a.warmup):
            gs.render_frame(rd)
        ms, wall = [], []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            _, st = gs.render_frame(rd)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(st.total_ms)
    finally:
        gs.close()
    print(json.dumps(dict(label=a.label, calls=a.calls, total_ms_median=round(float(np.median(ms)), 4), total_ms_min=round(min(ms), 4),
                          total_ms_max=round(max(ms), 4), wall_ms_median=round(float(np.median(wall)), 4),
                          launches=int(st.trace_launches + st.light_loop_launches), rays=int(st.rays.total()))))


if __name__ == "__main__":
    main()
