#!/usr/bin/env python3
"""Timing of the sample-variance kernel on the headline frame (profiles/sample_variance.txt, section 3): the dragon scene at 1920 x 1080,
8 x 8 spp, one resident scene, fjgpu_render_tiles and fjgpu_render_tiles_variance called in turn into the same device buffers.  The figures
are the calls' own HIP-event times (fjgpu_stats): total_ms of the frame, and resolve_ms -- k_resolve alone in the first call, k_resolve plus
k_sample_variance in the second, so their difference is the new kernel's time beside k_resolve's from the same run.  bench.py does not
call this.

    python scripts/sample_variance_bench.py [--calls 8] [--workload dragon] [--res 1920 1080] [--spp 8 8] [--albedo]
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
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--workload", default="dragon", choices=sorted(workloads.BUILDERS))
    ap.add_argument("--mesh", default=None)
    ap.add_argument("--res", type=int, nargs=2, default=None)
    ap.add_argument("--spp", type=int, nargs=2, default=None)
    ap.add_argument("--albedo", action="store_true", help="take the variance under the albedo of fjgpu_render_aov_albedo")
    a = ap.parse_args()
    import torch
    if gpu.device_count() < 1:
        raise SystemExit("needs a GPU")
    kw = {k: tuple(v) for k, v in (("res", a.res), ("spp", a.spp)) if v}
    if a.mesh:
        kw["mesh"] = a.mesh
    host.run_scene_text(workloads.BUILDERS[a.workload](workloads.default_asset_dir(), **kw), deferred=True)
    sp, rd = host.get_desc()
    gs = gpu.Scene(sp)
    dev = torch.device("cuda", 0)
    fb = torch.zeros((rd.yres, rd.xres, 4), dtype=torch.float32, device=dev)
    var = torch.zeros((rd.yres, rd.xres), dtype=torch.float32, device=dev)
    albedo = gs._render_aov_device(rd, want=("albedo",), names=gpu.AOV_ALL)[0]["albedo"] if a.albedo else None
    torch.cuda.synchronize(dev)
    plain = lambda: gs.render_tiles(rd, None, fb.data_ptr())
    withv = lambda: gs.render_tiles(rd, None, fb.data_ptr(), variance=var.data_ptr(), albedo=None if albedo is None else albedo.data_ptr())
    for f in (plain, withv, plain, withv):          # the cold frame, the arena's growth, code load
        f()
    print("%s %d x %d, %d x %d spp, filter %g x %g: window %d x %d samples%s; %d calls each, in turn; ms" % (
        a.workload, rd.xres, rd.yres, rd.rate_x, rd.rate_y, rd.filter_w, rd.filter_h,
        rd.rate_x + 2 * int(np.ceil((rd.filter_w - 1) * rd.rate_x * .5)), rd.rate_y + 2 * int(np.ceil((rd.filter_h - 1) * rd.rate_y * .5)),
        ", under the albedo" if a.albedo else "", a.calls))
    print("    %-6s %-28s %-28s %s" % ("call", "fjgpu_render_tiles", "fjgpu_render_tiles_variance", "resolve_ms difference"))
    print("    %-6s %-13s %-14s %-13s %-14s" % ("", "total_ms", "resolve_ms", "total_ms", "resolve_ms"))
    rows = []
    for k in range(a.calls):
        s0, s1 = plain(), withv()
        rows.append((s0.total_ms, s0.resolve_ms, s1.total_ms, s1.resolve_ms))
        print("    %-6d %-13.3f %-14.3f %-13.3f %-14.3f %.3f" % ((k + 1,) + rows[-1] + (s1.resolve_ms - s0.resolve_ms,)))
        assert s0.rays.as_dict() == s1.rays.as_dict() and s0.batches == s1.batches
    r = np.array(rows)
    med = np.median(r, axis=0)
    print("    median %-13.3f %-14.3f %-13.3f %-14.3f %.3f" % (tuple(med) + (float(np.median(r[:, 3] - r[:, 1])),)))
    print("    fjgpu_render_tiles total_ms: min %.3f, max %.3f (the run-to-run spread); with the variance: min %.3f, max %.3f" % (
        r[:, 0].min(), r[:, 0].max(), r[:, 2].min(), r[:, 2].max()))
    v = var.cpu().numpy()
    print("    variance: finite %s, min %.3e, median %.3e, max %.3e, %d of %d pixels > 0; batches per call %d" % (
        bool(np.isfinite(v).all()), float(v.min()), float(np.median(v)), float(v.max()), int((v > 0).sum()), v.size, s1.batches))
    gs.close()


if __name__ == "__main__":
    main()
