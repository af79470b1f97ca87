"""Cost of the first-hit AOV pass (csrc/aovkernel.hip) against the beauty frame on the same seeds.

Coffee at 1920x1080 (bench.py's frame): for 16 and 256 seeds the beauty frame is rendered as bench.py renders it (warm: one frame
first, then timed ones, the trace kernels' device time from moptix_kernel_time), then render_aovs on the same seeds is timed with HIP
events around the call on the library's stream (torch.cuda.Event on a torch stream the context is given).  Prints the primary rays per
second of the AOV pass and its time as a share of the beauty frame's.  Output: profiles/r07_aov_pass.txt.

  python tools/aov_time.py [--reps 3]
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import torch
    import minimaloptix_amd as M
    stream = torch.cuda.Stream()
    ctx = M.Context(0)
    ctx.set_stream(stream.cuda_stream)
    hs = M.HostScene("file:coffee", a.width, a.height)
    ctx.load(hs)
    print("coffee %dx%d, %d triangles, BVH depth %d" % (a.width, a.height, ctx.accel_info().nTriangles, ctx.accel_info().treeDepth))
    for spp in (16, 256):
        seeds = M.launch_seeds(spp)
        ctx.accum_clear(); ctx.render(seeds)                            # warm: code loaded, node format decided, depth history
        beauty = []
        for _ in range(a.reps):
            ctx.accum_clear()
            ctx.kernel_time(reset=True)
            ctx.render(seeds)
            ms, n = ctx.kernel_time()
            beauty.append(ms + ctx.reduce_time())
        ctx.aov_clear(); ctx.render_aovs(seeds)                         # warm
        aov, wall = [], []
        for _ in range(a.reps):
            ctx.aov_clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            ctx.render_aovs(seeds)                                       # blocking
            wall.append((time.perf_counter() - t0) * 1e3)
            e1.record(stream)
            e1.synchronize()
            aov.append(e0.elapsed_time(e1))
        rays = float(a.width * a.height * spp)
        b, v = float(np.median(beauty)), float(np.median(aov))
        print("seeds %3d: beauty frame %.2f ms (trace + reduction, median of %d) | AOV pass %.2f ms (HIP events; %.2f ms host wall) = %.2f G primary rays/s, "
              "%.1f %% of the beauty frame" % (spp, b, a.reps, v, float(np.median(wall)), rays / v * 1e-6, 100.0 * v / b))
        m = ctx.aov_means()
        print("           mean albedo %.4f, %.1f %% of the pixels hit something" % (float(m["albedo"].mean()), 100.0 * float(np.isfinite(m["depth"]).mean())))
    ctx.close()


if __name__ == "__main__":
    main()
