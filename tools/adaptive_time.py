"""What adaptive sampling costs and buys on one MI355X (profiles/r10_adaptive.txt, DESIGN.md "Adaptive sampling").

    python3 tools/adaptive_time.py [--scene file:coffee] [--width 1920 --height 1080] [--seeds 256] [--ref-seeds 2048] [--reduce-only]

1 Overhead of the machinery alone: threshold 0 (every pixel takes every pass) with minSamples = batch = 16, 32, 64 and 16 + n x 32 / 64 against
  moptix_render of the same seeds in the same process, three alternations, by moptix_kernel_time + moptix_reduce_time and by wall clock.
2 The gain: the shipped defaults on the same seeds -- samples traced, wall time, and the RMSE of both against a plain render of
  --ref-seeds disjoint seeds.
--reduce-only renders one 16-seed pass each way and nothing else: run it under `rocprofv3 --kernel-trace --stats` to compare
k_ad_reduce with k_reduce_samples on the same pass."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import minimaloptix_amd as M      # noqa: E402


def rmse(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


def timed(ctx, f):
    ctx.kernel_time(reset=True)
    t = time.perf_counter()
    out = f()
    wall = (time.perf_counter() - t) * 1e3
    return out, wall, ctx.kernel_time()[0] + ctx.reduce_time(), ctx.kernel_time()[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="file:coffee")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--ref-seeds", type=int, default=2048)
    ap.add_argument("--reduce-only", action="store_true")
    a = ap.parse_args()
    ctx = M.Context(0)
    ctx.load(M.HostScene(a.scene, a.width, a.height))
    seeds = M.launch_seeds(a.seeds, 0, 0)
    if a.reduce_only:
        ctx.set_option("kernel_variant", 4)      # the same trace kernel both ways
        ctx.accum_clear(); ctx.render(seeds[:16])
        ctx.adaptive_clear(); ctx.render_adaptive(seeds[:16], threshold=0.0, min_samples=16, batch=16)
        print("one 16-seed pass each way at %dx%d" % (a.width, a.height))
        return
    ctx.accum_clear(); ctx.render(seeds)             # warm-up: allocations, node format, depth history
    print("%s %dx%d, %d seeds; wall ms | kernel + reduce ms | launches" % (a.scene, a.width, a.height, a.seeds))
    for rep in range(3):
        ctx.accum_clear()
        _, w, k, n = timed(ctx, lambda: ctx.render(seeds))
        print("  plain render                      %8.1f | %8.1f | %d" % (w, k, n))
        plain = ctx.accum_read()
        for first, batch in ((16, 16), (32, 32), (64, 64), (16, 32), (16, 64)):
            ctx.adaptive_clear()
            st, w, k, n = timed(ctx, lambda: ctx.render_adaptive(seeds, threshold=0.0, min_samples=first, batch=batch))
            same = bool((ctx.accum_read().view(np.uint32) == plain.view(np.uint32)).all())
            print("  adaptive, threshold 0, %2d + n x %-2d  %8.1f | %8.1f | %d   (%d passes, same bits as the plain render: %s)" % (first, batch, w, k, n, st["passes"], same))
        ctx.adaptive_clear()
    d = ctx.adaptive_defaults()
    for batch in (16, 32, d["batch"]):
        for rep in range(3):
            ctx.adaptive_clear()
            st, w, k, n = timed(ctx, lambda: ctx.render_adaptive(seeds, batch=batch))
            print("  adaptive, threshold %.3g, %d + n x %-2d %8.1f | %8.1f | %d   %s" % (d["threshold"], d["min_samples"], batch, w, k, n, st))
    mean = ctx.adaptive_mean()
    count = ctx.adaptive_read()["count"]
    hist = dict(zip(*[x.tolist() for x in np.unique(count, return_counts=True)]))
    print("  samples traced / uniform: %.4f; pixels per count: %s" % (st["samples_traced"] / st["samples_uniform"], hist))
    ctx.adaptive_clear()
    ref_seeds = M.launch_seeds(a.ref_seeds, 0, 100000)
    for i in range(0, a.ref_seeds, 256):
        ctx.render(ref_seeds[i:i + 256])
    ref = ctx.accum_read() / np.float32(a.ref_seeds)
    print("  RMSE against %d disjoint seeds: plain %d seeds %.5f, adaptive %.5f" % (a.ref_seeds, a.seeds, rmse(plain / np.float32(a.seeds), ref), rmse(mean, ref)))
    n_eq = -(-st["samples_traced"] // (a.width * a.height))
    ctx.accum_clear(); ctx.render(seeds[:n_eq])
    print("  plain render of %d seeds (the equal-cost opponent): RMSE %.5f" % (n_eq, rmse(ctx.accum_read() / np.float32(n_eq), ref)))
    ctx.close()


if __name__ == "__main__":
    main()
