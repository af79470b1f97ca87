"""What an in-place refit costs and what it costs the frames after it (csrc/refitkernel.hip), against a rebuild.

    python3 tools/refit_time.py [--reps 10] [--spp 16] [--width 1920 --height 1080] [--scenes coffee,dining_standin,million_standin]

Per scene: the build's own time (moptix_get_accel_info buildMs), a full re-upload-and-rebuild through Context.load (wall clock), the
refit's device time (HIP events, moptix_get_refit_info refitMs: the first call, which makes the plan outside the events, and the median /
minimum / maximum of --reps warm ones), and for a sinusoidal displacement p + a sin(7 p.yzx + 0.3) of every vertex at a = 0, 1 % and 10 %
of the scene's extent, moved on the device and handed over as a torch tensor: sahCost / sahCostBuilt and the warm --spp frame (trace
kernel time, HIP events) on the refitted tree and on a tree rebuilt from the same positions.  Prints the table that profiles/r13_refit.txt keeps."""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import minimaloptix_amd as M          # noqa: E402

SCENES = dict(coffee=("file:coffee", {}), dining_standin=("dining_standin", dict(iarg=6)), million_standin=("million_standin", dict(iarg=1000000)))


def frame_ms(ctx, seeds, reps=3):
    """trace-kernel time of one warm frame: the minimum of reps after one warm-up"""
    best = None
    for i in range(reps + 1):
        ctx.accum_clear(); ctx.kernel_time(reset=True)
        ctx.render(seeds)
        ms = ctx.kernel_time()[0]
        if i > 0:
            best = ms if best is None else min(best, ms)
    return best


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scenes", default="coffee,dining_standin,million_standin")
    a = ap.parse_args()
    seeds = M.launch_seeds(a.spp)
    dev = torch.device("cuda", 0)
    print("# refit_time: %dx%d, %d spp frames, %d warm refits; times in ms" % (a.width, a.height, a.spp, a.reps))
    for name in a.scenes.split(","):
        kind, kw = SCENES[name]
        hs = M.HostScene(kind, a.width, a.height, **kw)
        ctx = M.Context(0)
        ctx.load(hs)
        t0 = time.perf_counter(); ctx.load(hs); load_ms = 1e3 * (time.perf_counter() - t0)
        info = ctx.accel_info()
        base = torch.from_numpy(hs.face_arrays()[0]).to(dev).reshape(-1, 3)
        ext = float((base.max(dim=0).values - base.min(dim=0).values).max())
        first = ctx.refit_accel()
        warm = []
        for _ in range(a.reps):
            ctx.update_faces(0, base.reshape(-1, 9))
            warm.append(ctx.refit_accel()["refitMs"])
        med = float(np.median(warm))
        print("%s: %d triangles, %d nodes, depth %d | buildMs %.3f | load (upload + build, wall) %.1f | refit first %.3f, warm median %.3f min %.3f max %.3f | "
              "warm refit / buildMs %.3f %s" % (name, info.nTriangles, info.nNodes, info.treeDepth, info.buildMs, load_ms, first["refitMs"], med, min(warm),
                                                max(warm), med / info.buildMs, "BELOW" if med < info.buildMs else "NOT BELOW"))
        for share in (0.0, 0.01, 0.10):
            amp = share * ext
            moved = (base + amp * torch.sin(7.0 * base[:, [1, 2, 0]] + 0.3)).reshape(-1, 9).contiguous()
            ctx.load(hs)
            ctx.update_faces(0, moved)
            r = ctx.refit_accel()
            f_refit = frame_ms(ctx, seeds)
            ctx.update_faces(0, moved)
            ctx.build_accel("Trbvh")
            f_build = frame_ms(ctx, seeds)
            print("  amplitude %4.1f %%: sahCost / sahCostBuilt %.4f | refit %.3f | frame on the refitted tree %.2f, on a rebuilt tree %.2f (buildMs %.3f) | ratio %.3f | has64 %d"
                  % (100 * share, r["sahCost"] / r["sahCostBuilt"], r["refitMs"], f_refit, f_build, ctx.accel_info().buildMs, f_refit / f_build, r["has64"]))
        ctx.close()


if __name__ == "__main__":
    main()
