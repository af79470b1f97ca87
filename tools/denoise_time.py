"""Device time of the denoiser (csrc/denoisekernel.hip) on the benchmark frame.

Coffee at 1920x1080 (bench.py's frame): the beauty and the AOVs of the same 4 seeds are rendered, then `denoise` is timed with HIP events
around the call on the library's stream (torch.cuda.Event on a torch stream the context is given; the output is bound to a torch tensor,
so only moptix_denoise is timed, not a read-back), for L = 0 (decode and final passes alone), 1, 3, 5 and 8 iterations with the other
parameters at their defaults.  Prints the median of --reps calls per L, the cost per
iteration, and the L = 5 time against the 2 ms target and the beauty frame.  Output (also written to --out): profiles/r08_denoise.txt.

  python tools/denoise_time.py [--reps 5] [--out profiles/r08_denoise.txt]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08_denoise.txt"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    import minimaloptix_amd as M
    from minimaloptix_amd import _capi as K
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    stream = torch.cuda.Stream()
    ctx = M.Context(0)
    ctx.set_stream(stream.cuda_stream)
    hs = M.HostScene("file:coffee", a.width, a.height)
    ctx.load(hs)
    seeds = M.launch_seeds(a.spp)
    ctx.accum_clear()
    ctx.kernel_time(reset=True)
    ctx.render(seeds)
    beauty = ctx.kernel_time()[0] + ctx.reduce_time()
    ctx.aov_clear()
    ctx.render_aovs(seeds)
    say("# r08: device time of the AOV-guided a-trous denoiser (csrc/denoisekernel.hip), python tools/denoise_time.py")
    say("coffee %dx%d, %d spp beauty (%.2f ms trace + reduction) + AOVs of the same seeds; defaults: normalPower 128, sigmaLuminance 4, "
        "sigmaDepth 1, no demodulation" % (a.width, a.height, a.spp, beauty))
    out = torch.empty((a.height, a.width, 3), dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.denoise_bind(out)
    p = K.DenoiseParams()
    assert K.device_lib().moptix_denoise_defaults(C.byref(p)) == 0

    def denoise():
        assert K.device_lib().moptix_denoise(ctx._h, C.byref(p), float(a.spp)) == 0, ctx.last_error()

    res = {}
    for it in (0, 1, 3, 5, 8):
        p.iterations = it
        denoise()                                                      # warm: code loaded, buffers allocated
        dev, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            denoise()                                                  # blocking
            wall.append((time.perf_counter() - t0) * 1e3)
            e1.record(stream)
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        res[it] = float(np.median(dev))
        say("L %d: %.3f ms device (HIP events, median of %d; min %.3f), %.3f ms host wall" % (
            it, res[it], a.reps, float(np.min(dev)), float(np.median(wall))))
    per_it = (res[8] - res[0]) / 8.0
    say("per iteration %.3f ms ((L8 - L0) / 8, the prepass shared out); L0 = decode + final passes %.3f ms" % (per_it, res[0]))
    say("verdict: 1080p L = 5 takes %.3f ms against the 2 ms target (%s); %.2f %% of a 256-spp beauty frame of 311 ms" % (
        res[5], "met" if res[5] <= 2.0 else "MISSED", 100.0 * res[5] / 311.0))
    ctx.denoise_bind(None)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
