"""Device time of the temporal denoiser entry (csrc/temporalkernel.hip) beside the spatial one on the benchmark frame.

Coffee at 1920x1080 (bench.py's frame): the beauty and the AOVs of the same 4 seeds are rendered, then moptix_denoise and
moptix_denoise_temporal, both at L = 5 with the defaults, are timed in the same run with HIP events around the call on the library's
stream (torch.cuda.Event on a torch stream the context is given; the output is bound to a torch tensor, so no read-back is timed).
The temporal entry is timed on its first frame (no history to fetch) and in steady state with a camera that moves between calls, so
that the four taps are real gathers; L = 0 isolates the reproject and reduce kernels (the window also holds the counters' 32-byte read-back).  Prints the median of --reps calls.  Output (also written to
--out): profiles/r09_temporal.txt.

  python tools/temporal_time.py [--reps 9] [--out profiles/r09_temporal.txt]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09_temporal.txt"))
    a = ap.parse_args()
    import ctypes as C
    import torch
    import minimaloptix_amd as M
    from minimaloptix_amd import _capi as K
    L = K.device_lib()
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
    ctx.render(seeds)
    ctx.aov_clear()
    ctx.render_aovs(seeds)
    say("# r09: device time of moptix_denoise_temporal (csrc/temporalkernel.hip) beside moptix_denoise, python tools/temporal_time.py")
    say("coffee %dx%d, %d spp beauty + AOVs of the same seeds; denoiser and temporal defaults; HIP events, median of %d (min)" % (
        a.width, a.height, a.spp, a.reps))
    out = torch.empty((a.height, a.width, 3), dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    ctx.denoise_bind(out)
    p, t = K.DenoiseParams(), K.TemporalParams()
    assert L.moptix_denoise_defaults(C.byref(p)) == 0 and L.moptix_temporal_defaults(C.byref(t)) == 0

    def cam(k):
        # the same beauty and AOVs every call; only the camera the reprojection sees moves (1e-3 scene units per call: sub-pixel to
        # a few pixels), so every pixel gathers its four taps at fractional positions
        q = K.Params.from_buffer_copy(hs.params)
        for name in ("origin", "scrLowerLeftCorner"):
            v = getattr(q.cam, name)
            setattr(q.cam, name, K.Float3(v.x + 1e-3 * k, v.y + 5e-4 * k, v.z))
        ctx.set_params(q)

    def timed(call, before=None):
        dev = []
        for k in range(a.reps + 1):                                    # the first call warms: code loaded, buffers allocated
            if before:
                before(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()                                                     # blocking
            e1.record(stream)
            e1.synchronize()
            dev.append(e0.elapsed_time(e1))
        return float(np.median(dev[1:])), float(np.min(dev[1:]))

    def spatial():
        assert L.moptix_denoise(ctx._h, C.byref(p), float(a.spp)) == 0, ctx.last_error()

    def temporal():
        assert L.moptix_denoise_temporal(ctx._h, C.byref(p), C.byref(t), float(a.spp)) == 0, ctx.last_error()

    res = {}
    for it in (5, 0):
        p.iterations = it
        res["spatial", it] = timed(spatial)
        res["first", it] = timed(temporal, lambda k: ctx.temporal_reset())
        ctx.temporal_reset()
        res["steady", it] = timed(temporal, cam)
        info = ctx.temporal_info()
        ctx.set_params(hs.params)
        say("L %d: moptix_denoise %.3f ms (%.3f); moptix_denoise_temporal first frame %.3f ms (%.3f), moving camera %.3f ms (%.3f)" % (
            (it,) + res["spatial", it] + res["first", it] + res["steady", it]))
        say("      last moving call: %d geometry pixels, %d with history, %d disoccluded, mean history %.2f" % (
            info["geometry_pixels"], info["history_pixels"], info["disoccluded_pixels"], info["mean_history"]))
    added = res["steady", 5][0] - res["spatial", 5][0]
    say("added by the temporal stage at L = 5: %.3f ms (%.0f %% of the spatial pass, %.3f %% of a 256-spp beauty frame of 311 ms)" % (
        added, 100.0 * added / res["spatial", 5][0], 100.0 * added / 311.0))
    ctx.denoise_bind(None)
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
