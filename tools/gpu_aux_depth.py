"""The benchmark frame under option "aux_depth" values, warm and as a context's first frame.

    [MOPTIX_DEVICE_LIB=lib.so] [AUX=0,16] [RUNS=4] [SPP=256] python3 tools/gpu_aux_depth.py

Does what bench.py's step does (clear the bound accumulation buffer, one blocking render of the frame's seeds: coffee 1920x1080) and
reports, per "aux_depth" value, the trace-kernel ms (HIP events on the launch stream) and the wall ms of RUNS warm frames and RUNS first
frames ("forget_history": no depth history orders the work), the values alternated run by run.  Prints which packet build ran
("kernel_slim_used", where the library has the option) and the hash of the last frame."""
import hashlib
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
from common import M   # noqa: E402

W, H = 1920, 1080
values = [int(v) for v in os.environ.get("AUX", "0,16").split(",")]
runs = int(os.environ.get("RUNS", "4"))
seeds = M.launch_seeds(int(os.environ.get("SPP", "256")))
ctx = M.Context(0)
ctx.load(M.HostScene("file:coffee", W, H))


def frame(aux, first):
    ctx.set_option("aux_depth", aux)
    if first:
        ctx.set_option("forget_history", 1)
    ctx.accum_clear(); ctx.kernel_time(reset=True)
    t0 = time.perf_counter(); ctx.render(seeds); wall = (time.perf_counter() - t0) * 1e3
    return ctx.kernel_time()[0], wall


def slim():
    try:
        return ctx.get_option("kernel_slim_used")
    except M.MoptixError:
        return -1


frame(values[0], False); frame(values[0], False)      # code objects loaded, a depth history in place
out = {(a, f): [] for a in values for f in (False, True)}
for first in (False, True):
    for r in range(runs):
        for a in values:
            if not first:
                frame(a, False)                     # the history this value's own frames leave
            out[(a, first)].append(frame(a, first))
    if first:
        frame(values[0], False)
for (a, first), v in sorted(out.items()):
    k = sorted(x[0] for x in v)
    print("aux_depth %-3d %-5s kernel ms %s  median %.3f spread %.3f | wall ms %s" % (
        a, "first" if first else "warm", " ".join("%.3f" % x[0] for x in v), (k[(len(k) - 1) // 2] + k[len(k) // 2]) / 2, k[-1] - k[0],
        " ".join("%.3f" % x[1] for x in v)), flush=True)
for a in values:
    frame(a, False)
    print("aux_depth %-3d variant %d features %d slim %d hash %s" % (a, ctx.get_option("kernel_variant_used"), ctx.get_option("kernel_features_used"), slim(),
                                                                  hashlib.md5(ctx.accum_read().tobytes()).hexdigest()[:10]), flush=True)
