"""Winding-number query throughput on coffee (csrc/windingkernel.hip pt_windingquery) beside the closest point query on the same points in
the same run, the exact sum on a smaller set, and the moments pass alone beside a refit.

    python3 tools/winding_bench.py [--log2 20] [--log2-exact 12] [--reps 8] [--step-timeout 300]

Scene file:coffee, tree built once per step.  A device-resident set of 2^log2 points uniform in the scene box (tools/point_bench.py's
"uniform" set).  Every step is a process of its own, started by this one (which never opens the GPU) under its own time limit; the
first step that fails or runs out of time ends the run.  Timed with HIP events on the context's stream after two warm-up runs: median,
minimum and maximum of --reps runs.
  step "walk"   moptix_query_points_device closest (maxDist = inf), then moptix_query_winding_device at beta 2, 3 and 4, with the share of
                points classified inside (w > 0.5) and the largest |w(beta) - w(4)|; then beta = +inf on the first 2^log2-exact points,
                with the largest |w(beta) - w(inf)| on those: what the expansion saves and what it costs.
  step "table"  the moments pass alone: a refit over unchanged positions makes the table stale; the first query on one point after it (pass
                + walk) minus the second (walk alone), beside refitMs of that refit.
Prints the table that profiles/r32_winding.txt keeps."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEPS = ("walk", "table")
BETAS = (2.0, 3.0, 4.0)


def _timed(torch, stream, K, ctx, launch, reps, warm=2):
    ms = []
    for i in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        rc = launch()
        assert rc == K.MOPTIX_OK, ctx.last_error()
        e1.record(stream)
        stream.synchronize()
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return ms


def step(name, log2, log2_exact, reps):
    import torch
    import minimaloptix_amd as M
    from point_bench import H, W, line, point_set
    K = M._capi
    n, ne = 1 << log2, 1 << min(log2, log2_exact)
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d points uniform in the scene box; %d CUs" % (
        info.nTriangles, info.nNodes, info.treeDepth, log2, ctx.get_option("num_cus")))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    vp = lambda t: C.c_void_p(t.data_ptr())
    pts = point_set(hs, "uniform", n, np.inf)
    if name == "table":
        one = torch.from_numpy(pts[:1].copy()).to(dev); one[:, 3] = 2.0
        o1 = torch.empty(1, dtype=torch.float32, device=dev)
        assert L.moptix_query_winding_device(ctx._h, vp(one), 1, vp(o1)) == K.MOPTIX_OK      # plan, table, overflow area
        stream.synchronize()
        first, second, refit = [], [], []
        for i in range(reps + 2):
            ctx.refit_accel()                                      # unchanged positions: the same words, and a stale table
            assert ctx.winding_info()["stale"] == 1
            t = _timed(torch, stream, K, ctx, lambda: L.moptix_query_winding_device(ctx._h, vp(one), 1, vp(o1)), 2, warm=0)
            if i >= 2:
                first.append(t[0]); second.append(t[1]); refit.append(ctx.refit_info()["refitMs"])
        line("first query on 1 point after a refit (pass + walk)", 1, first, "Mpoints/s")
        line("second query on 1 point (walk alone)", 1, second, "Mpoints/s")
        line("refit_accel, refitMs", 1, refit, "Mrefits/s")
        wi = ctx.winding_info()
        print("#   the moments pass: %.3f ms (median first - median second); table %d bytes for %d nodes; %d levels = launches" % (
            sorted(first)[len(first) // 2] - sorted(second)[len(second) // 2], wi["tableBytes"], wi["nodes"], info.treeDepth))
        ctx.close()
        return
    dp = torch.from_numpy(pts).to(dev)
    hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    base = line("pt_pointquery closest, maxDist inf", n, _timed(torch, stream, K, ctx, lambda: L.moptix_query_points_device(ctx._h, vp(dp), n, K.POINT_CLOSEST, vp(hits)), reps))
    w = {}
    for beta in BETAS:
        dp[:, 3] = beta
        torch.cuda.synchronize()
        med = line("pt_windingquery beta %g" % beta, n, _timed(torch, stream, K, ctx, lambda: L.moptix_query_winding_device(ctx._h, vp(dp), n, vp(out)), reps))
        w[beta] = out.clone()
        print("#   %.2fx the closest point query; inside (w > 0.5): %.4f of the points; w in %.3f .. %.3f" % (
            med / base, float((w[beta] > 0.5).float().mean()), float(w[beta].min()), float(w[beta].max())))
    for beta in BETAS[:-1]:
        print("#   max |w(%g) - w(4)| = %.4g; classified differently: %d of %d" % (
            beta, float((w[beta] - w[4.0]).abs().max()), int(((w[beta] > 0.5) != (w[4.0] > 0.5)).sum()), n))
    de = dp[:ne].clone(); de[:, 3] = float("inf")
    oe = torch.empty(ne, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    med = line("pt_windingquery beta inf (every triangle)", ne, _timed(torch, stream, K, ctx, lambda: L.moptix_query_winding_device(ctx._h, vp(de), ne, vp(oe)), max(2, reps // 4)))
    for beta in BETAS:
        d = (w[beta][:ne] - oe).abs()
        print("#   max |w(%g) - w(inf)| on these 2^%d points = %.4g (mean %.3g); classified differently: %d" % (
            beta, min(log2, log2_exact), float(d.max()), float(d.mean()), int(((w[beta][:ne] > 0.5) != (oe > 0.5)).sum())))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--log2-exact", type=int, default=12)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", default=None, help="internal: run one step")
    a = ap.parse_args()
    if a.step:
        step(a.step, a.log2, a.log2_exact, a.reps)
        return 0
    for s in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--log2", str(a.log2), "--log2-exact", str(a.log2_exact), "--reps", str(a.reps)]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print("# step %s ran out of its %d s: the run ends here" % (s, a.step_timeout), flush=True)
            return 124
        if rc != 0:
            print("# step %s ended with status %d: the run ends here" % (s, rc), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
