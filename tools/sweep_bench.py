"""Sweep-query throughput on coffee (csrc/sweepkernel.hip pt_sweepquery) beside the closest ray query on the same rays and the closest
point query on their origins, in the same run.

    python3 tools/sweep_bench.py [--log2 20] [--reps 8] [--step-timeout 240]

Scene file:coffee, tree built once per step.  Two device-resident ray sets of 2^log2 rays each (tools/query_bench.py ray_set) -- the pinhole
rays of a 1920x1080 frame ("primary") and uniform origins in the scene box with uniform directions ("box"), unit directions, tmax 1e27 -- swept
with radii of 0.1 %, 1 % and 10 % of the box diagonal: six steps.  Every step is a process of its own, started by this one (which never opens
the GPU) under its own time limit; the first step that fails or runs out of time ends the run.
Per step, timed with HIP events on the context's stream after a warm-up, median, minimum and maximum of --reps runs of
moptix_query_rays_device closest (the yardstick: the same rays without a radius), of moptix_query_points_device closest on the origins
(maxDist = inf) and of moptix_query_sweeps_device in closest and in any mode.  No target is set: the ratios to the ray query are the result.
Prints the table that profiles/r28_sweep.txt keeps."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RADII = (0.001, 0.01, 0.1)
SETS = ("box", "primary")


def step(name, radius, log2, reps):
    import torch
    import minimaloptix_amd as M
    from point_bench import H, W, line
    from query_bench import ray_set
    K = M._capi
    n = 1 << log2
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    diag = float(np.linalg.norm(hs.aabb_max.astype(np.float64) - hs.aabb_min.astype(np.float64)))
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d sweeps; %d CUs; box diagonal %.4g; set %s, radius %g of it" % (
        info.nTriangles, info.nNodes, info.treeDepth, log2, ctx.get_option("num_cus"), diag, name, radius))
    rays = ray_set(hs, name, n)
    sweeps = rays.copy()
    sweeps[:, 6] = np.float32(radius * diag)
    pts = np.ascontiguousarray(np.concatenate([rays[:, :3], np.full((n, 1), np.inf, np.float32)], axis=1))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    dr, ds, dp = torch.from_numpy(rays).to(dev), torch.from_numpy(sweeps).to(dev), torch.from_numpy(pts).to(dev)
    recs = torch.empty((n, 8), dtype=torch.float32, device=dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def timed(launch):
        ms = []
        for i in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = launch()
            assert rc == K.MOPTIX_OK, ctx.last_error()
            e1.record(stream)
            stream.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms

    vp = lambda t: C.c_void_p(t.data_ptr())
    where = "%s, radius %g" % (name, radius)
    base = line("pt_rayquery closest, %s rays" % name, n, timed(lambda: L.moptix_query_rays_device(ctx._h, vp(dr), n, K.QUERY_CLOSEST, vp(recs))), "Mrays/s")
    ray_hits = int((recs.view(torch.int32)[:, 1] >= 0).sum())
    line("pt_pointquery closest on the origins, %s" % name, n, timed(lambda: L.moptix_query_points_device(ctx._h, vp(dp), n, K.POINT_CLOSEST, vp(recs))))
    med = line("pt_sweepquery closest, %s" % where, n, timed(lambda: L.moptix_query_sweeps_device(ctx._h, vp(ds), n, K.SWEEP_CLOSEST, vp(recs))), "Msweeps/s")
    prim, t = recs.view(torch.int32)[:, 1], recs[:, 0]
    print("#   %.2fx the closest ray query; contacts %d (the rays hit %d), of them starts in contact %d" % (
        med / base, int((prim >= 0).sum()), ray_hits, int(((prim >= 0) & (t == 0)).sum())))
    med = line("pt_sweepquery any, %s" % where, n, timed(lambda: L.moptix_query_sweeps_device(ctx._h, vp(ds), n, K.SWEEP_ANY, vp(out))), "Msweeps/s")
    print("#   %.2fx the closest ray query; sweeps that touch anything: %d" % (med / base, int(out.sum())))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default=None, help="internal: run one step, SET:RADIUS")
    a = ap.parse_args()
    if a.step:
        name, radius = a.step.split(":")
        step(name, float(radius), a.log2, a.reps)
        return 0
    for name in SETS:
        for radius in RADII:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%g" % (name, radius), "--log2", str(a.log2), "--reps", str(a.reps)]
            try:
                rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
            except subprocess.TimeoutExpired:
                print("# step %s:%g ran out of its %d s: the run ends here" % (name, radius, a.step_timeout), flush=True)
                return 124
            if rc != 0:
                print("# step %s:%g ended with status %d: the run ends here" % (name, radius, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
