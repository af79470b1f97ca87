"""Segment-query throughput on coffee (csrc/segmentkernel.hip pt_segmentquery) beside the closest point query on the segments' midpoints
and the sweep query's "any" on the same motion, in the same run.

    python3 tools/segment_bench.py [--log2 20] [--reps 8] [--step-timeout 240]

Scene file:coffee, tree built once per step.  Device-resident sets of 2^log2 segments each: first ends uniform in the scene box with
uniform directions and a length of 0.1 %, 1 % and 10 % of the box diagonal ("box"), and the mesh's own edges, taken cyclically, displaced
along their face's normal by +-0.1 % and +-1 % of the diagonal ("edges") -- each with maxDist = 1 % of the diagonal and with maxDist = inf:
eight steps.  Every step is a process of its own, started by this one (which never opens the GPU) under its own time limit; the first
step that fails or runs out of time ends the run.
Per step, timed with HIP events on the context's stream after two warm-up runs, median, minimum and maximum of --reps runs of
moptix_query_segments_device in closest and in any mode, of moptix_query_points_device closest on the midpoints with the same maxDist
(the yardstick: the same walk without a length), and -- where maxDist is finite, a sweep's radius has to be -- of
moptix_query_sweeps_device any on (a, b - a, maxDist, 1): "does a sphere of that radius touch anything on its way from a to b", the same
yes or no up to the two contracts' roundings.  No target is set.  Prints the table that profiles/r34_segment.txt keeps."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LENGTHS = (0.001, 0.01, 0.1)
MAXDIST = (0.01, float("inf"))
STEPS = ["box:%g:%g" % (l, m) for m in MAXDIST for l in LENGTHS] + ["edges:0:%g" % m for m in MAXDIST]


def segment_set(hs, name, length, n, seed=43):
    """(a, b) float64 [n, 3] each."""
    rng = np.random.default_rng(seed)
    lo, hi = hs.aabb_min.astype(np.float64), hs.aabb_max.astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    if name == "box":
        a = rng.uniform(lo, hi, (n, 3))
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        return a, a + d * (length * diag)
    t = np.asarray(hs.face_arrays()[0], np.float64).reshape(-1, 3, 3)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    t = t[np.linalg.norm(nrm, axis=1) > 0]
    i = np.arange(n) % len(t)
    k = (np.arange(n) // len(t)) % 3
    nrm = np.cross(t[i, 1] - t[i, 0], t[i, 2] - t[i, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    off = nrm * (diag * np.array([1e-3, -1e-3, 1e-2, -1e-2])[np.arange(n) % 4])[:, None]
    return t[i, k] + off, t[i, (k + 1) % 3] + off


def step(name, length, max_dist, log2, reps):
    import torch
    import minimaloptix_amd as M
    from point_bench import H, W, line
    K = M._capi
    n = 1 << log2
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    diag = float(np.linalg.norm(hs.aabb_max.astype(np.float64) - hs.aabb_min.astype(np.float64)))
    md = np.float32(max_dist * diag)
    what = "the mesh's displaced edges" if name == "edges" else "box, length %g" % length
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d segments; %d CUs; box diagonal %.4g; %s and maxDist %g of it%s" % (
        info.nTriangles, info.nNodes, info.treeDepth, log2, ctx.get_option("num_cus"), diag, what, max_dist,
        "; library %s" % os.environ["MOPTIX_DEVICE_LIB"] if "MOPTIX_DEVICE_LIB" in os.environ else ""))
    a, b = segment_set(hs, name, length, n)
    col = np.full((n, 1), md, np.float64)
    segs = np.ascontiguousarray(np.concatenate([a, b, col, np.zeros((n, 1))], axis=1), np.float32)
    pts = np.ascontiguousarray(np.concatenate([0.5 * (a + b), col], axis=1), np.float32)
    sweeps = np.ascontiguousarray(np.concatenate([segs[:, 0:3], segs[:, 3:6] - segs[:, 0:3], col, np.ones((n, 1))], axis=1), np.float32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    dg, dp, dw = torch.from_numpy(segs).to(dev), torch.from_numpy(pts).to(dev), torch.from_numpy(sweeps).to(dev)
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
    where = "%s, maxDist %g" % (what, max_dist)
    base = line("pt_pointquery closest on the midpoints, %s" % where, n, timed(lambda: L.moptix_query_points_device(ctx._h, vp(dp), n, K.POINT_CLOSEST, vp(recs))))
    point_hits = int((recs.view(torch.int32)[:, 1] >= 0).sum())
    med = line("pt_segmentquery closest, %s" % where, n, timed(lambda: L.moptix_query_segments_device(ctx._h, vp(dg), n, K.SEGMENT_CLOSEST, vp(recs))), "Msegments/s")
    prim, dist = recs.view(torch.int32)[:, 1], recs[:, 0]
    print("#   %.2fx the closest point query; within maxDist %d (the midpoints %d), of them at distance 0 %d" % (
        med / base, int((prim >= 0).sum()), point_hits, int(((prim >= 0) & (dist == 0)).sum())))
    med = line("pt_segmentquery any, %s" % where, n, timed(lambda: L.moptix_query_segments_device(ctx._h, vp(dg), n, K.SEGMENT_ANY, vp(out))), "Msegments/s")
    print("#   %.2fx the closest point query; segments with anything within maxDist: %d" % (med / base, int(out.sum())))
    if np.isfinite(md):
        med = line("pt_sweepquery any on (a, b - a, maxDist, 1), %s" % where, n, timed(lambda: L.moptix_query_sweeps_device(ctx._h, vp(dw), n, K.SWEEP_ANY, vp(out))), "Msweeps/s")
        print("#   %.2fx the closest point query; sweeps that touch anything: %d" % (med / base, int(out.sum())))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--steps", default=",".join(STEPS), help="comma-separated SET:LENGTH:MAXDIST, in shares of the box diagonal")
    ap.add_argument("--step", default=None, help="internal: run one step, SET:LENGTH:MAXDIST")
    a = ap.parse_args()
    if a.step:
        name, length, max_dist = a.step.split(":")
        step(name, float(length), float(max_dist), a.log2, a.reps)
        return 0
    for s in a.steps.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", s, "--log2", str(a.log2), "--reps", str(a.reps)]
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
