"""Triangle-query throughput on coffee (csrc/trikernel.hip pt_triquery) beside the box query on each query's bounding box in the same run:
what the caller had to do before -- query the triangle's box and run a narrow phase on the list.

    python3 tools/tri_bench.py [--log2 20] [--reps 4] [--step-timeout 240]

Scene file:coffee, tree built once per step.  Device-resident sets of 2^log2 query triangles of three kinds: the mesh's own faces (drawn
with replacement) displaced along a random direction by 0.1 %, 1 % and 10 % of the box diagonal; random triangles of those sizes (vertices
= a centre uniform in the scene box + size x a standard normal); and 100:1 slivers 10 % of the diagonal long with uniform random
orientations: seven steps.  Every step is a process of its own, started by this one (which never opens the GPU) under its own time limit;
the first step that fails or runs out of time ends the run.  Per step, timed with HIP events on the context's stream after a warm-up,
median, minimum and maximum of --reps runs of moptix_query_boxes_device on the queries' bounding boxes (any, count) and of
moptix_query_tris_device (any, count), with the sums of the counts: the ids the caller no longer has to filter.  Prints the table that
profiles/r33_tri.txt keeps."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEPS = ("faces:0.001", "faces:0.01", "faces:0.1", "random:0.001", "random:0.01", "random:0.1", "sliver:0.1")


def directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def step(kind, size, log2, reps):
    import torch
    import minimaloptix_amd as M
    from point_bench import H, W, line, point_set
    K = M._capi
    n = 1 << log2
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    diag = float(np.linalg.norm(hs.aabb_max.astype(np.float64) - hs.aabb_min.astype(np.float64)))
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d query triangles; %d CUs; box diagonal %.4g; %s, %g of it" % (
        info.nTriangles, info.nNodes, info.treeDepth, log2, ctx.get_option("num_cus"), diag, kind, size))
    rng = np.random.default_rng(33)
    if kind == "faces":
        faces = np.asarray(hs.face_arrays()[0], np.float64).reshape(-1, 3, 3)
        t = faces[rng.integers(0, len(faces), n)] + (size * diag) * directions(rng, n)[:, None, :]
    elif kind == "random":
        t = point_set(hs, "uniform", n, np.inf)[:, None, :3].astype(np.float64) + (size * diag) * rng.normal(size=(n, 3, 3))
    else:
        c, a, b = point_set(hs, "uniform", n, np.inf)[:, :3].astype(np.float64), directions(rng, n), directions(rng, n)
        b = np.cross(a, b); b /= np.linalg.norm(b, axis=1, keepdims=True)
        ln = size * diag
        t = np.stack([c - 0.5 * ln * a, c + 0.5 * ln * a, c + 0.01 * ln * b], axis=1)
    tris = np.ascontiguousarray(t.reshape(n, 9), np.float32)
    t32 = tris.reshape(n, 3, 3)
    boxes = np.ascontiguousarray(np.concatenate([t32.min(axis=1), t32.max(axis=1)], axis=1), np.float32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    dt, db = torch.from_numpy(tris).to(dev), torch.from_numpy(boxes).to(dev)
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
    where = "%s, %g" % (kind, size)
    sums = {}
    for mode, m in (("any", K.BOX_ANY), ("count", K.BOX_COUNT)):
        base = line("pt_boxquery %s on the bounding boxes, %s" % (mode, where), n, timed(lambda: L.moptix_query_boxes_device(ctx._h, vp(db), n, m, vp(out))), "Mqueries/s")
        sums["box"] = int(out.to(torch.int64).sum())
        med = line("pt_triquery %s, %s" % (mode, where), n, timed(lambda: L.moptix_query_tris_device(ctx._h, vp(dt), n, m, vp(out))), "Mqueries/s")
        sums["tri"] = int(out.to(torch.int64).sum())
        print("#   %.2fx the bounding box query; %s: bounding boxes %d, triangles %d (%.4f of them)" % (
            med / base, "queries that meet anything" if mode == "any" else "ids", sums["box"], sums["tri"], sums["tri"] / max(sums["box"], 1)))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default=None, help="internal: run one step, KIND:SIZE")
    a = ap.parse_args()
    if a.step:
        kind, size = a.step.split(":")
        step(kind, float(size), a.log2, a.reps)
        return 0
    for s in STEPS:
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
