"""Oriented-box-query throughput on coffee (csrc/obbkernel.hip pt_obbquery) beside the box query on each query's enclosing axis-aligned box
in the same run: what the caller had to do before -- query the world box and filter the list.

    python3 tools/obb_bench.py [--log2 20] [--reps 4] [--step-timeout 240]

Scene file:coffee, tree built once per step.  Device-resident sets of 2^log2 oriented boxes centred uniformly in the scene box with uniform
random rotations: cubes with edges of 0.1 %, 1 % and 10 % of the box diagonal, and 100:1 beams 10 % of the diagonal long: four steps.
Every step is a process of its own, started by this one (which never opens the GPU) under its own time limit; the first step that fails
or runs out of time ends the run.  Per step, timed with HIP events on the context's stream after a warm-up, median, minimum and maximum of
--reps runs of moptix_query_boxes_device on the enclosing boxes c -+ E (any, count) and of moptix_query_obbs_device (any, count), with the
sums of the counts: the ids the caller no longer has to filter.  Prints the table that profiles/r30_obb.txt keeps."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEPS = ("cube:0.001", "cube:0.01", "cube:0.1", "beam:0.1")


def rotations(rng, n):
    """n rotation matrices uniform over SO(3), from unit quaternions; local-to-world."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def step(shape, edge, log2, reps):
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
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d oriented boxes centred uniformly in the scene box; %d CUs; box diagonal %.4g; %s, longest edge %g of it" % (
        info.nTriangles, info.nNodes, info.treeDepth, log2, ctx.get_option("num_cus"), diag, shape, edge))
    rng = np.random.default_rng(30)
    centre = point_set(hs, "uniform", n, np.inf)[:, :3]
    half = np.full(3, 0.5 * edge * diag) * (np.array([1.0, 0.01, 0.01]) if shape == "beam" else 1.0)
    obbs = M.oriented_boxes(centre, half, rotations(rng, n))
    e = np.einsum("njk,j->nk", np.abs(obbs[:, 6:15].reshape(n, 3, 3).astype(np.float64)), half)
    boxes = np.ascontiguousarray(np.concatenate([centre - e, centre + e], axis=1), np.float32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    do, db = torch.from_numpy(obbs).to(dev), torch.from_numpy(boxes).to(dev)
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
    where = "%s, edge %g" % (shape, edge)
    sums = {}
    for mode, m in (("any", K.BOX_ANY), ("count", K.BOX_COUNT)):
        base = line("pt_boxquery %s on the enclosing boxes, %s" % (mode, where), n, timed(lambda: L.moptix_query_boxes_device(ctx._h, vp(db), n, m, vp(out))), "Mboxes/s")
        sums["box"] = int(out.to(torch.int64).sum())
        med = line("pt_obbquery %s, %s" % (mode, where), n, timed(lambda: L.moptix_query_obbs_device(ctx._h, vp(do), n, m, vp(out))), "Mboxes/s")
        sums["obb"] = int(out.to(torch.int64).sum())
        print("#   %.2fx the enclosing box query; %s: enclosing boxes %d, oriented boxes %d" % (
            med / base, "boxes that meet anything" if mode == "any" else "ids", sums["box"], sums["obb"]))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default=None, help="internal: run one step, SHAPE:EDGE")
    a = ap.parse_args()
    if a.step:
        shape, edge = a.step.split(":")
        step(shape, float(edge), a.log2, a.reps)
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
