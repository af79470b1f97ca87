"""Frustum-query throughput on coffee (csrc/frustumkernel.hip pt_frustumquery) beside the box query on each query's enclosing axis-aligned box
in the same run: what the caller had to do before -- query the world box and filter the list.

    python3 tools/frustum_bench.py [--log2 20] [--reps 4] [--step-timeout 240]

Scene file:coffee, tree built once per step.  Device-resident sets of 2^log2 queries with the apex (beams: the centre) uniform in the scene
box and uniform random orientations: camera-like frusta (half-angles 25 and 15 degrees, near = a tenth of far) with far distances of
1 %, 10 % and 50 % of the box diagonal, and 100:1 beams 10 % of the diagonal long as six planes: four steps.  Every step is a process of
its own, started by this one (which never opens the GPU) under its own time limit; the first step that fails or runs out of time ends the
run.  Per step, timed with HIP events on the context's stream after a warm-up, median, minimum and maximum of --reps runs of
moptix_query_boxes_device on the enclosing boxes of the regions' eight corners (any, count) and of moptix_query_frusta_device (any,
count), with the sums of the counts: the ids the caller no longer has to filter.  Prints the table that profiles/r31_frustum.txt keeps."""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEPS = ("camera:0.01", "camera:0.1", "camera:0.5", "beam:0.1")
TAN_X, TAN_Y = float(np.tan(np.radians(25.0))), float(np.tan(np.radians(15.0)))


def plane(normal, point):
    return np.concatenate([normal, -(normal * point).sum(axis=1, keepdims=True)], axis=1)


def regions(shape, size, centre, rot):
    """(frusta [n, 24] float32, enclosing boxes [n, 6] float32) of n regions at the points `centre` with the frames `rot` (rows w, u, v)."""
    w, u, v = rot[:, 0], rot[:, 1], rot[:, 2]
    if shape == "camera":
        near, far = 0.1 * size, size
        planes = [plane(u + TAN_X * w, centre), plane(-u + TAN_X * w, centre), plane(v + TAN_Y * w, centre), plane(-v + TAN_Y * w, centre),
                  plane(w, centre + near * w), plane(-w, centre + far * w)]
        corners = [centre + t * (w + sx * TAN_X * u + sy * TAN_Y * v) for t in (near, far) for sx in (-1, 1) for sy in (-1, 1)]
    else:
        h = np.array([0.5 * size, 0.005 * size, 0.005 * size])
        planes = []
        for j, a in enumerate((w, u, v)):
            planes += [plane(a, centre - h[j] * a), plane(-a, centre + h[j] * a)]
        corners = [centre + sx * h[0] * w + sy * h[1] * u + sz * h[2] * v for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    corners = np.stack(corners, axis=1)
    lo = np.nextafter(corners.min(axis=1).astype(np.float32), np.float32(-np.inf))
    hi = np.nextafter(corners.max(axis=1).astype(np.float32), np.float32(np.inf))
    return np.ascontiguousarray(np.stack(planes, axis=1).reshape(-1, 24), np.float32), np.ascontiguousarray(np.concatenate([lo, hi], axis=1))


def step(shape, size, log2, reps):
    import torch
    import minimaloptix_amd as M
    from obb_bench import rotations
    from point_bench import H, W, line, point_set
    K = M._capi
    n = 1 << log2
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    diag = float(np.linalg.norm(hs.aabb_max.astype(np.float64) - hs.aabb_min.astype(np.float64)))
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d regions placed uniformly in the scene box; %d CUs; box diagonal %.4g; %s, length %g of it" % (
        info.nTriangles, info.nNodes, info.treeDepth, log2, ctx.get_option("num_cus"), diag, shape, size))
    rng = np.random.default_rng(31)
    centre = point_set(hs, "uniform", n, np.inf)[:, :3].astype(np.float64)
    frusta, boxes = regions(shape, size * diag, centre, rotations(rng, n))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    df, db = torch.from_numpy(frusta).to(dev), torch.from_numpy(boxes).to(dev)
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
    where = "%s, length %g" % (shape, size)
    sums = {}
    for mode, m in (("any", K.BOX_ANY), ("count", K.BOX_COUNT)):
        base = line("pt_boxquery %s on the enclosing boxes, %s" % (mode, where), n, timed(lambda: L.moptix_query_boxes_device(ctx._h, vp(db), n, m, vp(out))), "Mboxes/s")
        sums["box"] = int(out.to(torch.int64).sum())
        med = line("pt_frustumquery %s, %s" % (mode, where), n, timed(lambda: L.moptix_query_frusta_device(ctx._h, vp(df), n, m, vp(out))), "Mfrusta/s")
        sums["frustum"] = int(out.to(torch.int64).sum())
        print("#   %.2fx the enclosing box query; %s: enclosing boxes %d, frusta %d (1 : %.3g)" % (
            med / base, "regions that meet anything" if mode == "any" else "ids", sums["box"], sums["frustum"], sums["box"] / max(sums["frustum"], 1)))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default=None, help="internal: run one step, SHAPE:SIZE")
    a = ap.parse_args()
    if a.step:
        shape, size = a.step.split(":")
        step(shape, float(size), a.log2, a.reps)
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
