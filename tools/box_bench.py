"""Box-query throughput on coffee (csrc/boxkernel.hip pt_boxquery) beside the closest point query on the boxes' centres in the same run.

    python3 tools/box_bench.py [--log2 20] [--reps 8] [--step-timeout 240]

Scene file:coffee, tree built once per step.  Two device-resident box sets of 2^log2 cubes each -- centred uniformly in the scene box, and
centred on random surface points -- at cell edges of 0.1 %, 1 % and 10 % of the box diagonal: six steps.  Every step is a process of its own,
started by this one (which never opens the GPU) under its own time limit; the first step that fails or runs out of time ends the run.
Per step, timed with HIP events on the context's stream after a warm-up, median, minimum and maximum of --reps runs of
moptix_query_points_device (closest, maxDist = inf, on the centres: the yardstick, a kernel that was there before) and of
moptix_query_boxes_device in any and in count mode; then the two-pass list of Context.query_boxes (count, cumulative sum, fill; blocking,
wall clock, allocation of the result included) on the first m boxes, m the largest power of two whose lists hold at most 2^27 ids together.
Prints the table that profiles/r26_box.txt keeps."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

EDGES = (0.001, 0.01, 0.1)
SETS = ("uniform", "surface")
LIST_IDS = 1 << 27


def step(name, edge, log2, reps):
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
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d boxes; %d CUs; box diagonal %.4g; set %s, cell edge %g of it" % (
        info.nTriangles, info.nNodes, info.treeDepth, log2, ctx.get_option("num_cus"), diag, name, edge))
    pts = point_set(hs, "uniform", n, np.inf)
    if name == "surface":
        pts = point_set(hs, "near", n, np.inf)      # within 1 % of the diagonal of the surface ...
        rng = np.random.default_rng(23)
        tri = hs.face_arrays()[0].astype(np.float64).reshape(-1, 3, 3)[rng.integers(0, len(hs.face_arrays()[0]), n)]
        w = rng.dirichlet((1.0, 1.0, 1.0), n)
        pts[:, :3] = (w[:, :, None] * tri).sum(axis=1).astype(np.float32)      # ... replaced by points on it
    half = np.float32(0.5 * edge * diag)
    boxes = np.ascontiguousarray(np.concatenate([pts[:, :3] - half, pts[:, :3] + half], axis=1), np.float32)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    dp, db = torch.from_numpy(pts).to(dev), torch.from_numpy(boxes).to(dev)
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
    where = "%s, edge %g" % (name, edge)
    base = line("pt_pointquery closest on the centres, %s" % where, n, timed(lambda: L.moptix_query_points_device(ctx._h, vp(dp), n, K.POINT_CLOSEST, vp(recs))))
    med = line("pt_boxquery any, %s" % where, n, timed(lambda: L.moptix_query_boxes_device(ctx._h, vp(db), n, K.BOX_ANY, vp(out))), "Mboxes/s")
    print("#   %.2fx the closest query; boxes that meet anything: %d" % (med / base, int(out.sum())))
    med = line("pt_boxquery count, %s" % where, n, timed(lambda: L.moptix_query_boxes_device(ctx._h, vp(db), n, K.BOX_COUNT, vp(out))), "Mboxes/s")
    c = out.to(torch.int64)
    print("#   %.2fx the closest query; counts: sum %d, max %d, mean of the non-empty %.1f" % (
        med / base, int(c.sum()), int(c.max()), float(c.sum()) / max(1, int((c > 0).sum()))))
    m = n
    while m > 1 and int(c[:m].sum()) > LIST_IDS:
        m //= 2
    sub = db[:m].contiguous()
    ms = []
    for i in range(min(reps, 4) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prims, offsets = ctx.query_boxes(sub, "list")
        if i >= 1:
            ms.append((time.perf_counter() - t0) * 1e3)
    line("two-pass list of the first %d boxes, %s" % (m, where), m, ms, "Mboxes/s")
    print("#   %d ids; wall clock of Context.query_boxes, blocking" % int(offsets[-1]))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default=None, help="internal: run one step, SET:EDGE")
    a = ap.parse_args()
    if a.step:
        name, edge = a.step.split(":")
        step(name, float(edge), a.log2, a.reps)
        return 0
    for name in SETS:
        for edge in EDGES:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", "%s:%g" % (name, edge), "--log2", str(a.log2), "--reps", str(a.reps)]
            try:
                rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
            except subprocess.TimeoutExpired:
                print("# step %s:%g ran out of its %d s: the run ends here" % (name, edge, a.step_timeout), flush=True)
                return 124
            if rc != 0:
                print("# step %s:%g ended with status %d: the run ends here" % (name, edge, rc), flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
