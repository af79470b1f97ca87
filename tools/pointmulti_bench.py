"""K-nearest point-query throughput on coffee (csrc/pointkernel.hip pt_pointquery_multi) beside the closest point query on the same points in
the same run.

    python3 tools/pointmulti_bench.py [--log2 20] [--reps 8]

Scene file:coffee, tree built once; the device-resident point sets of tools/point_bench.py (uniform in the box; within 1 % of the diagonal
of the surface), 2^log2 points each, with maxDist = inf and with maxDist = 1 % of the box diagonal (the records of maxNear 16 take 512
bytes per point).  Timed with HIP events on the context's stream after a warm-up: median, minimum and maximum of --reps runs of
moptix_query_points_device (closest: the yardstick, the kernel that was there before) and of moptix_query_points_multi_device with maxNear
1, 4, 16 on all four sets, and with MOPTIX_POINT_MULTI_COUNT_ALL at maxNear 0 and 4 on the two sets with a limit -- without one the count is
the number of primitives and the walk a loop over all of them.  Prints the table that profiles/r23_pointmulti.txt keeps."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minimaloptix_amd as M          # noqa: E402
from point_bench import H, W, line, point_set      # noqa: E402

K = M._capi
CASES = ((1, 0, "maxNear 1"), (4, 0, "maxNear 4"), (16, 0, "maxNear 16"))
COUNTING = ((0, K.POINT_MULTI_COUNT_ALL, "maxNear 0, COUNT_ALL"), (4, K.POINT_MULTI_COUNT_ALL, "maxNear 4, COUNT_ALL"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=8)
    a = ap.parse_args()
    n = 1 << a.log2

    import torch
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    diag = float(np.linalg.norm(hs.aabb_max.astype(np.float64) - hs.aabb_min.astype(np.float64)))
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d points per set; %d CUs; box diagonal %.4g" % (
        info.nTriangles, info.nNodes, info.treeDepth, a.log2, ctx.get_option("num_cus"), diag))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    hits = torch.empty((n, 16, 8), dtype=torch.float32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)

    def timed(launch):
        ms = []
        for i in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = launch()
            assert rc == K.MOPTIX_OK, ctx.last_error()
            e1.record(stream)
            stream.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms

    for name in ("uniform", "near"):
        for limit, max_dist in (("no limit", np.inf), ("maxDist 1 %", 0.01 * diag)):
            pts = torch.from_numpy(point_set(hs, name, n, max_dist)).to(dev)
            torch.cuda.synchronize()
            pp, hp, cp = C.c_void_p(pts.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(counts.data_ptr())
            where = "%s, %s" % (name, limit)
            base = line("pt_pointquery closest, %s" % where, n, timed(lambda: L.moptix_query_points_device(ctx._h, pp, n, K.POINT_CLOSEST, hp)))
            for k, flags, label in CASES + (COUNTING if np.isfinite(max_dist) else ()):
                med = line("pt_pointquery_multi %s, %s" % (label, where), n,
                           timed(lambda: L.moptix_query_points_multi_device(ctx._h, pp, n, k, flags, hp if k else None, cp)))
                c = counts.to(torch.int64)
                print("#   %.2fx the closest query; counts: sum %d, max %d, points with any %d" % (med / base, int(c.sum()), int(c.max()), int((c > 0).sum())))
    ctx.close()


if __name__ == "__main__":
    main()
