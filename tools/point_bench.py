"""Point-query throughput on coffee (csrc/pointkernel.hip), with the ray queries' closest-hit time for the same count beside it for scale.

    python3 tools/point_bench.py [--log2 20] [--reps 12] [--sweep] [--signed]

Scene file:coffee, tree built once.  Two device-resident point sets of 2^log2 points each:
  uniform   uniform in the scene box, maxDist = inf: every walk has to find the surface from wherever it starts
  near      random surface points, each moved along a random direction by up to 1 % of the box diagonal; maxDist = inf
Timed with HIP events on the context's stream (a torch stream handed to moptix_set_stream), after a warm-up: median, minimum and maximum
of --reps runs of moptix_query_points_device in closest and in any mode ("any" with maxDist = 1 % of the diagonal: with no limit it ends at
the first primitive of the first leaf).  Then moptix_query_rays_device, closest, on as many incoherent rays (tools/query_bench.py's set).
--sweep adds the grid's cap ("query_blocks_per_cu") and the 128-byte nodes.  Prints the table that profiles/r16_point.txt keeps.
--signed adds the signed mode (its table: csrc/signkernel.hip) on the same two point sets beside the closest mode, with their ratio, and the rebuild of
the sign table after a refit: a signed query of 256 points with the table stale (moptix_update_faces + moptix_refit_accel before each run)
against the same query with the table current, beside the refit's own refitMs (profiles/r17_sign.txt)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import minimaloptix_amd as M          # noqa: E402
from query_bench import ray_set       # noqa: E402

K = M._capi
W, H = 1920, 1080


def point_set(hs, name, n, max_dist):
    rng = np.random.default_rng(21 if name == "uniform" else 22)
    lo, hi = hs.aabb_min.astype(np.float64), hs.aabb_max.astype(np.float64)
    if name == "uniform":
        p = rng.uniform(lo, hi, (n, 3))
    else:
        tri = hs.face_arrays()[0].astype(np.float64).reshape(-1, 3, 3)[rng.integers(0, len(hs.face_arrays()[0]), n)]
        a, b = rng.uniform(size=n), rng.uniform(size=n)
        flip = a + b > 1
        a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        p = tri[:, 0] + a[:, None] * (tri[:, 1] - tri[:, 0]) + b[:, None] * (tri[:, 2] - tri[:, 0])
        p = p + d * (0.01 * np.linalg.norm(hi - lo) * rng.uniform(size=(n, 1)))
    return np.ascontiguousarray(np.concatenate([p.astype(np.float32), np.full((n, 1), max_dist, np.float32)], axis=1))


def line(label, n, ms, unit="Mpoints/s"):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    print("%-52s %8.3f ms  [%7.3f .. %7.3f]  %8.1f %s  (%d runs)" % (label, med, ms[0], ms[-1], n / med * 1e-3, unit, len(ms)))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--signed", action="store_true")
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
    recs = torch.empty((n, 8), dtype=torch.float32, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)

    def timed(fn, buf, mode, out):
        ms = []
        for i in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = fn(ctx._h, C.c_void_p(buf.data_ptr()), n, mode, C.c_void_p(out.data_ptr()))
            assert rc == K.MOPTIX_OK, ctx.last_error()
            e1.record(stream)
            stream.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms

    sets = {}
    for name in ("uniform", "near"):
        sets[name] = torch.from_numpy(point_set(hs, name, n, np.inf)).to(dev)
        sets[name + ", maxDist 1 %"] = torch.from_numpy(point_set(hs, name, n, 0.01 * diag)).to(dev)
    torch.cuda.synchronize()
    for name in ("uniform", "near"):
        line("pt_pointquery closest, %s, no limit" % name, n, timed(L.moptix_query_points_device, sets[name], K.POINT_CLOSEST, recs))
        dist = recs[:, 0]
        print("#   mean distance %.4g (%.3g of the diagonal)" % (float(dist.mean()), float(dist.mean()) / diag))
        lim = sets[name + ", maxDist 1 %"]
        line("pt_pointquery closest, %s, maxDist 1 %%" % name, n, timed(L.moptix_query_points_device, lim, K.POINT_CLOSEST, recs))
        line("pt_pointquery any, %s, maxDist 1 %%" % name, n, timed(L.moptix_query_points_device, lim, K.POINT_ANY, flags))
        print("#   within 1 %% of the diagonal: %d of %d" % (int(flags.sum()), n))
        line("pt_pointquery any, %s, no limit" % name, n, timed(L.moptix_query_points_device, sets[name], K.POINT_ANY, flags))
    if a.sweep:
        for name in ("uniform", "near"):
            for val in (1, 4, 16, 32, 64):
                ctx.set_option("query_blocks_per_cu", val)
                line("  query_blocks_per_cu=%d closest, %s" % (val, name), n, timed(L.moptix_query_points_device, sets[name], K.POINT_CLOSEST, recs))
            ctx.set_option("query_blocks_per_cu", 32)
            ctx.set_option("node_format", 128)
            line("  node_format=128 closest, %s" % name, n, timed(L.moptix_query_points_device, sets[name], K.POINT_CLOSEST, recs))
            ctx.set_option("node_format", 0)
    if a.signed:
        print("# sign_info: %s" % ctx.sign_info())
        for name in ("uniform", "near"):
            closest = line("pt_pointquery closest, %s, no limit" % name, n, timed(L.moptix_query_points_device, sets[name], K.POINT_CLOSEST, recs))
            signed = line("pt_pointquery signed, %s, no limit" % name, n, timed(L.moptix_query_points_device, sets[name], K.POINT_SIGNED, recs))
            print("#   signed / closest %.3f; inside: %d of %d" % (signed / closest, int((recs[:, 0] < 0).sum()), n))
        fp = hs.face_arrays()[0]
        ext = float((hs.aabb_max - hs.aabb_min).max())
        p3 = fp.reshape(-1, 3)
        rows = (p3 + np.float32(0.01 * ext) * np.sin(7.0 * p3[:, [1, 2, 0]].astype(np.float64) + 0.3).astype(np.float32)).astype(np.float32).reshape(-1, 9)
        small = sets["uniform"][:256].contiguous()
        stale, current, refit = [], [], []
        for i in range(a.reps + 2):
            ctx.update_faces(0, rows if i % 2 == 0 else fp)
            refit.append(ctx.refit_accel()["refitMs"])
            for ms in (stale, current):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                rc = L.moptix_query_points_device(ctx._h, C.c_void_p(small.data_ptr()), 256, K.POINT_SIGNED, C.c_void_p(recs.data_ptr()))
                assert rc == K.MOPTIX_OK, ctx.last_error()
                e1.record(stream)
                stream.synchronize()
                if i >= 2:
                    ms.append(e0.elapsed_time(e1))
        refit = sorted(refit[2:])
        t_stale = line("signed query of 256 points, table stale (rebuilt first)", 256, stale)
        t_cur = line("signed query of 256 points, table current", 256, current)
        print("#   table rebuild %.3f ms beside refitMs %.3f ms (median): %.3f of the refit; tableBuilds %d" % (
            t_stale - t_cur, refit[len(refit) // 2], (t_stale - t_cur) / refit[len(refit) // 2], ctx.sign_info()["tableBuilds"]))
        ctx.update_faces(0, fp); ctx.refit_accel()
    rays = torch.from_numpy(ray_set(hs, "incoherent", n)).to(dev)
    torch.cuda.synchronize()
    line("for scale: pt_rayquery closest, incoherent rays", n, timed(L.moptix_query_rays_device, rays, K.QUERY_CLOSEST, recs), "Mrays/s")
    ctx.close()


if __name__ == "__main__":
    main()
