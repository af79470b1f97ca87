"""Multi-hit ray-query throughput on coffee (csrc/querykernel.hip pt_rayquery_multi) beside the closest query on the same rays in the same run.

    python3 tools/multihit_bench.py [--log2 20] [--reps 12]

Scene file:coffee, tree built once; the two device-resident ray sets of tools/query_bench.py (primary, incoherent), 2^log2 rays each (the
records of maxHits 16 take 512 bytes per ray: 2^20 rays by default).  Timed with HIP events on the context's stream after a warm-up: median,
minimum and maximum of --reps runs of moptix_query_rays_device (closest: the yardstick) and of moptix_query_rays_multi_device with
maxHits 1, 4, 16, with MOPTIX_MULTI_COUNT_ALL at maxHits 4, and the pure count (maxHits 0).  Prints the table that profiles/r18_multihit.txt keeps."""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minimaloptix_amd as M          # noqa: E402
from query_bench import H, W, line, ray_set      # noqa: E402

K = M._capi
CASES = ((1, 0, "maxHits 1"), (4, 0, "maxHits 4"), (16, 0, "maxHits 16"), (4, K.MULTI_COUNT_ALL, "maxHits 4, COUNT_ALL"), (0, K.MULTI_COUNT_ALL, "maxHits 0, COUNT_ALL"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    n = 1 << a.log2

    import torch
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    print("# file:coffee, %d triangles, %d nodes, depth %d; 2^%d rays per set; %d CUs" % (info.nTriangles, info.nNodes, info.treeDepth, a.log2, ctx.get_option("num_cus")))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    L = K.device_lib()
    sets = {name: torch.from_numpy(ray_set(hs, name, n)).to(dev) for name in ("primary", "incoherent")}
    hits = torch.empty((n, 16, 8), dtype=torch.float32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

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

    for name, rays in sets.items():
        rp, hp, cp = C.c_void_p(rays.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(counts.data_ptr())
        base = line("pt_rayquery closest, %s" % name, n, timed(lambda: L.moptix_query_rays_device(ctx._h, rp, n, K.QUERY_CLOSEST, hp)))
        for k, flags, label in CASES:
            med = line("pt_rayquery_multi %s, %s" % (label, name), n,
                       timed(lambda: L.moptix_query_rays_multi_device(ctx._h, rp, n, k, flags, hp if k else None, cp)))
            c = counts.to(torch.int64)
            print("#   %.2fx the closest query; counts: sum %d, max %d, rays with any %d" % (med / base, int(c.sum()), int(c.max()), int((c > 0).sum())))
    ctx.close()


if __name__ == "__main__":
    main()
