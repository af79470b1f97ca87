"""Ray-query throughput on coffee (csrc/querykernel.hip) against moptix_debug_trace's kernel on the same rays.

    python3 tools/query_bench.py [--log2 22] [--reps 12] [--sweep] [--no-rocprof]

Scene file:coffee, tree built once.  Two device-resident ray sets of 2^log2 rays each:
  primary     the pinhole rays of a 1920x1080 frame, pixel after pixel, a uniform jitter inside the pixel (about two per pixel at 2^22)
  incoherent  uniform origins in the scene box, uniform directions
Timed with HIP events on the context's stream (a torch stream handed to moptix_set_stream), after a warm-up: median, minimum and maximum
of --reps runs of moptix_query_rays_device in closest and in any mode.  k_debug_trace's kernel alone is timed in a process of its own
under `rocprofv3 --kernel-trace --stats` (this file with --debug-trace-worker SET), so that moptix_debug_trace's allocations and copies
are left out.  --sweep adds the grid's cap ("query_blocks_per_cu") and the 128-byte nodes on both sets.  Prints the table that profiles/r12_query.txt keeps."""
import argparse
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import minimaloptix_amd as M          # noqa: E402

K = M._capi
W, H = 1920, 1080


def ray_set(hs, name, n):
    rng = np.random.default_rng(12 if name == "primary" else 13)
    if name == "primary":
        cam = hs.params.cam
        v = lambda a: np.array([a.x, a.y, a.z], np.float32)
        i = np.arange(n, dtype=np.int64) % (W * H)
        fx = ((i % W).astype(np.float32) + rng.random(n, dtype=np.float32)) / np.float32(W)
        fy = ((i // W).astype(np.float32) + rng.random(n, dtype=np.float32)) / np.float32(H)
        d = v(cam.scrLowerLeftCorner)[None, :] + fx[:, None] * v(cam.horizontal)[None, :] + fy[:, None] * v(cam.vertical)[None, :] - v(cam.origin)[None, :]
        org = np.tile(v(cam.origin), (n, 1))
    else:
        org = rng.uniform(hs.aabb_min.astype(np.float64), hs.aabb_max.astype(np.float64), (n, 3)).astype(np.float32)
        d = rng.normal(size=(n, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([org, d, np.full((n, 1), 1e-3, np.float32), np.full((n, 1), 1e27, np.float32)], axis=1))


def worker(name, n, reps):
    """moptix_debug_trace on one ray set, reps + 1 times (the profiler outside sees k_debug_trace's dispatches)."""
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    rays = ray_set(hs, name, n)
    for _ in range(reps + 1):
        t, prim = ctx.debug_trace(rays)
    print("worker %s: %d rays, %d hits" % (name, n, int((prim >= 0).sum())))
    ctx.close()


def debug_trace_ms(name, n, reps):
    """[ms per dispatch of k_debug_trace] from a profiled child process, warm-up dispatch dropped; None if the profiler is not there."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--debug-trace-worker", name, "--log2", str(int(np.log2(n))), "--reps", str(reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as e:
            print("# rocprofv3 run failed: %s" % e)
            return None
        if r.returncode != 0:
            print("# rocprofv3 run failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-400:]))
            return None
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "k_debug_trace" in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        if rows:
            rows.sort()
            return [(e - s) * 1e-6 for s, e in rows[1:]]
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "k_debug_trace" in row["Name"]:
                    return [float(row["MinNs"]) * 1e-6, float(row["AverageNs"]) * 1e-6, float(row["MaxNs"]) * 1e-6]
    return None


def line(label, n, ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    print("%-44s %8.3f ms  [%7.3f .. %7.3f]  %8.1f Mrays/s  (%d runs)" % (label, med, ms[0], ms[-1], n / med * 1e-3, len(ms)))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--debug-trace-worker", default=None)
    a = ap.parse_args()
    n = 1 << a.log2
    if a.debug_trace_worker:
        return worker(a.debug_trace_worker, n, a.reps)

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
    hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def timed(rays, mode):
        out = hits if mode == K.QUERY_CLOSEST else flags
        ms = []
        for i in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = L.moptix_query_rays_device(ctx._h, C.c_void_p(rays.data_ptr()), n, mode, C.c_void_p(out.data_ptr()))
            assert rc == K.MOPTIX_OK, ctx.last_error()
            e1.record(stream)
            stream.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        return ms

    med = {}
    for name, rays in sets.items():
        for mode, mname in ((K.QUERY_CLOSEST, "closest"), (K.QUERY_ANY, "any")):
            med[name, mname] = line("pt_rayquery %s, %s" % (mname, name), n, timed(rays, mode))
        print("#   hits: %d of %d; occluded: %d" % (int((hits.view(torch.int32)[:, 1] >= 0).sum()), n, int(flags.sum())))
    if a.sweep:
        for name, rays in sets.items():
            for val in (1, 2, 4, 8, 16, 32, 64):
                ctx.set_option("query_blocks_per_cu", val)
                line("  query_blocks_per_cu=%d closest, %s" % (val, name), n, timed(rays, K.QUERY_CLOSEST))
            ctx.set_option("query_blocks_per_cu", 32)
            ctx.set_option("node_format", 128)
            line("  node_format=128 closest, %s" % name, n, timed(rays, K.QUERY_CLOSEST))
            ctx.set_option("node_format", 0)
    ctx.close()
    if not a.no_rocprof:
        for name in sets:
            ms = debug_trace_ms(name, n, a.reps)
            if ms:
                m = line("k_debug_trace (rocprofv3), %s" % name, n, ms)
                print("#   pt_rayquery closest is %.2fx k_debug_trace on this set" % (m / med[name, "closest"]))


if __name__ == "__main__":
    main()
