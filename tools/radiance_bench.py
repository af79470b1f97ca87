"""Radiance-query time on coffee (csrc/radiancekernel.hip) against moptix_render under kernel variant 0 on the same samples.

    python3 tools/radiance_bench.py [--spp 16] [--reps 5] [--probe-rays 4096] [--probe-samples 1024]

Scene file:coffee at 1920x1080, tree built once.
  camera  the camera's own rays and the RNG states its lens and jitter draws leave behind (tests/hostsim radiancesim_camera), for --spp
          launch seeds, as one device-resident batch of spp x 1920 x 1080 rays with one sample each and the clamp flag: the samples of
          moptix_render(seeds).  The render runs the per-lane megakernel the query's loops are copied from ("kernel_variant" 0); its time is
          moptix_kernel_time + moptix_reduce_time (trace kernel + ordered reduction), the query's is HIP events round the call on the
          context's stream (trace kernel + ordered sum).  The two results are compared bit for bit.
  probes  --probe-rays rays with uniform origins in the scene box and uniform directions, --probe-samples samples each from a seed list.
Median, minimum and maximum of --reps runs after a warm-up.  Prints the table that profiles/r15_radiance.txt keeps."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import minimaloptix_amd as M          # noqa: E402
from radiance_helpers import camera_rays_states          # noqa: E402

K = M._capi
W, H = 1920, 1080


def line(label, n, ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    print("%-52s %9.3f ms  [%8.3f .. %8.3f]  %8.1f Msamples/s  (%d runs)" % (label, med, ms[0], ms[-1], n / med * 1e-3, len(ms)))
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probe-rays", type=int, default=4096)
    ap.add_argument("--probe-samples", type=int, default=1024)
    a = ap.parse_args()

    import torch
    hs = M.HostScene("file:coffee", W, H)
    ctx = M.Context(0)
    ctx.load(hs)
    info = ctx.accel_info()
    print("# file:coffee %dx%d, %d triangles, %d nodes, depth %d; %d CUs" % (W, H, info.nTriangles, info.nNodes, info.treeDepth, ctx.get_option("num_cus")))
    dev = torch.device("cuda", 0)
    seeds = M.launch_seeds(a.spp)
    L = K.device_lib()

    # ---- the frame under kernel variant 0 ----
    ctx.set_option("kernel_variant", 0)
    ms = []
    for i in range(a.reps + 1):
        ctx.accum_clear(); ctx.kernel_time(reset=True)
        ctx.render(seeds)
        if i >= 1:
            ms.append(ctx.kernel_time()[0] + ctx.reduce_time())
    frame = ctx.accum_read().reshape(-1, 3)
    n = a.spp * W * H
    t_render = line("moptix_render, kernel_variant 0, %d spp" % a.spp, n, ms)

    # ---- the same samples through the radiance query ----
    parts = [camera_rays_states(hs, s) for s in seeds]
    rays = torch.from_numpy(np.concatenate([p[0] for p in parts])).to(dev)
    states = torch.from_numpy(np.concatenate([p[1] for p in parts]).view(np.int32)).to(dev)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    ctx.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()

    def timed(call):
        ms = []
        for i in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            rc = call()
            assert rc == K.MOPTIX_OK, ctx.last_error()
            e1.record(stream)
            stream.synchronize()
            if i >= 1:
                ms.append(e0.elapsed_time(e1))
        return ms

    t_query = line("moptix_query_radiance_device, camera rays, clamp", n, timed(lambda: L.moptix_query_radiance_device(
        ctx._h, C.c_void_p(rays.data_ptr()), n, None, C.c_void_p(states.data_ptr()), 1, 0, K.RADIANCE_CLAMP, C.c_void_p(out.data_ptr()))))
    acc = np.zeros((W * H, 3), np.float32)
    res = out.cpu().numpy()
    for s in range(a.spp):
        acc = (acc + res[s * W * H:(s + 1) * W * H, :3]).astype(np.float32)
    print("#   the query's samples summed per pixel in seed order %s the render's accumulation buffer" % ("ARE" if acc.tobytes() == frame.tobytes() else "ARE NOT"))
    hbm = 32.0 * n / 8e12 * 1e3      # a 16-byte record written and read once, at the 8 TB/s HBM rate of DESIGN.md's roofline
    print("#   query / render = %.3f; scratch traffic of the query: %d samples x 32 B = %.3f ms at 8 TB/s (%.1f %% of the render's time)" % (
        t_query / t_render, n, hbm, 100.0 * hbm / t_render))
    del rays, states, out

    # ---- a probe set: few rays, many samples each ----
    rng = np.random.default_rng(14)
    org = rng.uniform(hs.aabb_min.astype(np.float64), hs.aabb_max.astype(np.float64), (a.probe_rays, 3)).astype(np.float32)
    d = rng.normal(size=(a.probe_rays, 3)).astype(np.float32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    pr = np.concatenate([org, d, np.full((a.probe_rays, 1), 1e-3, np.float32), np.full((a.probe_rays, 1), 1e27, np.float32)], axis=1)
    prays = torch.from_numpy(np.ascontiguousarray(pr)).to(dev)
    pout = torch.empty((a.probe_rays, 4), dtype=torch.float32, device=dev)
    pseeds = M.launch_seeds(a.probe_samples)
    sp = pseeds.ctypes.data_as(C.POINTER(C.c_int32))
    torch.cuda.synchronize()
    line("moptix_query_radiance_device, %d probes x %d samples" % (a.probe_rays, a.probe_samples), a.probe_rays * a.probe_samples,
         timed(lambda: L.moptix_query_radiance_device(ctx._h, C.c_void_p(prays.data_ptr()), a.probe_rays, sp, None, a.probe_samples, 0, 0,
                                                      C.c_void_p(pout.data_ptr()))))
    mean = (pout[:, :3] / a.probe_samples).mean(dim=0).cpu().numpy()
    print("#   mean probe radiance %.4f %.4f %.4f; %d of %d probes see a surface" % (mean[0], mean[1], mean[2], int((pout[:, 3] < 1e27).sum()), a.probe_rays))
    ctx.close()


if __name__ == "__main__":
    main()
