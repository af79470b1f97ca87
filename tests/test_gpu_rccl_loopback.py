"""The N > 1 branches of moptix_gather_tiles / moptix_reduce_frame as N processes on ONE GPU.

RCCL refuses a communicator whose ranks share a device ("Duplicate GPU detected": tried in round 4, tools/rccl_two_ranks.py
--same-device without a transport override), and no multi-GPU box has been available.  So the nine ncclXxx entry points that
libmoptix.so binds are stood in for by tests/rccl_loopback (shared memory + hipMemcpy, MOPTIX_RCCL_LIB): what runs here is
everything on this project's side of those calls -- pack kernel -> send, grouped receives -> per-rank unpack kernels, the
reduce call, the partition / communicator checks, `moptix_render --spawn N` with its id file -- NOT RCCL and not xGMI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import M, REPO

LOOPBACK = os.path.join(REPO, "tests", "rccl_loopback", "librccl_loopback.so")


def _env():
    e = dict(os.environ)
    e["MOPTIX_RCCL_LIB"] = LOOPBACK
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_n_ranks_gather_and_reduce_through_the_c_abi(n):
    """N processes, one context each on device 0: tile split + moptix_gather_tiles is bit-identical to the one-rank frame,
    sample split + moptix_reduce_frame equals it within the summation-order bound (dist.SAMPLE_SPLIT_TOL)."""
    assert os.path.exists(LOOPBACK), "make -C tests/rccl_loopback"
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "rccl_two_ranks.py"), str(n), "--same-device"],
                       env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "bit-identical to the one-rank frame" in p.stdout and ("over %d ranks" % n) in p.stdout, p.stdout[-1000:]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["device", "host"])
def test_a_peer_that_never_sends_ends_the_collective_at_its_deadline(where):
    """moptix_gather_tiles with a peer that joined the communicator and then never calls.  "device": the receive's kernel sits on rank 0's
    stream and does not end (MOPTIX_LOOPBACK_STUCK=1 models RCCL's spinning kernel); comm_wait polls the stream and aborts the communicator
    after comm_timeout_ms (1.5 s here).  "host" (ADVICE r5): the call never gets that far -- the library is still setting the peer's
    connections up, which a blocking communicator does INSIDE ncclGroupEnd; the communicator is therefore non-blocking
    (ncclCommInitRankConfig), ncclGroupEnd returns ncclInProgress (MOPTIX_LOOPBACK_STUCK=2) and comm_settle polls the communicator's state
    against the same deadline.  Either way the call returns MOPTIX_ERR_COMM and the context is a one-rank context again."""
    e = _env(); e["MOPTIX_LOOPBACK_STUCK"] = "1" if where == "device" else "2"; e["RCCL_TWO_RANKS_DEAD_PEER"] = "1"
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "rccl_two_ranks.py"), "2", "--same-device"],
                       env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "came back after" in p.stdout and "code -6" in p.stdout and "dead peer: rank 0's collective was aborted" in p.stdout, p.stdout[-1500:]
    assert ("still in progress on the host" in p.stdout) == (where == "host"), p.stdout[-1500:]


def _read_png(path):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from test_gpu_configs import _read_png as rp
    return rp(path)


@pytest.mark.gpu
def test_cli_spawn_2_ranks_on_one_gpu(tmp_path):
    """moptix_render --spawn 2 --spawn-same-device: the parent forks two ranks before anything touches the GPU, rank 0 publishes the
    communicator id through the file, both render their tiles, moptix_gather_tiles brings rank 1's tiles to rank 0, which writes
    the frame: the same bytes as the plain run."""
    exe = os.path.join(REPO, "minimaloptix_amd", "lib", "moptix_render")
    common = ["--scene", "spheres", "--spp", "3", "--width", "160", "--height", "90", "--outdir", str(tmp_path), "--scenes", M.scenes_dir()]
    r1 = subprocess.run([exe] + common + ["--out", "one"], capture_output=True, text=True, timeout=300)
    r2 = subprocess.run([exe] + common + ["--out", "two", "--spawn", "2", "--spawn-same-device", "--spawn-timeout", "120"],
                        env=_env(), capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1500:], r2.stderr[-1500:])
    assert np.array_equal(_read_png(os.path.join(str(tmp_path), "one.png")), _read_png(os.path.join(str(tmp_path), "two.png")))


@pytest.mark.gpu
def test_cli_spawn_ends_the_other_ranks_when_one_fails(tmp_path):
    """A rank that dies must not leave its peers (and the parent's wait) blocked for ever: with real RCCL on this one-GPU box
    ncclCommInitRank fails in every rank ("Duplicate GPU"), the parent reports the failure and exits non-zero, within its deadline."""
    exe = os.path.join(REPO, "minimaloptix_amd", "lib", "moptix_render")
    args = ["--scene", "spheres", "--spp", "1", "--width", "64", "--height", "36", "--outdir", str(tmp_path), "--scenes", M.scenes_dir(),
            "--out", "x", "--spawn", "2", "--spawn-same-device", "--spawn-timeout", "90"]
    e = dict(os.environ); e.pop("MOPTIX_RCCL_LIB", None)
    r = subprocess.run([exe] + args, env=e, capture_output=True, text=True, timeout=200)
    assert r.returncode != 0, r.stderr[-1000:]


def _bench_two_ranks(e, split, extra=()):
    sys.path.insert(0, REPO)
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e["MOPTIX_BENCH_BACKEND"] = "gloo"; e["MOPTIX_BENCH_DEVICE"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(bench.free_port()), os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--width", "320", "--height", "180", "--spp", "8", "--no-cpu-baseline", "--no-fast-leg", "--split", split] + list(extra)
    return subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
def test_bench_py_times_both_modes_in_one_run_and_reports_the_better():
    """from PIPELINE_FROM_RANKS ranks on (8; lowered to 2 here) one run times BOTH modes -- one frame at a time, then two
    frames in flight (second context + second communicator per rank, made when the mode starts, with its own pre-flight collective) -- K steps
    each; config.modes carries both, `value` is the better one and config.mode names it."""
    import json
    e = _env(); e["MOPTIX_BENCH_PIPELINE_FROM"] = "2"; e.pop("MOPTIX_BENCH_PIPELINE", None)
    p = _bench_two_ranks(e, "tile")
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    modes = d["config"]["modes"]
    assert set(modes) == {"one_frame", "two_in_flight"} and all(m["ms_per_frame"] > 0 for m in modes.values())
    assert d["config"]["mode"] == min(modes, key=lambda m: modes[m]["ms_per_frame"]) and d["ms_per_step"] == modes[d["config"]["mode"]]["ms_per_frame"]
    assert d["config"]["pipeline"] == (d["config"]["mode"] == "two_in_flight") and d["pmc_live"] is False
    assert "non-blocking" in d["config"]["communicator"] and d["config"]["communicator_note"] is None


@pytest.mark.gpu
def test_bench_py_prints_an_error_line_when_the_ranks_cannot_communicate():
    """A peer that never delivers (MOPTIX_LOOPBACK_STUCK=1: rank 0's receive is a kernel that does not end): the pre-flight collective hits its
    deadline (1.5 s here), every rank falls back to a blocking communicator once, that fails too, and rank 0 prints ONE JSON line with "error" and
    each rank's diagnosis; the processes exit non-zero -- nobody hangs, nobody is re-executed."""
    import json
    e = _env(); e["MOPTIX_LOOPBACK_STUCK"] = "1"; e["MOPTIX_BENCH_PREFLIGHT_MS"] = "1500"
    p = _bench_two_ranks(e, "tile")
    assert p.returncode != 0, p.stdout[-1500:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(lines[0])
    assert d["value"] is None and "pre-flight" in d["error"] and d["n_gpus"] == 2
    diag = d["config"]["ranks"]["diagnosis"]
    assert len(diag) == 2 and "rank 0" in diag[0] and ("aborted" in diag[0] or "abandoned" in diag[0]) and diag[1].endswith("ok")


@pytest.mark.gpu
@pytest.mark.parametrize("split,pipeline", [("tile", "0"), ("sample", "0"), ("tile", "1")])
def test_bench_py_two_ranks_on_one_gpu(split, pipeline):
    """bench.py's N > 1 body on the GPU: two ranks under torch.distributed.run (gloo for the control plane, both on device 0, the frame's
    collective through the loop-back transport).  One JSON line from rank 0 with the per-rank diagnosis VERDICT r3 asked for; the line
    says itself that it is test plumbing."""
    import json
    e = _env()
    e["MOPTIX_BENCH_BACKEND"] = "gloo"; e["MOPTIX_BENCH_DEVICE"] = "0"
    e["MOPTIX_BENCH_PIPELINE"] = pipeline      # "1": two frames in flight = two contexts with a communicator each per rank (the default from 8 ranks on)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    sys.path.insert(0, REPO)
    import bench
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(bench.free_port()), os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--width", "320", "--height", "180", "--spp", "8", "--no-cpu-baseline", "--no-fast-leg", "--split", split, "--full"]
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    r = d["config"]["ranks"]
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["split"] == split and "TEST PLUMBING" in d["config"]["parallelism"]
    assert d["config"]["pipeline"] == (pipeline == "1")
    assert len(r["kernel_ms_per_frame"]) == 2 and min(r["kernel_ms_per_frame"]) > 0 and r["comm_ranks_seen"] == 2
    assert len(r["collective_ms_per_frame"]) == 2 and max(r["collective_ms_per_frame"]) > 0
    assert len(r["rays_per_frame"]) == 2 and sum(r["rays_per_frame"]) == d["config"]["rays_per_frame"]
    fc = d["config"]["frame_check"]             # rank 0 rendered the whole frame itself and compared
    assert fc["ok"] and (fc["bit_identical"] if split == "tile" else fc["max_abs_diff_per_sample"] <= fc["bound"]), fc
    if split == "tile":                       # the rotating tile deal: the two shares within a few per cent of each other
        assert abs(r["rays_per_frame"][0] - r["rays_per_frame"][1]) < 0.1 * sum(r["rays_per_frame"])
