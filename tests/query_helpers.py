"""The ray queries of the CPU mirror (tests/hostsim/querysim.cpp) and the ray sets of the query tests."""
import numpy as np

from common import M, _f32, _ptr, hostsim_handle, hostsim_lib

HIT_DTYPE = M.HIT_DTYPE


def querysim(hs, rays, mode="closest", node_format=64, leaf_size=4):
    """moptix_query_rays on the CPU: a HIT_DTYPE record array ("closest") or an int32 array ("any").  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    rays = _f32(np.asarray(rays, np.float32).reshape(-1, 8))
    out = np.zeros(len(rays), HIT_DTYPE if mode == "closest" else np.int32)
    rc = hostsim_lib().querysim_query(sim._h, int(node_format), _ptr(rays), len(rays), 0 if mode == "closest" else 1, out.ctypes.data)
    assert rc == 0
    return out


def same_bits(a, b):
    """Two result arrays (records or flags) are the same bytes (NaN payloads included)."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_rays(org, d, tmin=1e-3, tmax=1e27):
    n = len(org)
    return np.ascontiguousarray(np.concatenate([org.astype(np.float32), d.astype(np.float32), np.full((n, 1), tmin, np.float32),
                                                np.full((n, 1), tmax, np.float32)], axis=1))


def coffee_rays(n=4096, seed=7):
    """The ray set of test_gpu_parity's test_bvh_trace_equals_oracle_closest_hit: same generator, same construction."""
    rng = np.random.default_rng(seed)
    org = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32); org[:, 1] = rng.uniform(0.0, 0.9, n)
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([org, d.astype(np.float32), np.full((n, 1), 1e-3, np.float32), np.full((n, 1), 1e27, np.float32)], axis=1)


def scene_box(hs):
    """The scene's box as the host library reports it (meshes, the Cornell box); for the scenes of spheres on a ground quad thousands of
    units wide, which report none, the box around the spheres."""
    lo, hi = hs.aabb_min.astype(np.float64), hs.aabb_max.astype(np.float64)
    if (lo <= hi).all():
        return lo, hi
    sph = hs.flat()["spheres"]
    c = np.array([[sph[i].center.x, sph[i].center.y, sph[i].center.z] for i in range(hs.sizes.nSpheres)], np.float64)
    r = np.array([sph[i].radius for i in range(hs.sizes.nSpheres)], np.float64)[:, None]
    return (c - r).min(axis=0), (c + r).max(axis=0)


def box_rays(hs, n=2048, seed=11):
    """n rays with uniform origins inside the scene's box and uniform unit directions."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(hs)
    org = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return make_rays(org, d)


# (scene kind, iarg, ray set): the scenes of the exact comparisons
SCENES = (("file:coffee", 0), ("spheres", 0), ("cornell_quads", 0), ("random_spheres", 60))


def scene_and_rays(kind, iarg):
    hs = M.HostScene(kind, 64, 36, iarg=iarg)
    return hs, (coffee_rays() if kind == "file:coffee" else box_rays(hs))


def shortened(rays, t_oracle, prim_oracle):
    """Half the rays (even indices) end at 0.5 t_oracle, the other half at 2 t_oracle; rays the oracle misses keep their tmax."""
    out = rays.copy()
    hit = prim_oracle >= 0
    f = np.where(np.arange(len(rays)) % 2 == 0, np.float32(0.5), np.float32(2.0)).astype(np.float32)
    out[hit, 7] = (f[hit] * t_oracle[hit]).astype(np.float32)
    return out


def invalid_rays():
    """Rays that are misses by definition, one defect each, on top of a ray that hits coffee's floor from above."""
    base = np.array([0.1, 0.5, 0.2, 0.0, -1.0, 0.0, 1e-3, 1e27], np.float32)
    rows = []
    for k in range(8):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy(); r[k] = bad; rows.append(r)
    r = base.copy(); r[3:6] = 0.0; rows.append(r)                      # zero direction
    r = base.copy(); r[6] = 2.0; r[7] = 2.0; rows.append(r)            # tmax == tmin
    r = base.copy(); r[6] = 3.0; r[7] = 2.0; rows.append(r)            # tmax < tmin
    return np.ascontiguousarray(np.array(rows, np.float32)), base
