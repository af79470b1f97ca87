"""The multi-hit ray queries of the CPU mirror (tests/hostsim/multihitsim.cpp, in libhostsim.so): the traversal through the kernel's per-ray
code, and the definition itself as a loop over every primitive record; the ray sets and checks the multi-hit tests share."""
import ctypes as C

import numpy as np

from common import M, _f32, _ptr, hostsim_handle, hostsim_lib
from query_helpers import same_bits, scene_and_rays      # noqa: F401  (for the tests)

HIT_DTYPE = M.HIT_DTYPE
COUNT_ALL = 1                                             # MOPTIX_MULTI_COUNT_ALL, spelled out here apart from the package's definition
KS = (1, 2, 4, 8, 64)

_signed = False


def _lib():
    """libhostsim.so with the signatures of multihitsim.cpp's two entries (common.hostsim_lib declares the ones of the mirrors before it)."""
    global _signed
    L = hostsim_lib()
    if not _signed:
        vp, f32p, i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.multihitsim_query.argtypes, L.multihitsim_query.restype = [vp, C.c_int, f32p, C.c_int64, C.c_int, C.c_uint32, vp, i32p], C.c_int
        L.multihitsim_brute.argtypes, L.multihitsim_brute.restype = [vp, f32p, C.c_int64, C.c_int, C.c_uint32, vp, i32p], C.c_int
        _signed = True
    return L


def _rays(rays):
    return _f32(np.asarray(rays, np.float32).reshape(-1, 8))


def multisim(hs, rays, max_hits=4, count_all=False, node_format=64, leaf_size=4):
    """moptix_query_rays_multi on the CPU, by the traversal: (hits (n, max_hits) HIT_DTYPE, counts int32).  hs: a scene, or a built one."""
    sim = hostsim_handle(hs, leaf_size)
    rays = _rays(rays)
    hits, counts = np.zeros((len(rays), max_hits), HIT_DTYPE), np.zeros(len(rays), np.int32)
    rc = _lib().multihitsim_query(sim._h, int(node_format), _ptr(rays), len(rays), int(max_hits), COUNT_ALL if count_all else 0,
                                  hits.ctypes.data if max_hits else None, _ptr(counts, C.c_int32))
    assert rc == 0
    return hits, counts


def multibrute(hs, rays, max_hits=4, count_all=False, leaf_size=4):
    """The same from the definition: every primitive record tested, the hit set sorted by (t, prim)."""
    sim = hostsim_handle(hs, leaf_size)
    rays = _rays(rays)
    hits, counts = np.zeros((len(rays), max_hits), HIT_DTYPE), np.zeros(len(rays), np.int32)
    rc = _lib().multihitsim_brute(sim._h, _ptr(rays), len(rays), int(max_hits), COUNT_ALL if count_all else 0,
                                  hits.ctypes.data if max_hits else None, _ptr(counts, C.c_int32))
    assert rc == 0
    return hits, counts


def is_miss_record(h, tmax):
    """Element-wise: the record is a miss record with t = tmax's bits (h: (n, k) records, tmax: (n,) float32)."""
    t_ok = h["t"].view(np.uint32) == np.asarray(tmax, np.float32).view(np.uint32)[:, None]
    zero = (h["u"].view(np.uint32) == 0) & (h["v"].view(np.uint32) == 0) & (h["ng"].view(np.uint32) == 0).all(axis=-1)
    return t_ok & (h["prim"] == -1) & (h["mat"] == -1) & zero


def axis_rays(org, axis, sign=1.0, tmin=0.0, tmax=1e27):
    """Rays from the points org along +-axis, with exact zeros in the other two components."""
    org = np.asarray(org, np.float32).reshape(-1, 3)
    d = np.zeros((len(org), 3), np.float32); d[:, axis] = sign
    return np.ascontiguousarray(np.concatenate([org, d, np.full((len(org), 1), tmin, np.float32), np.full((len(org), 1), tmax, np.float32)], axis=1))
