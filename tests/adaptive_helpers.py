"""The adaptive sampling of the CPU mirror (tests/hostsim/adaptivesim.cpp) and helpers for the adaptive-sampling tests."""
import ctypes as C

import numpy as np

from common import K, _ptr, hostsim_handle, hostsim_lib, hostsim_render

ADAPTIVE_DEFAULTS = dict(threshold=0.03, min_samples=16, batch=64)
STATS_KEYS = ("passes", "samples_traced", "samples_uniform", "active_pixels_last", "converged_pixels", "min_count", "max_count")


def adaptive_params(threshold=None, min_samples=None, batch=None):
    d = ADAPTIVE_DEFAULTS
    return K.AdaptiveParams(float(d["threshold"] if threshold is None else threshold), int(d["min_samples"] if min_samples is None else min_samples),
                            int(d["batch"] if batch is None else batch))


def check_params(threshold, min_samples, batch):
    """The argument check of moptix_render_adaptive, as the mirror carries it: MOPTIX_OK or ERR_INVALID."""
    p = K.AdaptiveParams(float(threshold), int(min_samples), int(batch))
    return hostsim_lib().adaptivesim_check_params(C.byref(p))


class AdaptiveSim:
    """A context's adaptive state and accumulation buffer on the CPU: render() is Context.render_adaptive over per-seed sample images,
    clear() is adaptive_clear, read() is accum_read + adaptive_read."""

    def __init__(self, width, height):
        self._h = C.c_void_p(hostsim_lib().adaptivesim_create())
        self.width, self.height = int(width), int(height)
        self.clear()

    def __del__(self):
        if getattr(self, "_h", None):
            hostsim_lib().adaptivesim_destroy(self._h)
            self._h = None

    def clear(self):
        hostsim_lib().adaptivesim_clear(self._h, self.width, self.height)

    def render(self, samples, threshold=None, min_samples=None, batch=None):
        """samples: (nSeeds, H, W, 3) float32, the image each seed adds to a zero accumulator.  Returns the stats dict."""
        samples = np.ascontiguousarray(samples, np.float32).reshape(-1, self.height, self.width, 3)
        p = adaptive_params(threshold, min_samples, batch)
        st = K.AdaptiveStats()
        rc = hostsim_lib().adaptivesim_render(self._h, self.width, self.height, _ptr(samples), len(samples), C.byref(p), C.byref(st))
        assert rc == 0, rc
        return st.as_dict()

    def read(self):
        h, w = self.height, self.width
        out = dict(accum=np.empty((h, w, 3), np.float32), count=np.empty((h, w), np.uint32), moments=np.empty((h, w, 2), np.float32),
                   error=np.empty((h, w), np.float32), converged=np.empty((h, w), np.uint8))
        hostsim_lib().adaptivesim_read(self._h, _ptr(out["accum"]), _ptr(out["count"], C.c_uint32), _ptr(out["moments"]), _ptr(out["error"]),
                                           _ptr(out["converged"], C.c_uint8))
        return out

    def mean(self):
        m = np.empty((self.height, self.width, 3), np.float32); rgb8 = np.empty((self.height, self.width, 3), np.uint8)
        hostsim_lib().adaptivesim_mean(self._h, _ptr(m), _ptr(rgb8, C.c_uint8))
        return m, rgb8


def hostsim_samples(hs, seeds):
    """(nSeeds, H, W, 3): hostsim_render with one seed at a time into a zero accumulator -- that IS the clamped sample."""
    sim = hostsim_handle(hs)                                 # the tree is built once, not once per seed
    return np.stack([hostsim_render(sim, [int(s)])[0] for s in seeds])


def sequential_sums(samples):
    """(nSeeds + 1, H, W, 3): the plain float32 sum of the first k sample images, k = 0 .. nSeeds, added in seed order."""
    out = np.zeros((len(samples) + 1,) + samples.shape[1:], np.float32)
    for k in range(len(samples)):
        out[k + 1] = out[k] + samples[k]
    return out


def prefix_pick(snapshots, count):
    """Per pixel the snapshot taken at that pixel's count: snapshots (n + 1, H, W, 3), count (H, W) -> (H, W, 3)."""
    c = np.asarray(count, np.int64)
    yy, xx = np.mgrid[0:c.shape[0], 0:c.shape[1]]
    return snapshots[c, yy, xx]
