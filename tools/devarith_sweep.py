#!/usr/bin/env python3
"""The exhaustive sweep behind tests/test_gpu_devarith.py: device against host twin over EVERY input (not a test: minutes, on the GPU).

    python3 tools/devarith_sweep.py [rcp sqrt floor exp_ac sincos_ac pow22]      # default: all six

  rcp, sqrt, floor, exp_ac   all 2^32 bit patterns
  sincos_ac                  every float of [-100, 100], both zeros
  pow22                      every positive float, +inf included

in chunks of 2^26 through tests/devarith/libdevarith.so (one launch per chunk), compared by the rule of tests/devarith_helpers.py (bits;
NaNs equal).  Stops at the first HIP error.  Prints, per primitive, the number of inputs, the number of mismatches and the first 16
mismatching inputs; profiles/r27_devarith.txt keeps a run."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import devarith_helpers as D      # noqa: E402

CHUNK = 1 << 26
RANGES = {      # runs of bit patterns, first and last inclusive
    "rcp": [(0x00000000, 0xffffffff)], "sqrt": [(0x00000000, 0xffffffff)], "floor": [(0x00000000, 0xffffffff)], "exp_ac": [(0x00000000, 0xffffffff)],
    "sincos_ac": [(0x00000000, 0x42c80000), (0x80000000, 0xc2c80000)],      # +0 .. 100.0f, -0 .. -100.0f
    "pow22": [(0x00000001, 0x7f800000)],
}


def sweep(name):
    total = bad_total = 0
    examples = []
    t0 = time.time()
    for lo, last in ((lo, last) for first, last in RANGES[name] for lo in range(first, last + 1, CHUNK)):
        x = np.arange(lo, min(lo + CHUNK, last + 1), dtype=np.uint64).astype(np.uint32)
        dev = D.run(name, x, device=True, sweep=True)          # any HIP error raises here and ends the sweep
        host = D.run(name, x, device=False)
        for d, h in zip(np.atleast_2d(np.stack(dev) if isinstance(dev, list) else dev), np.atleast_2d(np.stack(host) if isinstance(host, list) else host)):
            cand = np.nonzero(d != h)[0]
            cand = cand[~(D.is_nan(d[cand]) & D.is_nan(h[cand]))]
            bad_total += len(cand)
            for i in cand[: max(0, 16 - len(examples))]:
                examples.append("0x%08x -> device 0x%08x, host 0x%08x" % (int(x[i]), int(d[i]), int(h[i])))
        total += len(x)
        print("  %s: %d inputs done, %d mismatches, %.0f s" % (name, total, bad_total, time.time() - t0), flush=True)
    print("%s: %d inputs, %d mismatches%s" % (name, total, bad_total, "".join("\n    " + e for e in examples)), flush=True)
    return bad_total


def main():
    names = sys.argv[1:] or list(RANGES)
    bad = sum(sweep(n) for n in names)
    print("sweep: %d mismatches over %s" % (bad, ", ".join(names)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
