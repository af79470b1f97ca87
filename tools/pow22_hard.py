#!/usr/bin/env python3
"""The hard cases of pow22 (pt_texture.h, AC6): writes tests/golden/pow22_hard.json.  CPU only.

pow22(x) = (float)pow((double)x, (double)2.2f) runs the ROCm device library's binary64 pow on the device and glibc's on the host.  Two
faithful pows may differ in the last binary64 bit, and the binary32 result then differs wherever that bit decides the rounding.  This
scan (da_host_pow22_scan in tests/devarith/devarith_host.cpp) visits every positive finite float whose result is a finite binary32 and
keeps the inputs whose glibc pow lies within 16 binary64 ulps of a binary32 rounding boundary, boundaries of the subnormal range included.
Each is written with glibc's binary32 result, the correctly rounded one (mpmath, 240 bits) and the true value's distance from the boundary in
binary64 ulps.

    python3 tools/pow22_hard.py            # rewrites the golden file (about ten seconds)
    python3 tools/pow22_hard.py --check    # compares with the committed file instead"""
import ctypes as C
import json
import os
import sys
from fractions import Fraction

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import devarith_helpers as D      # noqa: E402

WINDOW = 16


def scan(first=0x00000001, last=0x7f7fffff):
    cap = 1 << 16
    xs = np.zeros(cap, np.uint32); dist = np.zeros(cap, np.int32)
    n = D.lib().da_host_pow22_scan(first, last, WINDOW, xs.ctypes.data_as(C.POINTER(C.c_uint32)), dist.ctypes.data_as(C.POINTER(C.c_int32)), cap)
    assert 0 <= n <= cap, n
    order = np.argsort(xs[:n])
    return xs[:n][order], dist[:n][order]


def exact(xbits):
    """(correctly rounded binary32 bits, distance of the true value from the nearest binary32 rounding boundary in binary64 ulps)"""
    import mpmath
    mpmath.mp.prec = 240
    x = mpmath.mpf(float(D.f32(np.array([xbits], np.uint32))[0]))
    y = mpmath.power(x, mpmath.mpf(float(np.float32(2.2))))
    q = Fraction(int(y.man), 1) * Fraction(2) ** int(y.exp)
    b = D.round_to_f32(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()                      # 2^e <= q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1
    half = Fraction(2) ** (max(e, -126) - 24)                                      # half a binary32 spacing: boundaries are its odd multiples
    k = (q / half).numerator // (q / half).denominator
    odd = k if k & 1 else k + 1                                                    # the nearest one to q in [k, k + 1) half
    return b, float(abs(q - odd * half) / Fraction(2) ** (e - 52))


def build():
    xs, dist = scan()
    glibc = D.run("pow22", xs, device=False)
    rows = []
    for x, d, g in zip(xs, dist, glibc):
        b, de = exact(int(x))
        rows.append({"x": "0x%08x" % int(x), "dist": int(d), "glibc": "0x%08x" % int(g), "exact": "0x%08x" % b, "dist_exact": round(de, 4)})
    return {"what": "positive finite binary32 x whose glibc pow((double)x, (double)2.2f) lies within `window` binary64 ulps of a binary32 "
                    "rounding boundary; dist: that distance; glibc / exact: the binary32 result of glibc and the correctly rounded one; "
                    "dist_exact: the true value's distance from the boundary in binary64 ulps",
            "window": WINDOW, "inputs": rows}


def main():
    doc = build()
    unit = [r for r in doc["inputs"] if int(r["x"], 16) <= 0x3f800000]
    print("%d inputs, %d of them in (0, 1]; %d within 2 ulps, %d where glibc is not the correctly rounded value" % (
        len(doc["inputs"]), len(unit), sum(r["dist"] <= 2 for r in doc["inputs"]), sum(r["glibc"] != r["exact"] for r in doc["inputs"])))
    if "--check" in sys.argv:
        with open(D.POW22_GOLDEN) as f:
            assert json.load(f) == doc, "tests/golden/pow22_hard.json differs from this scan"
        print("matches", os.path.relpath(D.POW22_GOLDEN, REPO))
        return
    with open(D.POW22_GOLDEN, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("wrote", os.path.relpath(D.POW22_GOLDEN, REPO))


if __name__ == "__main__":
    main()
