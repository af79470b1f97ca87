"""The arithmetic contract's primitives on the host (no GPU): what the device comparison of tests/test_gpu_devarith.py rests on.

  * the host twin of + - x / sqrt fma equals the exact rational value rounded once (round_to_f32) -- this validates the reference, which
    is otherwise this machine's hardware;
  * sincos_ac: the host twin and the oracle's orc_sincos are the same bits, and the absolute error against binary64 is below the 2e-7 that
    pt_math.h documents;
  * pow22: the host twin reproduces tests/golden/pow22_hard.json, and glibc's value is the correctly rounded one on every listed input;
  * every input set is deterministic (the hash of its bytes)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import devarith_helpers as D
from common import O


def test_round_to_f32_known_values():
    cases = [(Fraction(1), 0x3f800000), (Fraction(-3, 2), 0xbfc00000), (Fraction(1, 3), 0x3eaaaaab), (Fraction(2) ** -149, 0x00000001),
             (Fraction(2) ** -150, 0x00000000), (Fraction(3, 2) * Fraction(2) ** -149, 0x00000002), (Fraction(2) ** -126, 0x00800000),
             (Fraction(2) ** -126 - Fraction(2) ** -150, 0x00800000), (Fraction(2) ** -126 - Fraction(2) ** -149, 0x007fffff),
             (Fraction(2) ** 128 - Fraction(2) ** 104, 0x7f7fffff), (Fraction(2) ** 128 - Fraction(2) ** 103, 0x7f800000),
             (Fraction(2) ** 130, 0x7f800000), (1 + Fraction(2) ** -24, 0x3f800000), (1 + 3 * Fraction(2) ** -24, 0x3f800002),
             (-(1 + Fraction(2) ** -24 + Fraction(2) ** -60), 0xbf800001), (Fraction(0), 0)]
    for q, want in cases:
        assert D.round_to_f32(q) == want, (q, hex(D.round_to_f32(q)), hex(want))
    # every finite pattern of a sample is a fixed point
    for b in D.set_U()[:: 997]:
        if D.is_finite(b):
            assert D.round_to_f32(D.frac(b)) == (int(b) if int(b) != 0x80000000 else 0)


EXACT = {
    "add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b,
    "fma": lambda a, b, c: a * b + c,
}


@pytest.mark.parametrize("name", ["add", "sub", "mul", "div", "fma", "sqrt"])
def test_host_twin_equals_the_exact_value(name):
    if name == "sqrt":
        x = D.set_U()
        got = D.run("sqrt", x, device=False)
        idx = D.exact_subset(D.is_finite(x) & ((x >> 31) == 0) & (x != 0))
        bad = [(int(x[i]), int(got[i])) for i in idx if D.sqrt_round_to_f32(x[i]) != int(got[i])]
        assert not bad, bad[:6]
        return
    ops = D.set_T() if name == "fma" else D.set_P()
    got = D.run(name, *ops, device=False)
    fin = np.logical_and.reduce([D.is_finite(o) for o in ops])
    if name == "div":
        fin &= (D.bits(ops[1]) & 0x7fffffff) != 0
    # half of the subset from the set's tail: the division-hard, subnormal-quotient and cancellation cases
    n = len(got)
    tail = fin & (np.arange(n) >= n - (1 << 19))
    idx = np.concatenate([D.exact_subset(fin, 2048), D.exact_subset(tail, 2048, seed=7)])
    D.assert_exact(name, got, ops, idx, EXACT[name])


def test_sincos_ac_host_twin_is_the_oracle_and_within_2e7_of_binary64():
    L = O.lib()
    f32p = C.POINTER(C.c_float)
    L.orc_sincos_n.argtypes, L.orc_sincos_n.restype = [f32p, f32p, f32p, C.c_long], None
    worst = 0.0
    for part, x in zip(("[0, 2 pi]", "(2 pi, 100]", "[-100, 0)"), D.set_sincos()):
        s, c = D.run("sincos_ac", x, device=False)
        xs = np.ascontiguousarray(D.f32(x))
        so, co = np.empty_like(xs), np.empty_like(xs)
        L.orc_sincos_n(xs.ctypes.data_as(f32p), so.ctypes.data_as(f32p), co.ctypes.data_as(f32p), len(xs))      # every point of the set
        D.assert_same("sincos_ac against orc_sincos, " + part, [s, c], [D.bits(so), D.bits(co)], (x,))
        x64 = xs.astype(np.float64)
        err = np.maximum(np.abs(D.f32(s).astype(np.float64) - np.sin(x64)), np.abs(D.f32(c).astype(np.float64) - np.cos(x64)))
        print("sincos_ac: max absolute error against binary64 %.3g on %s (%d points, worst at 0x%08x)" % (err.max(), part, len(x), int(x[np.argmax(err)])))
        worst = max(worst, err.max())
    assert worst < 2e-7


def test_pow22_host_twin_gives_the_golden_values_and_glibc_is_correctly_rounded_there():
    doc = D.pow22_hard()
    rows = doc["inputs"]
    x = np.array([int(r["x"], 16) for r in rows], D.U32)
    got = D.run("pow22", x, device=False)
    unit = [r for r in rows if int(r["x"], 16) <= 0x3f800000]
    assert len(unit) == 34                                                        # the scan of (0, 1]
    assert sorted(r["x"] for r in rows if r["dist"] <= 1 and int(r["x"], 16) <= 0x3f800000) == ["0x244429fd", "0x2a392c2a", "0x3947403d", "0x3e22373b"]
    for r, g in zip(rows, got):
        assert "0x%08x" % int(g) == r["glibc"], (r, hex(int(g)))                  # this machine's glibc
        assert r["glibc"] == r["exact"], r                                        # ... which is the correctly rounded value
    # the six closest inputs against mpmath, recomputed here
    import mpmath
    mpmath.mp.prec = 240
    closest = sorted(rows, key=lambda r: r["dist_exact"])[:6]
    for r in closest:
        xv = float(D.f32(np.array([int(r["x"], 16)], D.U32))[0])
        y = mpmath.power(mpmath.mpf(xv), mpmath.mpf(float(np.float32(2.2))))
        assert D.round_to_f32(Fraction(int(y.man)) * Fraction(2) ** int(y.exp)) == int(r["glibc"], 16), r


# the first 16 hex digits of the SHA-256 of each set's bytes (devarith_helpers.all_sets)
SET_HASHES = {
    "U": "f67b57ce159a0f6e", "P": "5f7c61610391a1c5", "T": "dcd4ae184b2285da", "sincos": "35c516ef7da5b415", "exp": "6b0fdb89aa4c2bd1", "atan2": "ebc7aac565a96e52",
    "childkey": "dc11075c4f671c7d", "tex": "fb25cb91644f544f",
}


def test_input_sets_are_deterministic():
    sets = D.all_sets()
    got = {k: D.set_hash(*sets[k]) for k in SET_HASHES}
    print(got)
    assert got == SET_HASHES
    assert len(D.set_U()) == 2 * 256 * 64 + (1 << 21) + 6 and len(D.set_P()[0]) == 1 << 22 and len(D.set_T()[0]) == 64 ** 3 + (1 << 20)
