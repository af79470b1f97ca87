"""The arithmetic contract tests' helpers: bindings of tests/devarith/libdevarith.so (every primitive of pt_math.h's contract as a kernel of
its own and as a host function from the same headers), the input sets, and exact references.

The comparison rule, stated once (mismatches()): results are compared as BITS; two NaNs count as equal whatever their payload (the x86 and
AMD default NaNs differ in sign); min and max are compared as values where both operands are zeros of opposite sign (zero_pair()).

Every set is a pure function of fixed seeds: SET_HASHES pins their bytes (tests/test_devarith_cpu.py)."""
import ctypes as C
import functools
import decimal
import hashlib
import json
import math
import os
import subprocess
from fractions import Fraction

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DIR = os.path.join(REPO, "tests", "devarith")
_lib = None

U32 = np.uint32


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("DEVARITH_LIB", os.path.join(_DIR, "libdevarith.so"))
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", REPO, "-s", "devarith"])
        L = C.CDLL(path)
        f32p = C.POINTER(C.c_float)
        for side in ("dev", "host"):
            f = getattr(L, "da_%s_run" % side); f.argtypes, f.restype = [C.c_char_p, f32p, f32p, C.c_long], C.c_int
            f = getattr(L, "da_%s_arity" % side); f.argtypes, f.restype = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int
            f = getattr(L, "da_%s_tex2d" % side); f.argtypes, f.restype = [f32p, C.c_int, C.c_int, f32p, f32p, C.c_long], C.c_int
        L.da_host_pow22_scan.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.c_long]
        L.da_host_pow22_scan.restype = C.c_long
        _lib = L
    return _lib


def bits(a):
    """Any float32 / uint32 / int32 array as uint32 bit patterns."""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return np.ascontiguousarray(a).view(U32)
    return np.ascontiguousarray(a.astype(U32, copy=False) if a.dtype in (np.uint32, np.int32) else a, U32)


def f32(a):
    """uint32 bit patterns (or floats) as float32 values."""
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.float32) if a.dtype in (np.uint32, np.int32) else np.ascontiguousarray(a, np.float32)


def run(name, *operands, device, sweep=False):
    """One primitive of devarith_ops.h over arrays of operands (bit patterns or float32), on the device (one launch) or on the host twin.
    Returns the outputs as uint32 bit patterns, one array per output (a single array when there is one).  sweep: tools/devarith_sweep.py,
    the one caller that is not a test."""
    L = lib()
    side = "dev" if device else "host"
    nin, nout = C.c_int(), C.c_int()
    assert getattr(L, "da_%s_arity" % side)(name.encode(), C.byref(nin), C.byref(nout)) == 0, "no primitive %r on the %s side" % (name, side)
    assert len(operands) == nin.value, (name, len(operands), nin.value)
    ops = np.ascontiguousarray(np.stack([bits(o) for o in operands]))
    n = ops.shape[1]
    assert n <= 1 << 22 or not device or sweep, "a GPU test moves at most 2^22 elements"
    out = np.empty((nout.value, n), U32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = getattr(L, "da_%s_run" % side)(name.encode(), fp(ops), fp(out), n)
    assert rc == 0, "%s on the %s side: error %d" % (name, side, rc)
    return out[0] if nout.value == 1 else list(out)


def tex2d(tex, u, v, device):
    """pt::tex2d of an [h, w, 4] float32 texture at (u, v): [n, 4] bit patterns."""
    tex = np.ascontiguousarray(tex, np.float32)
    uv = np.ascontiguousarray(np.stack([f32(u), f32(v)]))
    n = uv.shape[1]
    out = np.empty((4, n), U32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    f = lib().da_dev_tex2d if device else lib().da_host_tex2d
    rc = f(fp(tex), tex.shape[1], tex.shape[0], fp(uv), fp(out), n)
    assert rc == 0, "tex2d: error %d" % rc
    return np.ascontiguousarray(out.T)


def is_nan(b):
    b = bits(b)
    return (b & U32(0x7fffffff)) > U32(0x7f800000)


def is_quiet_or_number(b):
    """not a signalling NaN"""
    b = bits(b)
    return ~(is_nan(b) & ((b & U32(0x00400000)) == 0))


def is_finite(b):
    return (bits(b) & U32(0x7f800000)) != U32(0x7f800000)


def is_normal_or_zero(b):
    e = bits(b) & U32(0x7f800000)
    return ((e != 0) & (e != U32(0x7f800000))) | ((bits(b) & U32(0x7fffffff)) == 0)


def is_normal(b):
    e = bits(b) & U32(0x7f800000)
    return (e != 0) & (e != U32(0x7f800000))


def zero_pair(a, b):
    """both operands zeros of opposite sign: min / max may return either (compared as values)"""
    a, b = bits(a), bits(b)
    return ((a | b) == U32(0x80000000)) & ((a & b) == 0)


def mismatches(got, want, free=None):
    """Indices where got and want differ under the comparison rule; `free`: a mask of elements compared as values (zeros of either sign)."""
    got, want = bits(got), bits(want)
    ok = (got == want) | (is_nan(got) & is_nan(want))
    if free is not None:
        ok |= free & (f32(got) == f32(want))
    return np.nonzero(~ok)[0]


def report(name, bad, operands, got, want, limit=8):
    """The assertion message of a comparison: how many, and the first few with every operand's bits."""
    rows = ["%s: %d mismatches; first %d (operand bits -> got, want):" % (name, len(bad), min(limit, len(bad)))]
    for i in bad[:limit]:
        rows.append("  " + " ".join("0x%08x" % int(bits(o)[i]) for o in operands) + " -> 0x%08x, 0x%08x" % (int(bits(got)[i]), int(bits(want)[i])))
    return "\n".join(rows)


def assert_same(name, got, want, operands, free=None, mask=None):
    """mask: compare only there (the documented range of a primitive)."""
    got, want = np.atleast_2d(np.stack(got) if isinstance(got, list) else got), np.atleast_2d(np.stack(want) if isinstance(want, list) else want)
    for k in range(got.shape[0]):
        bad = mismatches(got[k], want[k], free)
        if mask is not None:
            bad = bad[mask[bad]]
        assert len(bad) == 0, report("%s[%d]" % (name, k), bad, operands, got[k], want[k])


# ------------------------------------------------------------------------------------------------ exact references
def round_to_f32(q):
    """Exact round-to-nearest-even of a rational to binary32, gradual underflow and overflow included: the bit pattern.  A zero result
    is +0 (the sign of an exact zero depends on the operation, not on its value: callers compare zeros as values)."""
    q = Fraction(q)
    if q == 0:
        return 0
    sign = 0x80000000 if q < 0 else 0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()            # 2^e <= q < 2^(e+1), up to one
    if (Fraction(1 << e) if e >= 0 else Fraction(1, 1 << -e)) > q:
        e -= 1
    e = max(e, -126)                                                      # below FLT_MIN the spacing stays 2^-149
    scaled = q * (1 << (23 - e)) if e <= 23 else q / (1 << (e - 23))      # in units of the spacing 2^(e-23)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    b = ((e + 126) << 23) + n                                             # n carries the implicit bit (and a carry into the exponent)
    return sign | min(b, 0x7f800000)


def frac(b):
    """The exact value of a finite binary32 bit pattern."""
    b = int(b)
    e, m = (b >> 23) & 0xff, b & 0x7fffff
    assert e != 0xff
    v = Fraction(m + (1 << 23), 1) * Fraction(2) ** (e - 150) if e else Fraction(m, 1) * Fraction(2) ** -149
    return -v if b >> 31 else v


def rnd(q):
    """fl(q) as a Fraction: one binary32 operation's result, for chains (dot, cross, lerp)."""
    return frac(round_to_f32(q))


def sqrt_round_to_f32(b):
    """Correctly rounded square root of a positive finite binary32, from integers alone."""
    q = frac(b)
    # q = num / den; scale to an integer with plenty of bits: isqrt(q * 4^k), whose root has >= 125 bits for every q >= 2^-149
    k = 200
    num = q.numerator << (2 * k)
    s = num // q.denominator
    r = math.isqrt(s)
    exact = (r * r == s) and (num % q.denominator == 0)
    # the root lies in [r, r + 1) / 2^k; with >= 40 bits in r, no binary32 boundary lies strictly inside, so any point of the open
    # interval rounds as the root does
    return round_to_f32(Fraction(r, 1 << k) if exact else Fraction(2 * r + 1, 2 << k))


def exact_subset(mask, count=4096, seed=99):
    """`count` indices where mask holds (finite operands), a fixed pseudo-random choice."""
    idx = np.nonzero(mask)[0]
    rng = np.random.RandomState(seed)
    return np.sort(rng.choice(idx, size=min(count, len(idx)), replace=False))


def assert_exact(name, got, operands, idx, fn):
    """got[idx] equals round_to_f32(fn(*exact operands)); exact zeros are compared as values."""
    got = bits(got)
    bad = []
    for i in idx:
        want = fn(*[frac(bits(o)[i]) for o in operands])
        want = want if isinstance(want, int) else round_to_f32(want)
        g = int(got[i])
        if g != want and not ((want & 0x7fffffff) == 0 and (g & 0x7fffffff) == 0):
            bad.append((i, want))
    assert not bad, "%s: %d of %d differ from the exact value; first: %s" % (name, len(bad), len(idx), "; ".join(
        " ".join("0x%08x" % int(bits(o)[i]) for o in operands) + " -> 0x%08x, exact 0x%08x" % (int(got[i]), w) for i, w in bad[:6]))


# ------------------------------------------------------------------------------------------------ input sets
def _mk(sign, exp, mant):
    return (np.asarray(sign, np.uint64) << 31 | np.asarray(exp, np.uint64) << 23 | np.asarray(mant, np.uint64)).astype(U32)


def _rand_bits(rng, n):
    return rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(U32)


def _rand_exp_range(rng, n, lo, hi):
    """random sign and mantissa, unbiased exponent uniform in [lo, hi]"""
    return _mk(rng.randint(0, 2, n), rng.randint(lo + 127, hi + 128, n), rng.randint(0, 1 << 23, n))


SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001], U32)      # +-0, +-inf, two quiet NaNs


@functools.lru_cache(None)
def set_U():
    """Unary set: every sign and exponent with 8 edge mantissas and 56 fixed pseudo-random ones, 2^21 random patterns, the specials."""
    rng = np.random.RandomState(2701)
    mant = np.concatenate([[0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff], rng.randint(0, 1 << 23, 56)])
    s, e, m = np.meshgrid(np.arange(2), np.arange(256), mant, indexing="ij")
    out = np.concatenate([_mk(s.ravel(), e.ravel(), m.ravel()), _rand_bits(rng, 1 << 21), SPECIALS])
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def set_S():
    s, e, m = np.meshgrid(np.arange(2), np.arange(256), [0, 1, 0x7fffff], indexing="ij")
    return _mk(s.ravel(), e.ravel(), m.ravel())


@functools.lru_cache(None)
def set_P():
    """Pairs: S x S (1,536 values: sign x exponent x mantissa in {0, 1, 0x7fffff}), 2^20 random pairs, 2^19 pairs (fl(q b), b) whose
    quotients lie next to representable values, 2^18 pairs with subnormal quotients: 2^22 pairs."""
    rng = np.random.RandomState(2702)
    S = set_S()
    a0, b0 = [x.ravel() for x in np.meshgrid(S, S, indexing="ij")]
    a1, b1 = _rand_bits(rng, 1 << 20), _rand_bits(rng, 1 << 20)
    q = f32(_rand_exp_range(rng, 1 << 19, -40, 40)); b2 = f32(_rand_exp_range(rng, 1 << 19, -40, 40))
    a2 = (q * b2).astype(np.float32)
    qs = f32(_mk(rng.randint(0, 2, 1 << 18), 0, rng.randint(1, 1 << 23, 1 << 18)))          # a subnormal quotient
    b3 = f32(_rand_exp_range(rng, 1 << 18, 30, 100))
    a3 = (qs.astype(np.float64) * b3.astype(np.float64)).astype(np.float32)                   # normal: >= 2^-149 * 2^30
    a = np.concatenate([a0, a1, bits(a2), bits(a3)]); b = np.concatenate([b0, b1, bits(b2), bits(b3)])
    assert len(a) == 1 << 22
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(None)
def set_T():
    """Triples: 64^3 special values, 2^19 random triples, 2^19 cancellation triples (a, b, -fl(a b)) whose fma is the product's exact
    rounding error, subnormal errors included."""
    rng = np.random.RandomState(2703)
    pos = [0x00000000, 0x00000001, 0x00000002, 0x00400000, 0x007fffff, 0x00800000, 0x00800001, 0x00ffffff, 0x0d800000, 0x1f800000,
           0x1fec1e4a, 0x33800000, 0x34000000, 0x3f000000, 0x3f7fffff, 0x3f800000, 0x3f800001, 0x3fffffff, 0x40000000, 0x40400000,
           0x4b000000, 0x4b7fffff, 0x4b800000, 0x4f000000, 0x5f800000, 0x5f7fffff, 0x60ad78ec, 0x7e800000, 0x7f000000, 0x7f7ffffe,
           0x7f7fffff]
    sp = np.array(pos + [p | 0x80000000 for p in pos] + [0x7f800000, 0x7fc00000], U32)
    assert len(sp) == 64
    a0, b0, c0 = [x.ravel() for x in np.meshgrid(sp, sp, sp, indexing="ij")]
    n = 1 << 19
    a1, b1, c1 = [np.concatenate([_rand_bits(rng, n // 2), _rand_exp_range(rng, n // 2, -30, 30)]) for _ in range(3)]
    a2 = _rand_exp_range(rng, n, -75, 40); b2 = _rand_exp_range(rng, n, -75, 40)
    c2 = bits(-(f32(a2) * f32(b2)).astype(np.float32))
    out = tuple(np.concatenate(x) for x in ((a0, a1, a2), (b0, b1, b2), (c0, c1, c2)))
    for x in out:
        x.setflags(write=False)
    return out


def _near(values, ulps=64):
    """every float within `ulps` binary32 ulps (bit-pattern steps) of each value; around zero: +0, -0 and both signs' neighbours"""
    out = []
    for v in values:
        b = int(bits(np.float32(v)).reshape(-1)[0])
        if b & 0x7fffffff == 0:
            out.append(0x80000000)
        for d in range(-ulps, ulps + 1):
            if b & 0x7fffffff or d >= 0:
                out.append((b + d) & 0xffffffff)                  # one sign's patterns are consecutive
            else:
                out.append(0x80000000 | (-d))                     # below +0: -0's neighbours
    return np.array(out, U32)


def _stratified(rng, n, lo, hi):
    """one binary32 point in each of n equal strata of [lo, hi]"""
    x = lo + (np.arange(n) + rng.random_sample(n)) * ((hi - lo) / n)
    return np.clip(x, lo, hi).astype(np.float32)


SINCOS_WORST = np.array([0x3f4d56a3, 0x40175ae2], U32)      # the largest errors of a CPU scan of [0, 2 pi] against binary64


@functools.lru_cache(None)
def set_sincos():
    """|x| <= 100, the range pt_math.h documents, in three parts of at most 2^22 elements:
      [0, 2 pi]     every float within 64 ulps of k pi / 4 (k = 0..8; around 0: -0 and the negative neighbours too), the two worst points,
                    2^21 stratified points -- what the path tracer calls it with
      (2 pi, 100]   2^21 stratified points
      [-100, 0)     every float within 64 ulps of -k pi / 4 (k = 1..8), 2^21 stratified points: the floor of a negative product, a negative
                    quadrant number"""
    rng = np.random.RandomState(2704)
    two_pi = 2 * np.pi
    parts = (np.concatenate([_near([k * np.pi / 4 for k in range(9)]), SINCOS_WORST, bits(_stratified(rng, 1 << 21, 0.0, two_pi))]),
             bits(_stratified(rng, 1 << 21, float(np.nextafter(np.float32(two_pi), np.float32(100))), 100.0)),
             np.concatenate([_near([-k * np.pi / 4 for k in range(1, 9)]), bits(_stratified(rng, 1 << 21, -100.0, float(np.float32(-1e-45))))]))
    for x in parts:
        x.setflags(write=False)
    return parts


@functools.lru_cache(None)
def set_exp():
    """every float within 64 ulps of -87, 0, 88 and of (k + 1/2) ln 2 for k = -126..127 (where the reduction's k changes), and 2^20
    stratified points of [-100, 100] (both cut-offs inside)."""
    rng = np.random.RandomState(2705)
    out = np.concatenate([_near([-87.0, 0.0, 88.0] + [(k + 0.5) * np.log(2.0) for k in range(-126, 128)]),
                          bits(_stratified(rng, 1 << 20, -100.0, 100.0))])
    out.setflags(write=False)
    return out


@functools.lru_cache(None)
def set_atan2():
    """the grid of tests/test_sign_cpu.py: 361 magnitudes 1e-6 .. 1e3 log-uniform (10^(k / 40), k = -240..120) in both arguments, both
    signs of x, y = 0, x = 0, y = x.  The magnitudes are 10^(k / 40) to 40 decimal digits rounded once to binary32 -- no libm, so the
    bytes are the same everywhere."""
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        m = np.array([float(decimal.Decimal(10) ** (decimal.Decimal(k) / 40)) for k in range(-240, 121)], np.float64).astype(np.float32)
    y, x = [a.reshape(-1) for a in np.meshgrid(m, m)]
    y = np.concatenate([y, y, np.zeros_like(m), np.zeros_like(m), m, m, m]).astype(np.float32)
    x = np.concatenate([x, -x, m, -m, np.zeros_like(m), m, -m]).astype(np.float32)
    return bits(y), bits(x)


@functools.lru_cache(None)
def set_childkey():
    """2^18 quadruples of (entry distance, child reference) for the node step's sort: t > 0 normal, t = tmin = 1e-3, equal t with
    different refs, t subnormal and +0, t = kFar; refs 0, 1, 0x7fffffff and negative leaf refs."""
    rng = np.random.RandomState(2706)
    n = 1 << 18
    tpool = np.concatenate([bits(np.float32([1e-3, 3.0e38, 1.0, 1e-3, 1e-3])), np.array([0, 1, 2, 0x7fffff, 0x400000, 0x00800000], U32)])
    kind = rng.randint(0, 4, (4, n))
    t_rand = _mk(0, rng.randint(1, 255, (4, n)), rng.randint(0, 1 << 23, (4, n)))              # positive normal
    t_pool = tpool[rng.randint(0, len(tpool), (4, n))]
    t_near = (t_rand[0][None, :] + rng.randint(0, 3, (4, n)).astype(U32)).astype(U32)            # equal or adjacent distances
    t_near = np.where(is_normal(t_near), t_near, t_rand)
    t = np.where(kind == 0, t_rand, np.where(kind == 1, t_pool, t_near)).astype(U32)
    t = np.where(kind == 3, t[0][None, :], t).astype(U32)                                        # all four equal: the refs decide
    rpool = np.array([0, 1, 2, 0x7fffffff, 0xffffffff, 0x80000000, 0xfffffff7, 0x7ffffffe], U32)
    r = np.where(rng.randint(0, 2, (4, n)) == 0, rpool[rng.randint(0, len(rpool), (4, n))], _rand_bits(rng, 4 * n).reshape(4, n)).astype(U32)
    out = np.ascontiguousarray(np.concatenate([t, r]))
    out.setflags(write=False)
    return out


TEX_SIZES = ((1, 1), (1, 5), (7, 3), (8, 8), (32, 24))      # width, height


def texture(w, h):
    return np.random.RandomState(2707 + 100 * w + h).random_sample((h, w, 4)).astype(np.float32)


@functools.lru_cache(None)
def tex_coords(w, h):
    """(u, v) for a w x h texture: texel centres, centre +- 1/512 and +- 1/1024 of a texel, 0, -0, +-1e-9, k + {0, 1/2}, +-1e6, +-1e30
    (all finite), 2^18 random in [-4, 4]."""
    rng = np.random.RandomState(2708 + 100 * w + h)

    def axis(n):
        c = (np.arange(n) + 0.5) / n
        off = np.array([0.0, 1 / 512, -1 / 512, 1 / 1024, -1 / 1024]) / n
        pts = np.concatenate([(c[:, None] + off[None, :]).ravel(), [0.0, -0.0, 1e-9, -1e-9], np.arange(-3, 4) + 0.0, np.arange(-3, 4) + 0.5,
                              [1e6, -1e6, 1e30, -1e30]])
        return pts.astype(np.float32)
    au, av = axis(w), axis(h)
    u0, v0 = [x.ravel() for x in np.meshgrid(au, av, indexing="ij")]
    u1 = rng.uniform(-4, 4, 1 << 18).astype(np.float32); v1 = rng.uniform(-4, 4, 1 << 18).astype(np.float32)
    return np.concatenate([u0, u1]), np.concatenate([v0, v1])


TEX_NONFINITE = np.array([np.inf, -np.inf, np.nan, 0.25], np.float32)      # out of the contract: the call returns, nothing is compared


# ------------------------------------------------------------------------------------------------ pow22 (AC6)
POW22_GOLDEN = os.path.join(REPO, "tests", "golden", "pow22_hard.json")


def pow22_hard():
    with open(POW22_GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(None)
def set_pow22():
    """The inputs of the device comparison: the hard list, all k / 255, every t00 + ax (t10 - t00) for k / 255 pairs differing by <= 8 and
    all 257 weights (tex2d's interpolation of 8-bit texels), the inputs whose results straddle FLT_MIN and the least subnormal, 0, 1, 2,
    1e17, +inf, 2^21 stratified points of (0, 1], negative and NaN inputs."""
    rng = np.random.RandomState(2709)
    hard = np.array([int(r["x"], 16) for r in pow22_hard()["inputs"]], U32)
    k = (np.arange(256) / np.float32(255)).astype(np.float32)
    i, j = [x.ravel() for x in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
    keep = np.abs(i - j) <= 8
    t00, t10 = k[i[keep]], k[j[keep]]
    ax = (np.arange(257) * np.float32(1 / 256)).astype(np.float32)
    interp = (t00[:, None] + ax[None, :] * (t10 - t00)[:, None]).astype(np.float32).ravel()      # binary32 operations, as tex2d's
    # x^2.2 = FLT_MIN at x = 2^(-126 / 2.2), = 2^-149 at 2^(-149 / 2.2), rounds to zero below 2^(-150 / 2.2)
    edges = _near([2.0 ** (-126 / 2.2), 2.0 ** (-149 / 2.2), 2.0 ** (-150 / 2.2), 2.0 ** (-127 / 2.2)], 32)
    fixed = bits(np.float32([0.0, 1.0, 2.0, 1e17, np.inf, -1.0, -0.5, -np.inf, np.nan]))
    strat = _stratified(rng, 1 << 21, 0.0, 1.0)
    strat = np.where(strat == 0, np.float32(1.0), strat)
    out = np.concatenate([hard, bits(k), bits(interp), edges, fixed, np.array([0x80000001, 0xffc00000], U32), bits(strat)])
    out.setflags(write=False)
    return out


def set_hash(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def all_sets():
    """name -> arrays, for the determinism check"""
    tex = [c for w, h in TEX_SIZES for c in (texture(w, h),) + tex_coords(w, h)]
    return {"U": (set_U(),), "P": set_P(), "T": set_T(), "sincos": set_sincos(), "exp": (set_exp(),), "atan2": set_atan2(),
            "childkey": (set_childkey(),), "tex": tuple(tex)}
