"""The arithmetic contract on the device, one primitive at a time.

Every "bit for bit the CPU mirror" test of this suite takes for granted that + - x / sqrt fma, the conversions, floor and min / max are the
same correctly rounded binary32 operations on the MI355X and on the host, and that the specified algorithms built from them (sincos_ac,
exp_ac, pow_int_ac, atan2_ac, tex2d, the node step's key sort) therefore give the same bits.  Here each primitive runs ALONE in a kernel of
tests/devarith/devarith.hip -- the product headers' own function, compiled with the product's flags -- over input sets chosen for where
such operations go wrong (devarith_helpers.py), and is compared with the same function compiled for the host (the twin), with binary64
arithmetic rounded once, and with exact rational values on a subset.  The comparison rule is devarith_helpers.mismatches: bits, NaNs equal
whatever their payload, zeros of opposite sign free for min / max.

The limit of these tests: the kernels are the headers' functions compiled alone, not the product kernels' instruction streams.  They pin
the primitives; the render and query tests pin the kernels.

Out of the contract, and so not compared: sincos_ac beyond |x| <= 100 (no caller leaves [0, 2 pi]), (int) conversions of |x| >= 2^31, and
tex2d with non-finite coordinates, for which only the return of the call is asserted (tex_wrap keeps every index in range for any int).
Signalling NaNs are no value any operation of the contract produces; fminf_ / fmaxf_ / clampf are compared on them like on every other
operand (a NaN operand is missing, on both sides), the lean forms on their stated domain."""
from fractions import Fraction

import ctypes as C
import numpy as np
import pytest

import devarith_helpers as D
from common import O

pytestmark = pytest.mark.gpu
U32 = np.uint32


def both(name, *ops):
    return D.run(name, *ops, device=True), D.run(name, *ops, device=False)


def vec_inputs():
    """Six / seven operand arrays from the triples: a = (Ta, Tb, Tc), b and t the same arrays displaced against each other."""
    a, b, c = D.set_T()
    return (a, b, c, np.roll(b, 1), np.roll(c, 7), np.roll(a, 13), np.roll(b, 29))


def finite_all(*arrays):
    return np.logical_and.reduce([D.is_finite(x) for x in arrays])


def rnd_chain_ok(got, ops):
    """where an exact chain of roundings can be followed: finite operands and a finite result (an overflowing intermediate ends non-finite)"""
    return finite_all(*ops) & D.is_finite(got)


def f64(b):
    with np.errstate(invalid="ignore"):                     # a signalling NaN is quieted by the conversion
        return D.f32(b).astype(np.float64)


def to_f32_bits(x64):
    """binary64 -> binary32, round to nearest even (numpy's cast), as bits"""
    with np.errstate(all="ignore"):
        return D.bits(x64.astype(np.float32))


# ------------------------------------------------------------------------------------------------ + - x fma and the fused forms
@pytest.mark.parametrize("name", ["add", "sub", "mul"])
def test_add_sub_mul(name):
    a, b = D.set_P()
    dev, host = both(name, a, b)
    D.assert_same(name, dev, host, (a, b))
    fn = {"add": lambda x, y: x + y, "sub": lambda x, y: x - y, "mul": lambda x, y: x * y}[name]
    D.assert_exact(name, dev, (a, b), D.exact_subset(finite_all(a, b)), fn)


def test_fma_and_lerp():
    a, b, c = D.set_T()
    dev, host = both("fma", a, b, c)
    D.assert_same("fma_", dev, host, (a, b, c))
    fin = finite_all(a, b, c)
    n = len(a)
    idx = np.concatenate([D.exact_subset(fin, 2048), D.exact_subset(fin & (np.arange(n) >= n - (1 << 19)), 2048, seed=7)])      # the cancellation triples
    D.assert_exact("fma_", dev, (a, b, c), idx, lambda x, y, z: x * y + z)
    dev, host = both("lerp", a, b, c)
    D.assert_same("lerp", dev, host, (a, b, c))
    D.assert_exact("lerp", dev, (a, b, c), D.exact_subset(rnd_chain_ok(dev, (a, b, c))), lambda x, y, t: x + D.rnd(t * D.rnd(y - x)))


def test_dot_cross_ray_at_lerp3():
    v = vec_inputs()
    six = v[:6]
    dev, host = both("dot", *six)
    D.assert_same("dot", dev, host, six)
    D.assert_exact("dot (AC1)", dev, six, D.exact_subset(rnd_chain_ok(dev, six)),
                   lambda ax, ay, az, bx, by, bz: az * bz + D.rnd(ay * by + D.rnd(ax * bx)))
    dev, host = both("cross", *six)
    D.assert_same("cross", dev, host, six)
    ok = rnd_chain_ok(dev[0], six) & D.is_finite(dev[1]) & D.is_finite(dev[2])
    idx = D.exact_subset(ok)
    D.assert_exact("cross.x (AC2)", dev[0], six, idx, lambda ax, ay, az, bx, by, bz: ay * bz - D.rnd(az * by))
    D.assert_exact("cross.y (AC2)", dev[1], six, idx, lambda ax, ay, az, bx, by, bz: az * bx - D.rnd(ax * bz))
    D.assert_exact("cross.z (AC2)", dev[2], six, idx, lambda ax, ay, az, bx, by, bz: ax * by - D.rnd(ay * bx))
    dev, host = both("ray_at", *v)
    D.assert_same("ray_at", dev, host, v)
    D.assert_exact("ray_at.x (AC7)", dev[0], v, D.exact_subset(finite_all(*v)), lambda ox, oy, oz, dx, dy, dz, t: t * dx + ox)
    dev, host = both("lerp3", *v)
    D.assert_same("lerp3", dev, host, v)
    D.assert_exact("lerp(v3).y", dev[1], v, D.exact_subset(rnd_chain_ok(dev[1], v)), lambda ax, ay, az, bx, by, bz, t: ay + D.rnd(D.rnd(by - ay) * t))


# ------------------------------------------------------------------------------------------------ / 1/x sqrt and what is built from them
def test_division():
    a, b = D.set_P()
    dev, host = both("div", a, b)
    D.assert_same("a / b", dev, host, (a, b))
    with np.errstate(all="ignore"):
        want = to_f32_bits(f64(a) / f64(b))                  # innocuous double rounding: 53 >= 2 * 24 + 2
    D.assert_same("a / b against binary64", dev, want, (a, b))
    fin = finite_all(a, b) & ((b & U32(0x7fffffff)) != 0)
    n = len(a)
    idx = np.concatenate([D.exact_subset(fin, 2048), D.exact_subset(fin & (np.arange(n) >= n - (1 << 19)), 2048, seed=7)])      # the hard direction, subnormal quotients
    D.assert_exact("a / b", dev, (a, b), idx, lambda x, y: x / y)
    sub = ~D.is_normal_or_zero(dev) & D.is_finite(dev)
    assert sub.sum() >= 1 << 17                              # gradual underflow is part of the contract: subnormal quotients were compared


def test_reciprocal_sqrt_slab_inv():
    x = D.set_U()
    dev, host = both("rcp", x)
    D.assert_same("1.0f / x", dev, host, (x,))
    with np.errstate(all="ignore"):
        D.assert_same("1.0f / x against binary64", dev, to_f32_bits(1.0 / f64(x)), (x,))
    D.assert_exact("1.0f / x", dev, (x,), D.exact_subset(D.is_finite(x) & ((x & U32(0x7fffffff)) != 0)), lambda v: 1 / v)
    dev, host = both("sqrt", x)
    D.assert_same("sqrtf", dev, host, (x,))
    with np.errstate(all="ignore"):
        D.assert_same("sqrtf against binary64", dev, to_f32_bits(np.sqrt(f64(x))), (x,))
    idx = D.exact_subset(D.is_finite(x) & ((x >> 31) == 0) & (x != 0))
    bad = [hex(int(x[i])) for i in idx if D.sqrt_round_to_f32(x[i]) != int(dev[i])]
    assert not bad, "sqrtf differs from the exact root at %s" % bad[:8]
    dev, host = both("slab_inv", x)
    D.assert_same("slab_inv", dev, host, (x,))
    with np.errstate(all="ignore"):
        d = f64(x)
        k = np.float64(np.float32(1e-19))
        D.assert_same("slab_inv against binary64", dev, to_f32_bits(1.0 / np.where(np.abs(d) < k, np.copysign(k, d), d)), (x,))


def test_length_normalize_v3_over_scalar():
    a, b, c, s = vec_inputs()[:4]
    s = D.set_U()[: len(a)]                                  # the scalar of v / s: every exponent, subnormals included
    dot = D.run("dot", a, b, c, a, b, c, device=True)
    dev, host = both("length", a, b, c)
    D.assert_same("length", dev, host, (a, b, c))
    with np.errstate(all="ignore"):
        D.assert_same("length = sqrtf(dot) (AC3)", dev, to_f32_bits(np.sqrt(f64(dot))), (a, b, c))
        inv = to_f32_bits(1.0 / f64(to_f32_bits(np.sqrt(f64(dot)))))
    dev, host = both("normalize", a, b, c)
    D.assert_same("normalize", dev, host, (a, b, c))
    for k, comp in enumerate((a, b, c)):
        with np.errstate(all="ignore"):
            D.assert_same("normalize = v * (1 / sqrtf(dot)) (AC3)", dev[k], to_f32_bits(f64(comp) * f64(inv)), (a, b, c))
    dev, host = both("v3div", a, b, c, s)
    D.assert_same("v / s", dev, host, (a, b, c, s))
    with np.errstate(all="ignore"):
        inv = to_f32_bits(1.0 / f64(s))
        for k, comp in enumerate((a, b, c)):
            D.assert_same("v / s = v * (1 / s) (AC3)", dev[k], to_f32_bits(f64(comp) * f64(inv)), (a, b, c, s))


# ------------------------------------------------------------------------------------------------ conversions, floor, sign operations
def test_floor_conversions_sign_operations():
    x = D.set_U()
    in_range = np.abs(f64(x)) < 2.0 ** 31                    # (int)x is defined there alone; NaN compares false
    for name, mask in (("floor", None), ("bfloor", None), ("fabs", None), ("bits", None), ("int2f", None), ("f2int", in_range), ("f2int2f", in_range)):
        dev, host = both(name, x)
        D.assert_same(name, dev, host, (x,), mask=mask)
    dev = D.run("floor", x, device=True)
    with np.errstate(all="ignore"):
        D.assert_same("floorf against binary64", dev, to_f32_bits(np.floor(f64(x))), (x,))
    dev = D.run("f2int", x, device=True)
    want = np.trunc(f64(x)[in_range]).astype(np.int64).astype(np.int32).view(U32)
    assert np.array_equal(dev[in_range], want), "(int)x differs from truncation"
    dev = D.run("int2f", x, device=True)
    assert np.array_equal(dev, D.bits(x.view(np.int32).astype(np.float64).astype(np.float32))), "(float)(int) is not the correctly rounded value"
    a, b = D.set_P()
    dev, host = both("copysign", a, b)
    D.assert_same("copysignf", dev, host, (a, b))
    assert np.array_equal(dev, (a & U32(0x7fffffff)) | (b & U32(0x80000000)))


@pytest.mark.parametrize("chunk", range(4))
def test_rnd_over_all_states(chunk):
    """(float)lcg / 2^24 for every one of the 2^24 values the generator can return: the low 24 bits of the state decide them, bijectively."""
    s = np.arange(chunk << 22, (chunk + 1) << 22, dtype=np.uint64).astype(U32)
    if chunk == 3:
        s[-4096:] |= U32(0xff000000)                         # the high byte of the state changes the next state alone
    dev, host = both("rnd", s)
    D.assert_same("rnd", dev, host, (s,))
    nxt = (s.astype(np.uint64) * 1664525 + 1013904223) & 0xffffffff
    assert np.array_equal(dev[1], nxt.astype(U32))
    assert np.array_equal(D.f32(dev[0]).astype(np.float64), (nxt & 0xffffff).astype(np.float64) / 2.0 ** 24)      # exact: 24 bits


# ------------------------------------------------------------------------------------------------ min / max
def test_min_max_clamp_and_the_lean_forms():
    a, b = D.set_P()
    free = D.zero_pair(a, b)
    # the lean forms' domain, as their comment states it (pt_path.h): at most one NaN, a quiet one.  A raw v_min_f32 / v_max_f32 answers a
    # signalling NaN with a NaN where fminf_ / fmaxf_ answer with the other operand; neither tmin nor tbest is ever one.
    claim = D.is_quiet_or_number(a) & D.is_quiet_or_number(b) & ~(D.is_nan(a) & D.is_nan(b))
    snan = ~(D.is_quiet_or_number(a) & D.is_quiet_or_number(b))
    out, fails = {}, []
    for name in ("fmin", "fmax", "lean_min", "lean_max"):
        dev, host = both(name, a, b)
        out[name] = dev
        bad = D.mismatches(dev, host, free)
        print("%s: %d mismatches against the host twin over %d pairs (%d of them with a signalling NaN operand)" % (name, len(bad), len(a), snan[bad].sum()))
        if name.startswith("lean"):
            bad = bad[claim[bad]]
        if len(bad):
            fails.append(D.report(name, bad, (a, b), dev, host))
    pz, nz = np.array([0], U32), np.array([0x80000000], U32)
    for name in ("fmin", "fmax", "lean_min", "lean_max"):
        print("%s(+0, -0) = 0x%08x, %s(-0, +0) = 0x%08x on the device" % (name, D.run(name, pz, nz, device=True)[0], name, D.run(name, nz, pz, device=True)[0]))
    assert not fails, "\n".join(fails)
    for lean, full in (("lean_min", "fmin"), ("lean_max", "fmax")):
        bad = D.mismatches(out[lean], out[full], free)
        bad = bad[claim[bad]]
        assert len(bad) == 0, D.report("%s against %s on the device" % (lean, full), bad, (a, b), out[lean], out[full])
    x, lo, hi = D.set_T()
    dev, host = both("clamp", x, lo, hi)
    zeros = ((x & U32(0x7fffffff)) == 0).astype(int) + ((lo & U32(0x7fffffff)) == 0) + ((hi & U32(0x7fffffff)) == 0)
    D.assert_same("clampf", dev, host, (x, lo, hi), free=zeros >= 2)


# ------------------------------------------------------------------------------------------------ the node step's sort
def test_childkey_sort_is_the_integer_order():
    q = D.set_childkey()
    dev, host = both("childkey", *q)
    for k in range(8):
        bad = np.nonzero(dev[k] != host[k])[0]               # bits, no NaN rule: the keys are not arithmetic values
        assert len(bad) == 0, D.report("ChildKey output %d" % k, bad, list(q), dev[k], host[k])
    keys = np.sort((q[:4].astype(np.uint64) << 32) | q[4:].astype(np.uint64), axis=0)
    assert np.array_equal(np.stack(dev[:4]), (keys >> 32).astype(U32)) and np.array_equal(np.stack(dev[4:]), keys.astype(U32))
    flushed = (q[:4] == 0).any(axis=0)                       # a key whose high word is 0 is a binary64 subnormal: it came back whole
    assert flushed.sum() > 1000


# ------------------------------------------------------------------------------------------------ the specified algorithms
@pytest.mark.parametrize("part", range(3), ids=["0..2pi", "2pi..100", "-100..0"])
def test_sincos_ac(part):
    """[0, 2 pi], with the neighbourhoods of k pi / 4 (-0 and the negative neighbours of 0 among them) and the two worst points, is what
    the path tracer calls it with; (2 pi, 100] and [-100, 0) are the rest of the range pt_math.h documents -- on the negative side the
    floor of a negative product and a negative quadrant number.  Three launches: each moves at most 2^22 elements."""
    x = D.set_sincos()[part]
    dev, host = both("sincos_ac", x)
    D.assert_same("sincos_ac", dev, host, (x,))


def test_exp_ac_pow_int_ac_atan2_ac():
    x = np.concatenate([D.set_exp(), D.set_U()])
    dev, host = both("exp_ac", x)
    D.assert_same("exp_ac", dev, host, (x,))
    rng = np.random.RandomState(11)
    u = D.set_U()
    base = np.concatenate([u[: 2 * 256 * 64: 5], rng.choice(u, 1 << 14)])[: 1 << 14]
    xb, n = [v.ravel() for v in np.meshgrid(base, np.arange(1, 257, dtype=U32), indexing="ij")]
    dev, host = both("pow_int_ac", xb, n)
    D.assert_same("pow_int_ac", dev, host, (xb, n))
    y, xx = D.set_atan2()
    dev, host = both("atan2_ac", y, xx)
    D.assert_same("atan2_ac", dev, host, (y, xx))


def test_disney_color_constants():
    rng = np.random.RandomState(12)
    n = 1 << 18
    col = rng.random_sample((3, n)).astype(np.float32)
    col[:, :256] = 0.0                                        # Cdlum == 0: the tint is white
    col[:, 256:512] = np.float32(1e-42)                       # a subnormal luminance
    col[:, 512:768] = (rng.randint(0, 256, (3, 256)) / np.float32(255)).astype(np.float32)            # 8-bit texel values
    par = rng.random_sample((4, n)).astype(np.float32)
    par[:, ::7] = np.round(par[:, ::7])                       # the ends of the parameter ranges
    ops = tuple(col) + tuple(par)
    dev, host = both("disney_consts", *ops)
    D.assert_same("disney_color_constants", dev, host, ops)


# ------------------------------------------------------------------------------------------------ textures
@pytest.mark.parametrize("w,h", D.TEX_SIZES)
def test_tex2d(w, h):
    tex = D.texture(w, h)
    u, v = D.tex_coords(w, h)
    dev, host = D.tex2d(tex, u, v, device=True), D.tex2d(tex, u, v, device=False)
    bad = np.unique(D.mismatches(dev.ravel(), host.ravel()) // 4)
    assert len(bad) == 0, D.report("tex2d %dx%d (u v -> .x)" % (w, h), bad, (u, v), dev[:, 0], host[:, 0])
    if (w, h) == (32, 24):
        # the oracle's own sampler on the structured coordinates and a stride through the random ones
        t = O.OrcTexture(w, h, tex.ctypes.data_as(C.POINTER(C.c_float)))
        out = (C.c_float * 4)()
        n0 = len(u) - (1 << 18)
        for i in list(range(0, n0, 7)) + list(range(n0, len(u), 61)):
            O.lib().orc_tex2d(C.byref(t), float(u[i]), float(v[i]), out)
            got = D.bits(np.array(list(out), np.float32))
            assert len(D.mismatches(dev[i], got)) == 0, (float(u[i]), float(v[i]), dev[i], got)
    # out of the contract: non-finite coordinates.  The call returns; nothing is compared.
    uu, vv = [x.ravel() for x in np.meshgrid(D.TEX_NONFINITE, D.TEX_NONFINITE)]
    assert D.tex2d(tex, uu, vv, device=True).shape == (len(uu), 4)


# ------------------------------------------------------------------------------------------------ the hardware approximations
def _ulps(got, exact64):
    """|got - exact| in units of the binary32 spacing at the exact value"""
    with np.errstate(all="ignore"):
        return np.abs(f64(got) - exact64) / 2.0 ** (np.floor(np.log2(np.abs(exact64))) - 23)


def test_hardware_rcp_sqrt_rsq_are_within_one_ulp_and_node_inv_is_finite():
    """What fast_shading (pt_disney.h ShadeMath<true>), the WINDOW sphere prefilter (pt_path.h) and the packet kernel's node_inv
    (pt_lanestack.h) rely on: v_rcp_f32, v_sqrt_f32 and v_rsq_f32 are within 1 ulp of the exact value on normal inputs and results."""
    x = D.set_U()
    xv = f64(x)
    pos = D.is_normal(x) & ((x >> 31) == 0)
    with np.errstate(all="ignore"):
        cases = (("hw_rcp", D.is_normal(x), 1.0 / xv), ("hw_sqrt", pos, np.sqrt(xv)), ("hw_rsq", pos, 1.0 / np.sqrt(xv)))
    for name, ok, exact in cases:
        dev = D.run(name, x, device=True)
        with np.errstate(all="ignore"):
            ok = ok & D.is_normal(to_f32_bits(exact)) & D.is_normal(dev)
        err = _ulps(dev[ok], exact[ok])
        print("%s: max error %.4f ulp over %d normal inputs with normal results (worst input 0x%08x)" % (name, err.max(), ok.sum(), int(x[ok][np.argmax(err)])))
        assert err.max() <= 1.0
    dev = D.run("node_inv", x, device=True)
    slab = D.run("slab_inv", x, device=True)
    number = ~D.is_nan(x)
    assert D.is_finite(dev[number]).all(), "node_inv is not finite at 0x%08x" % int(x[number][~D.is_finite(dev[number])][0])
    assert np.array_equal(dev[number] >> 31, slab[number] >> 31), "node_inv and slab_inv differ in sign"
    # within 1 ulp of the exact reciprocal of the clamped operand (the binary64 reference of slab_inv), normal inputs and results
    with np.errstate(all="ignore"):
        k = np.float64(np.float32(1e-19))
        exact = 1.0 / np.where(np.abs(xv) < k, np.copysign(k, xv), xv)
        ok = number & (D.is_normal(x) | (np.abs(xv) < k)) & D.is_normal(to_f32_bits(exact)) & D.is_normal(dev)
    err = _ulps(dev[ok], exact[ok])
    print("node_inv: max error %.4f ulp over %d inputs with normal results (worst input 0x%08x)" % (err.max(), ok.sum(), int(x[ok][np.argmax(err)])))
    assert err.max() <= 1.0


# ------------------------------------------------------------------------------------------------ pow22 (AC6)
# Inputs on which the device library's binary64 pow and glibc's round to different binary32 values: bit pattern -> the device's value.
# Only inputs of tests/golden/pow22_hard.json whose distance from a rounding boundary is <= 2 binary64 ulps may stand here.
POW22_DEVICE_DIFFERS = {}


def test_pow22_device_equals_host():
    x = D.set_pow22()
    dev, host = both("pow22", x)
    bad = D.mismatches(dev, host)
    close = {int(r["x"], 16) for r in D.pow22_hard()["inputs"] if r["dist"] <= 2}
    seen = {}
    for i in bad:
        seen[int(x[i])] = int(dev[i])
    print("pow22: %d of %d inputs differ between the device's pow and glibc's: %s" % (
        len(seen), len(x), ", ".join("0x%08x -> device 0x%08x, host 0x%08x" % (k, v, int(host[np.nonzero(x == k)[0][0]])) for k, v in sorted(seen.items())[:16])))
    assert set(POW22_DEVICE_DIFFERS) <= close
    assert seen == POW22_DEVICE_DIFFERS, D.report("pow22", bad, (x,), dev, host)
    neg = ((x >> 31) == 1) & ((x & U32(0x7fffffff)) != 0) & D.is_finite(x) | D.is_nan(x)
    assert D.is_nan(dev[neg]).all() and neg.sum() >= 4        # negative and NaN inputs: NaN on both sides
