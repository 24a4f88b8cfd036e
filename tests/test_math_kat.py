"""Known answers for the arithmetic every other test takes for granted.

The render parity tests compare the device with the oracle on bits and the known-answer series compares it with float64 closed forms
through the host twin; both assume that hipcc's gfx950 build of include/ptrs_detmath.h and csrc/pt_vec.h returns the bits of g++'s
x86-64 build, and that those bits are the right ones.  Here both are asked directly, through the math probe (csrc/pt_probe.h
math_probe_row: the functions themselves, one call per row):
  - the transcendental stand-ins against tests/golden/math_kat.npz -- mpmath values rounded once to the binary32 grid, subnormal
    results on their own grid -- on each function's domain of use and at its edges: no argument left out;
  - / and sqrt_ against binary64 rounded once (safe for these two operations at 53 versus 24 bits), the other binary32 helpers against
    numpy binary32 arithmetic (no contraction) or Python integers;
  - the two cdf searches against a bisection of the same predicate;
  - Sobol' values against Python integers over data/sobol_tables.bin.
Every test body runs on the host twin (CPU); under -m gpu the same rows also run on the device -- one launch per op -- and every row
of every op, the out-of-domain ones included, must equal the twin's bit for bit (two NaNs count as equal).
"""
import bisect
import importlib
import importlib.util
import os

import numpy as np
import pytest

import twin
from conftest import ROOT

ptrs = importlib.import_module("pathtracer-rs_amd")
A = ptrs.abi

BACKENDS = ["twin", pytest.param("gpu", marks=pytest.mark.gpu)]
ONE_MINUS_EPS = np.float32(float.fromhex("0x1.fffffep-1"))
F32_MAX, F32_TINY, F32_MIN_NORMAL = np.float32(3.4028234663852886e38), np.float32(1.401298464324817e-45), np.float32(2.0 ** -126)
INF, NAN = np.float32(np.inf), np.float32(np.nan)

_spec = importlib.util.spec_from_file_location("make_math_kat", os.path.join(ROOT, "tests", "golden", "make_math_kat.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(gen.PATH) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(np.asarray(b, np.int64).astype(np.uint32)).view(np.float32)


def cat(*parts):
    """the parts end to end, each converted to binary32 on its own (a NaN's payload survives: no pass through binary64)"""
    return np.concatenate([np.asarray(q, np.float32).reshape(-1) for q in parts])


def same(a, b):
    """bit equality of two binary32 arrays, two NaNs counting as equal"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def probe(backend, op, cols):
    """One probe call: cols (n x k, k <= 16, zero padded) -> the twin's (n x 16).  On the gpu backend the device runs the same rows in
    one launch and every column of every row must equal the twin's (the counts are printed: pytest -s)."""
    cols = np.ascontiguousarray(cols, np.float32)
    cols = cols.reshape(len(cols), -1)
    rows = np.zeros((len(cols), A.PROBE_MATH_WIDTH), np.float32)
    rows[:, :cols.shape[1]] = cols
    out = twin.math_probe(op, rows)
    if backend == "gpu":
        dev = ptrs.probe_math(op, rows)
        bad = ~same(dev, out).all(axis=1)
        print("math probe op %d: %d rows on the device, %d differ from the twin" % (op, len(rows), bad.sum()))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError("op %d: device != twin in %d of %d rows; first: in %s device %s twin %s" % (
                op, bad.sum(), len(bad), [hex(v) for v in bits(rows[i])], [hex(v) for v in bits(dev[i])], [hex(v) for v in bits(out[i])]))
    return out


# ---- the transcendental stand-ins ------------------------------------------------------------------------------------------------
DETMATH = {"sin": A.MATH_SIN, "cos": A.MATH_COS, "sincos": A.MATH_SINCOS, "tan": A.MATH_TAN, "log": A.MATH_LOG, "log2": A.MATH_LOG2,
           "exp": A.MATH_EXP, "pow": A.MATH_POW, "atan2": A.MATH_ATAN2, "acos": A.MATH_ACOS}


def fixture_args(name, c99=False):
    """(arguments, expected bit patterns) of one fixture function; the regenerated grid must be the one the file was written for.
    c99: pow's expected bits as C99 has them everywhere, the header's documented restrictions not applied."""
    fx = fixture()
    args = gen.all_args(name, from_bits(fx[name + "_edge_x"]))
    assert np.array_equal(gen.digest(args), fx[name + "_sha"]), "the regenerated arguments of %s are not the fixture's" % name
    exp = gen.unplanes(fx[name + "_e"])
    assert len(exp) == len(args) >= gen.N_GRID + 30
    if name == "pow" and not c99:  # the rows the header documents as not C99's pow: listed in the fixture by value, held to the documented answer
        rx, c99, doc = fx["pow_restricted_x"], fx["pow_restricted_c99"], fx["pow_restricted_header"]
        at = np.flatnonzero((bits(args)[:, None, :] == rx[None, :, :]).all(axis=2).any(axis=1))
        assert len(at) == len(rx) == len(np.unique(rx, axis=0)) and np.array_equal(bits(args)[at], rx) and np.array_equal(exp[at], c99)
        assert (at >= gen.N_GRID).all() and (c99 != doc).all()
        x, y = args[at, 0], args[at, 1]
        assert (np.signbit(x) | ((x == 1) & np.isnan(y))).all()  # a negative base or -0, or pow(1, NaN): nothing a renderer raises
        exp = exp.copy()
        exp[at] = doc
    return args, exp


def assert_fixture(name, args, got, exp):
    """got == exp on every row (exp 0x7fc00000 stands for any NaN), but for the generator's listed near-tie"""
    got = np.ascontiguousarray(got, np.float32)
    ok = (bits(got) == exp) | (np.isnan(got) & (exp == 0x7FC00000))
    if name in gen.NEAR_TIES:
        ok |= (bits(args) == bits(np.array(gen.NEAR_TIES[name], np.float32))).all(axis=1)
    if not ok.all():
        i = int(np.flatnonzero(~ok)[0])
        raise AssertionError("%s: %d of %d differ from the fixture; first: args %s got %#x expected %#x" % (
            name, (~ok).sum(), len(ok), [float(v).hex() for v in args[i]], bits(got)[i], exp[i]))


@pytest.mark.parametrize("name", list(DETMATH))
@pytest.mark.parametrize("backend", BACKENDS)
def test_detmath_is_the_correctly_rounded_value(backend, name):
    """pt_*f == the exact value rounded once to binary32 at every fixture argument (domain of use and edges), none left out.  The
    arguments outside the domain of use (gen.extra_args: sin beyond 1e4, exp beyond 2, pow with y beyond 128) ride in the same launch;
    they are held to the twin's bits only, because there the header does not promise the correctly rounded value."""
    base = "sin" if name == "sincos" else name
    args, exp = fixture_args(base)
    rows = np.concatenate([args, gen.extra_args(base)])
    out = probe(backend, DETMATH[name], rows)[:len(args)]
    assert_fixture(base, args, out[:, 0], exp)
    if name == "sincos":
        cos_args, cos_exp = fixture_args("cos")
        assert np.array_equal(bits(args), bits(cos_args))  # sin's and cos's fixtures are for the same arguments
        assert_fixture("cos", args, out[:, 1], cos_exp)
    else:
        assert not bits(out[:, 1:]).any()


def test_fixture_is_what_mpmath_says():
    """Every edge argument and every 20th grid argument (5 %) recomputed with mpmath; and the rounding itself at the values where
    rounding to 24 bits first would go wrong (subnormal results) and at ties."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 300
    mpf = mpmath.mpf
    for name in gen.FUNCTIONS:
        args, exp = fixture_args(name, c99=True)
        idx = np.concatenate([np.arange(7, gen.N_GRID, 20), np.arange(gen.N_GRID, len(args))])
        got = np.array([gen.expected_bits(name, args[i]) for i in idx], np.uint32)
        assert np.array_equal(got, exp[idx]), name
    R = lambda v: gen.round_once(v, mpmath.mp)
    assert R(mpf(2) ** -149) == 1 and R(mpf(2) ** -150) == 0 and R(mpf(2) ** -150 * mpf("1.0000001")) == 1 and R(3 * mpf(2) ** -150) == 2
    assert R(-(mpf(2) ** -149) * mpf("2.5")) == 0x80000002 and R(mpf(2) ** -149 * mpf("3.5")) == 4  # ties to even on the subnormal grid
    assert R(mpf(2) ** -126 - mpf(2) ** -151) == 0x00800000 and R(mpf(2) ** -126 - mpf(2) ** -150) == 0x00800000 and R(mpf(2) ** -126 - 3 * mpf(2) ** -150) == 0x007FFFFE
    assert R(1 + mpf(2) ** -24) == 0x3F800000 and R(1 + 3 * mpf(2) ** -24) == 0x3F800002 and R(1 + mpf(2) ** -24 + mpf(2) ** -200) == 0x3F800001
    assert R(mpf(2) ** 128 - mpf(2) ** 103) == 0x7F800000 and R(mpf(2) ** 128 - mpf(2) ** 103 - 1) == 0x7F7FFFFF and R(mpf(0)) == 0


# ---- binary32 primitives ---------------------------------------------------------------------------------------------------------
EDGE_VALUES = np.array([0.0, -0.0, F32_TINY, -F32_TINY, 2.0 ** -140, F32_MIN_NORMAL, -F32_MIN_NORMAL, 2.0 ** -127, 2.0 ** -104, 2.0 ** -103, 2.0 ** -48,
                        2.0 ** -47, 1.0 / 3.0, 1.0, -1.0, 3.0, 0.1, 2.0 ** 47, 2.0 ** 48, 2.0 ** 96, 2.0 ** 126, 2.0 ** 127, F32_MAX, -F32_MAX, INF, -INF, NAN],
                       np.float32)


def _next_to_ties(rng, n):
    """(a, b) whose quotient is as close to a rounding tie as binary32 operands allow: for an odd 24-bit b and the quotient's scale s,
    a = (b +- 1) / 2 * 2^-s (mod b), so that a * 2^s / b = integer + 1/2 +- 1/(2b): within 2^-24 ulp of the tie, on either side."""
    rows = []
    while len(rows) < n:
        b = int(rng.integers(1 << 23, 1 << 24)) | 1
        for half in ((b + 1) // 2, (b - 1) // 2):
            for s in (23, 24):
                a = half * pow(2, -s, b) % b
                for a in (a, a + b):
                    if (1 << 23) <= a < (1 << 24) and (s == 24) == (a < b):
                        rows.append((a, b))
    ab = np.array(rows[:n], np.float64)
    scale = np.ldexp(1.0, rng.integers(-60, 60, (n, 2)))  # the same mantissas at other exponents, subnormal quotients among them
    sign = rng.choice([-1.0, 1.0], (n, 2))
    return np.concatenate([ab, ab * scale * sign, ab * np.array([2.0 ** -100, 2.0 ** 40])]).astype(np.float32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_division_and_sqrt_are_ieee(backend):
    """a / b and sqrt_ == the binary64 result rounded once to binary32: random bit patterns, every pair of edge values (subnormal
    operands and results, divisors outside div_shared3's window [2^-47, 2^48)), quotients next to ties, squares' neighbours."""
    rng = np.random.default_rng(11)
    rnd = from_bits(rng.integers(0, 1 << 32, (20000, 2)))
    small = from_bits(rng.integers(0, 1 << 24, (3000, 2)) | (rng.integers(0, 2, (3000, 2)) << 31))  # subnormal and tiny operands
    mixed = np.stack([small[:, 0], rnd[:3000, 1]], axis=1)
    sub_q = np.stack([rng.uniform(1, 2, 3000) * 2.0 ** rng.integers(-126, -100, 3000), rng.uniform(1, 2, 3000) * 2.0 ** rng.integers(0, 40, 3000)], axis=1).astype(np.float32)
    edges = np.array([(a, b) for a in EDGE_VALUES for b in EDGE_VALUES], np.float32)
    ab = np.concatenate([rnd, small, mixed, mixed[:, ::-1], sub_q, edges, _next_to_ties(rng, 2000)]).astype(np.float32)
    with np.errstate(all="ignore"):
        want = (ab[:, 0].astype(np.float64) / ab[:, 1].astype(np.float64)).astype(np.float32)
    got = probe(backend, A.MATH_DIV, ab)[:, 0]
    ok = same(got, want)
    assert ok.all(), "a / b: %d differ, first %s" % ((~ok).sum(), ab[~ok][0])
    sub = (want != 0) & (np.abs(want) < F32_MIN_NORMAL)
    assert sub.sum() > 500 and (np.abs(ab[:, 1]) >= 2.0 ** 48).sum() > 1000 and ((np.abs(ab[:, 1]) < 2.0 ** -47) & (ab[:, 1] != 0)).sum() > 1000

    k = rng.integers(1, 1 << 12, 2000).astype(np.float64)
    sq = (k * k * 4.0 ** rng.integers(-40, 40, 2000)).astype(np.float32)  # exact squares: their neighbours' roots sit next to a representable value
    x = np.concatenate([np.abs(rnd[:, 0]), rnd[:2000, 1], np.abs(small[:, 0]), sq, from_bits(bits(sq) + 1), from_bits(bits(sq) - 1), EDGE_VALUES]).astype(np.float32)
    with np.errstate(all="ignore"):
        want = np.sqrt(x.astype(np.float64)).astype(np.float32)
    got = probe(backend, A.MATH_SQRT, x)[:, 0]
    ok = same(got, want)
    assert ok.all(), "sqrt_: %d differ, first %s" % ((~ok).sum(), x[~ok][0])
    assert bits(got[x == 0]).tolist() == bits(x[x == 0]).tolist()  # sqrt(-0) = -0


@pytest.mark.parametrize("backend", BACKENDS)
def test_min_max_rounding_and_clamp_helpers(backend):
    """max_ / min_ are Rust's f32::max / min (a NaN operand is ignored); max_nz / min_nz equal them wherever the operands do not tie as
    +0 against -0 (on the device they are the hardware's instructions); floor_, ceil_, max0_, clamp_ against numpy."""
    rng = np.random.default_rng(12)
    rnd = from_bits(rng.integers(0, 1 << 32, (20000, 2)))
    near = rnd[:4000].copy()
    near[:, 1] = from_bits(bits(near[:, 0]) + rng.integers(-1, 2, 4000))  # equal and neighbouring operands
    one_nan = rnd[:2000].copy()
    one_nan[::2, 0] = NAN
    one_nan[1::2, 1] = from_bits([0xFFC00001])[0]
    edges = np.array([(a, b) for a in EDGE_VALUES for b in EDGE_VALUES], np.float32)
    ab = np.concatenate([rnd, near, one_nan, edges]).astype(np.float32)
    tie = (ab[:, 0] == 0) & (ab[:, 1] == 0) & (np.signbit(ab[:, 0]) != np.signbit(ab[:, 1]))
    assert tie.sum() == 2
    mm = probe(backend, A.MATH_MINMAX, ab)
    with np.errstate(all="ignore"):
        assert same(mm[~tie, 0], np.fmax(ab[~tie, 0], ab[~tie, 1])).all() and same(mm[~tie, 1], np.fmin(ab[~tie, 0], ab[~tie, 1])).all()
    assert np.array_equal(bits(mm[tie, :2]), bits(np.stack([ab[tie, 1], ab[tie, 1]], axis=1)))  # the comparison form returns its second argument
    nz = probe(backend, A.MATH_MINMAX_NZ, ab[~tie])  # the documented domain: no +0 / -0 tie, one NaN operand allowed
    both_nan = np.isnan(ab[~tie]).all(axis=1)
    assert np.array_equal(bits(nz[~both_nan]), bits(mm[~tie][~both_nan])) and np.isnan(nz[both_nan, :2]).all()

    x = cat(rnd[:, 0], rng.uniform(-5, 5, 4000), np.arange(-4, 5) * 0.5, [8388607.5, -8388607.5, 8388608.0, 16777216.0, 2147483648.0, -0.75, 0.25], EDGE_VALUES)
    lo = np.concatenate([rng.uniform(-2, 1, len(x) - 6), [0.0, -0.0, 0.0, NAN, 0.0, 1.0]]).astype(np.float32)
    hi = np.concatenate([lo[:-6] + rng.uniform(0, 3, len(x) - 6).astype(np.float32), [ONE_MINUS_EPS, 0.0, NAN, 1.0, 0.0, 0.0]]).astype(np.float32)
    r = probe(backend, A.MATH_ROUND, np.stack([x, lo, hi], axis=1))
    with np.errstate(all="ignore"):
        assert same(r[:, 0], np.floor(x)).all() and same(r[:, 1], np.ceil(x)).all()
        assert same(r[:, 2], np.where(x >= 0, x, np.float32(0.0))).all()
        c = np.where(x < lo, lo, x)
        assert same(r[:, 3], np.where(c > hi, hi, c)).all()


def _u32_to_f32(v):
    """uint32 -> binary32, round to nearest even, in Python integers; returns the float"""
    if v < (1 << 24):
        return float(v)
    sh = v.bit_length() - 24
    q, rem = v >> sh, v & ((1 << sh) - 1)
    half = 1 << (sh - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    return float(q << sh)


@pytest.mark.parametrize("backend", BACKENDS)
def test_uint_to_unit_float_as_sobol_sample_ends(backend):
    """(float)v * 2^-32 rounds v to nearest even at 24 bits, then min_nz(1 - eps, .) clamps what rounded up to 1."""
    rng = np.random.default_rng(13)
    v = np.concatenate([[0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFF81, 0xFFFFFFFF, 0xFFFFFE80, 0xFFFFFE7F, 0xFFFFFE81, 0, 1, 0x00FFFFFF, 0x01000000, 0x01000001, 0x01000002, 0x01000003,
                         0x80000000, 0x80000040, 0x80000080, 0x800000C0, 0x80000140, 0x7FFFFFFF], rng.integers(0, 1 << 32, 20000), rng.integers(0xFFFFF000, 1 << 32, 2000)]).astype(np.int64)
    want = np.array([_u32_to_f32(int(x)) * 2.0 ** -32 for x in v], np.float64)
    assert (want.astype(np.float32) == want).all()
    out = probe(backend, A.MATH_U2F, from_bits(v))
    assert np.array_equal(bits(out[:, 0]), bits(want.astype(np.float32)))
    assert np.array_equal(bits(out[:, 1]), bits(np.minimum(want.astype(np.float32), ONE_MINUS_EPS)))
    assert out[:4, 0].tolist() == [float(ONE_MINUS_EPS), 1.0, 1.0, 1.0] and (out[:4, 1] == ONE_MINUS_EPS).all() and out[:, 1].max() == ONE_MINUS_EPS


def _i32(a):
    return np.asarray(a, np.int64) & 0xFFFFFFFF


def _signed(u):
    u = np.asarray(u, np.int64)
    return np.where(u >= 1 << 31, u - (1 << 32), u)


@pytest.mark.parametrize("backend", BACKENDS)
def test_integer_helpers(backend):
    """f2i_sat is Rust's `as i32` (NaN 0, saturating, truncating); inc_wrap wraps at i32::MAX; abs_mod lands in [0, b) for negative a,
    for powers of two (the mask form) and other moduli (the division form)."""
    rng = np.random.default_rng(14)
    p31 = np.float32(2147483648.0)
    x = cat([p31, -p31, np.nextafter(p31, INF), np.nextafter(p31, np.float32(0)), np.nextafter(-p31, -INF), np.nextafter(-p31, np.float32(0)), NAN, INF, -INF,
             0.0, -0.0, 0.99999994, -0.99999994, 1.5, -1.5, 2.5, -2.5, 16777216.0, -16777217.0, F32_MAX, -F32_MAX, F32_TINY],
            rng.uniform(-3e9, 3e9, 4000), rng.uniform(-100, 100, 4000), from_bits(rng.integers(0, 1 << 32, 4000)))
    n = len(x)
    i = np.concatenate([[2147483647, -1, 0, -2147483648, 2147483646], rng.integers(-(1 << 31), 1 << 31, n - 5)])
    a = np.concatenate([[-1, -1, -7, -8, -2147483648, -2147483648, -2147483648, -2147483647, 2147483647, -5, 0, -3], rng.integers(-(1 << 31), 1 << 31, n - 12)])
    b = np.concatenate([[1, 2, 4, 8, 3, 1 << 30, 2147483647, 1 << 30, 2147483647, 5, 7, 3], np.where(rng.integers(0, 2, n - 12) == 0, 1 << rng.integers(0, 31, n - 12), rng.integers(1, 1 << 31, n - 12))])
    out = bits(probe(backend, A.MATH_INT, np.stack([x, from_bits(_i32(i)), from_bits(_i32(a)), from_bits(_i32(b))], axis=1)))
    with np.errstate(all="ignore"):
        want = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x.astype(np.float64)), -2147483648.0, 2147483647.0)).astype(np.int64)
    assert np.array_equal(_signed(out[:, 0]), want)
    assert _signed(out[:9, 0]).tolist() == [2147483647, -2147483648, 2147483647, 2147483520, -2147483648, -2147483520, 0, 2147483647, -2147483648]
    assert np.array_equal(out[:, 1].astype(np.int64), _i32(i + 1)) and _signed(out[0, 1]) == -2147483648
    assert np.array_equal(out[:, 2].astype(np.int64), np.array([int(p) % int(q) for p, q in zip(a, b)], np.int64))
    refused = bits(probe(backend, A.MATH_INT, np.stack([x[:3], from_bits(_i32(i[:3])), from_bits(_i32([5, 5, -5])), from_bits(_i32([0, -3, -2147483648]))], axis=1)))
    assert not refused[:, 2].any()  # the probe answers 0 for a modulus that is not positive instead of dividing by it


def _next_up(u):
    if u == 0x7F800000:
        return u
    if u == 0x80000000:
        u = 0
    return (u + 1 if not (u >> 31) and not (u & 0x7FFFFFFF) > 0x7F800000 else u - 1) & 0xFFFFFFFF


def _next_down_q32(u):
    """math.rs:98-103 as written (Q32): positive values move UP, +-0 becomes a NaN pattern, negative values move towards zero; on bit patterns"""
    if u == 0xFF800000:
        return u
    if (u & 0x7FFFFFFF) == 0:
        u = 0x80000000
    positive = not (u >> 31) and (u & 0x7FFFFFFF) <= 0x7F800000
    return (u + 1 if positive else u - 1) & 0xFFFFFFFF


@pytest.mark.parametrize("backend", BACKENDS)
def test_next_float_gamma_power_heuristic_solve(backend):
    """next_float_up / next_float_down (with the reference's quirk Q32, the cases of test_next_float_quirk among them) on bit
    patterns in Python integers; gamma_err, power_heuristic and solve_2x2 against numpy binary32 arithmetic, operation by operation
    (a contracted a*b - c*d or a reciprocal in place of the division would differ)."""
    rng = np.random.default_rng(15)
    f = np.float32
    v = cat([1.0, -1.0, 0.0, -0.0, F32_TINY, -F32_TINY, F32_MAX, -F32_MAX, INF, -INF, F32_MIN_NORMAL, -F32_MIN_NORMAL, 0.99999994, 2.0],
            from_bits(rng.integers(0, 1 << 32, 6000)))
    v = v[~np.isnan(v)]
    n = len(v)
    gi = np.concatenate([[0, 1, 2, 3, 5, 7, 1 << 22, 1 << 23, 16777215], rng.integers(0, 1000, n - 9)])
    pq = np.abs(from_bits(rng.integers(0x20000000, 0x5F000000, (n, 2))))  # pdfs in [1e-19, 1e19]: the squares stay finite and normal
    pq[:8] = [(1, 1), (0, 1), (1, 0), (0, 0), (INF, 1), (1e-30, 1e-30), (1e30, 1), (F32_TINY, 3)]
    out = probe(backend, A.MATH_NEXT, np.stack([v, from_bits(gi), pq[:, 0], pq[:, 1]], axis=1))
    assert np.array_equal(bits(out[:, 0]), np.array([_next_up(u) for u in bits(v).tolist()], np.uint32))
    assert np.array_equal(bits(out[:, 1]), np.array([_next_down_q32(u) for u in bits(v).tolist()], np.uint32))
    up1 = bits(np.nextafter(f(1), f(2)))
    assert bits(out[0, 0]) == up1 and bits(out[0, 1]) == up1 and bits(out[1, 1]) == bits(np.nextafter(f(-1), f(0))) and np.isnan(out[2, 1]) and np.isnan(out[3, 1])
    with np.errstate(all="ignore"):
        ne = gi.astype(np.float32) * (f(1.1920929e-07) * f(0.5))
        assert same(out[:, 2], ne / (f(1) - ne)).all()
        ff, gg = pq[:, 0] * pq[:, 0], pq[:, 1] * pq[:, 1]
        assert same(out[:, 3], ff / (ff + gg)).all()

    m = np.concatenate([rng.uniform(-4, 4, (6000, 6)), rng.uniform(-4, 4, (2000, 6)) * 10.0 ** rng.integers(-8, 8, (2000, 6))]).astype(np.float32)
    m[:6] = [(0, 1, 1, 0, 2, 4), (0, 0, 0, 0, 2, 4), (1, 1, -1, 1, 2, 2), (1e-4, 0, 0, 1e-4, 1, 1), (1e-6, 0, 0, 1e-6, 1, 1), (1, 2, 3, 4, INF, INF)]
    m[6:200, 3] = m[6:200, 1] * m[6:200, 2] / m[6:200, 0]  # nearly singular: the determinant is what is left of a cancellation
    out = probe(backend, A.MATH_SOLVE, m)
    with np.errstate(all="ignore"):
        det = m[:, 0] * m[:, 3] - m[:, 1] * m[:, 2]
        r0 = (m[:, 3] * m[:, 4] - m[:, 1] * m[:, 5]) / det
        r1 = (m[:, 0] * m[:, 5] - m[:, 2] * m[:, 4]) / det
        ok = ~(np.abs(det) < f(1e-10)) & ~np.isnan(r0) & ~np.isnan(r1)
    assert np.array_equal(out[:, 0] == 1.0, ok) and ok[[0, 2, 3]].all() and not ok[[1, 4, 5]].any() and 0.8 < ok.mean() < 1
    assert np.array_equal(bits(out[:, 1]), bits(np.where(ok, r0, f(0)))) and np.array_equal(bits(out[:, 2]), bits(np.where(ok, r1, f(0))))
    assert (out[0, 1], out[0, 2]) == (4.0, 2.0) and (out[2, 1], out[2, 2]) == (0.0, 2.0)  # math.rs:276-299


# ---- composites ------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("backend", BACKENDS)
def test_frames_and_spherical_angles(backend):
    """normalize and coordinate_system against numpy binary32 arithmetic in the same order; spherical_theta / spherical_phi are
    pt_acosf / pt_atan2f (pinned to the fixture above) of the clamped z and of (y, x), with 2 pi added below zero."""
    rng = np.random.default_rng(16)
    f = np.float32
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.6, 0.52915026), (0.6, -0.6, 0.52915026), (1e-20, 0, 1), (0, -1e-20, -1),
                     (-0.0, -0.0, 1), (0.0, -0.0, -1), (-1e-3, -0.0, 1), (-1e-3, 0.0, 1), (1, -1e-10, 0)], np.float32)
    v = np.concatenate([axes, _unit(rng, 8000), _unit(rng, 2000) * (10.0 ** rng.uniform(-15, 15, (2000, 1))).astype(np.float32)]).astype(np.float32)
    out = probe(backend, A.MATH_FRAME, v)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        ln = np.sqrt((x * x + y * y + z * z).astype(np.float64)).astype(np.float32)  # (sqrt_ itself is pinned above)
        assert same(out[:, 0:3], v / ln[:, None]).all()
        first = np.abs(x) > np.abs(y)
        la = np.sqrt((x * x + z * z).astype(np.float64)).astype(np.float32)
        lb = np.sqrt((y * y + z * z).astype(np.float64)).astype(np.float32)
        zero = np.zeros_like(x)
        v2 = np.where(first[:, None], np.stack([-z, zero, x], axis=1) / la[:, None], np.stack([zero, z, -y], axis=1) / lb[:, None])
        v3 = np.stack([y * v2[:, 2] - z * v2[:, 1], z * v2[:, 0] - x * v2[:, 2], x * v2[:, 1] - y * v2[:, 0]], axis=1)
    assert same(out[:, 3:6], v2).all() and same(out[:, 6:9], v3).all()
    theta = probe("twin", A.MATH_ACOS, np.clip(z, f(-1), f(1)))[:, 0]
    phi = probe("twin", A.MATH_ATAN2, np.stack([y, x], axis=1))[:, 0]
    assert same(out[:, 9], theta).all() and same(out[:, 10], np.where(phi < 0, phi + f(2) * f(3.14159265358979323846), phi)).all()
    assert (out[:, 10] >= 0).all() and (out[:, 10] <= f(6.2831855)).all() and out[14, 10] == f(6.2831855)  # (-1e-10 + 2 pi rounds to 2 pi)


@pytest.mark.parametrize("backend", BACKENDS)
def test_spawn_pair_is_offset_ray_origin(backend):
    """spawn_from(spawn_pair(p, p_error, n), w) == offset_ray_origin(p, p_error, n, w) on bits, whichever side w is on; the side not
    taken is the other member of the pair; a zero offset leaves the point where it is, and no offset carries it far."""
    rng = np.random.default_rng(17)
    k = 8000
    p = (rng.uniform(-1, 1, (k, 3)) * 10.0 ** rng.integers(-3, 4, (k, 1))).astype(np.float32)
    p[:200, 0] = 0.0                      # a coordinate at zero
    p[200:400] = 0.0                      # the origin: no error bound either
    pe = (np.abs(p) * rng.uniform(0, 8, (k, 3)) * 2.0 ** -23).astype(np.float32)
    nrm, w = _unit(rng, k), _unit(rng, k)
    pe[400:600] = 0.0                     # no error bound: no offset
    nrm[600:800, 1] = 0.0                 # an offset component of exactly zero
    w[800:1000] = np.cross(nrm[800:1000], _unit(rng, 200)).astype(np.float32)  # grazing: dot(w, n) next to zero
    w[1000:1100] = nrm[1000:1100]
    w[1100:1200] = -nrm[1100:1200]
    out = probe(backend, A.MATH_SPAWN, np.concatenate([p, pe, nrm, w], axis=1))
    o, plus, minus, sf = out[:, 0:3], out[:, 3:6], out[:, 6:9], out[:, 9:12]
    assert np.array_equal(bits(o), bits(sf))
    below = (w[:, 0] * nrm[:, 0] + w[:, 1] * nrm[:, 1] + w[:, 2] * nrm[:, 2]) < 0  # dot() in binary32, the same order
    assert 0.3 < below.mean() < 0.7
    assert np.array_equal(bits(o), bits(np.where(below[:, None], minus, plus)))
    assert np.array_equal(bits(plus[400:600]), bits(p[400:600])) and np.array_equal(bits(minus[400:600]), bits(p[400:600]))
    far = np.abs(p).max(axis=1, keepdims=True) * 1e-4 + 1e-30  # (the error bounds are at most 8 ulp of the coordinate: |offset| < 3 * 8 * 2^-23 |p|)
    assert (np.abs(plus - p) <= far).all() and (np.abs(minus - p) <= far).all()


# ---- searches --------------------------------------------------------------------------------------------------------------------
CDFS = [
    [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0],                                      # 8 equal cells: every value on a guide boundary
    [0.0, 0.0, 0.0, 0.0, 0.3, 0.3, 0.30000001, 0.7, 1.0, 1.0, 1.0, 1.0],                          # a leading run of zeros, equal neighbours, a trailing run of ones
    [0.0, 1e-30, 2e-30, 0.1, 0.10000001, 0.10000002, 0.5, 0.5, 0.5, 0.99999994, 0.99999994, 1.0, 1.0, 1.0],  # 14 entries: the 16-cell guide; crowded cells
    [0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],                                           # one cell holds everything
    [0.0, 0.06, 0.12, 0.13, 0.2, 0.4, 0.41, 0.9, 0.95, 0.96, 0.97, 0.98, 1.0],
    [0.0, 1.0],                                                                                   # the smallest table
]


@pytest.mark.parametrize("backend", BACKENDS)
def test_cdf_searches_agree_with_a_bisection(backend):
    """find_interval_cdf_guided == find_interval_cdf == Python's bisect of cdf[i] <= u, clamped as math.rs:186-202 clamps (Q27), for u
    at every cdf value and its two neighbours, every guide boundary and its neighbours, 0, 1 - eps, negative and NaN."""
    rows, want = [], []
    for cdf in CDFS:
        c = np.array(cdf, np.float32)
        assert (np.diff(c) >= 0).all() and 2 <= len(c) <= 14
        grid = np.arange(17, dtype=np.float32) / np.float32(16)
        us = np.concatenate([c, grid, np.linspace(0, 1, 97, dtype=np.float32)])
        us = np.concatenate([us, np.nextafter(us, INF), np.nextafter(us, -INF), [0.0, -0.0, ONE_MINUS_EPS, -1.0, -F32_TINY, -INF, NAN, F32_TINY]]).astype(np.float32)
        us = us[~(us > ONE_MINUS_EPS)]  # samples live in [0, 1): the guide table's domain (negative and NaN take the plain search)
        for u in us:
            first = 0 if np.isnan(u) else bisect.bisect_right(c.tolist(), float(u))
            want.append(len(c) - 2 if first == 0 else min(first - 1, len(c) - 2))
            rows.append(np.concatenate([[u], from_bits([len(c)]), c, np.zeros(14 - len(c), np.float32)]))
    out = bits(probe(backend, A.MATH_SEARCH, np.array(rows, np.float32)))
    want = np.array(want, np.uint32)
    assert np.array_equal(out[:, 0], want), "plain search"
    assert np.array_equal(out[:, 1], want), "guided search"
    assert len(want) > 2000 and len(np.unique(want)) >= 10


# ---- Sobol' values from the table itself -----------------------------------------------------------------------------------------
def _matrices():
    raw = open(os.path.join(ROOT, "data", "sobol_tables.bin"), "rb").read()
    assert raw[:8] == b"PTRSSOB1"
    return np.frombuffer(raw, dtype="<u4", count=1024 * 52, offset=32).reshape(1024, 52).astype(np.int64)


def _sobol_backend(name):
    if name == "oracle":
        from oracle import orc
        return orc.sobol_samples
    return twin.sobol_samples if name == "twin" else ptrs.sobol_samples


SOBOL_CASES = [(5, 3, 1), (256, 256, 16), (3840, 2160, 512)]


@pytest.mark.parametrize("case", SOBOL_CASES, ids=lambda c: "%dx%dx%d" % c)
@pytest.mark.parametrize("backend", ["oracle", "twin", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_sobol_values_from_the_matrices(backend, case):
    """sobol_sample from Python integers over data/sobol_tables.bin: the XOR of the matrix columns at the set bits of the returned
    index, XOR the low 32 bits of the pixel's Cantor pairing, rounded uint32 -> binary32 to nearest even, times 2^-32, clamped to
    1 - eps.  Dimensions 2 .. 1023: the byte table, its upper half (33-bit indices at 4096^2 x 512) and, from 256 on, the bit-serial
    loop.  The index itself: its unscrambled dimensions 0 and 1 land in the pixel's cell of the 2^m grid, the bits above 2m are the
    sample number, and within an 8 x 8 block of pixels all spp samples have pairwise distinct indices."""
    from oracle import orc
    w, h, spp = case
    mats = _matrices()
    sample = _sobol_backend(backend)
    p = orc.make_params(w, h, spp, 4)
    m = orc.round_up_pow2(max(w + 4, h + 4)).bit_length() - 1
    rng = np.random.default_rng(18)
    n = 2000
    px, py, sn = rng.integers(-2, w + 2, n), rng.integers(-2, h + 2, n), rng.integers(0, spp, n)
    dims = rng.integers(2, 1024, n)
    dims[:10] = [4, 255, 256, 257, 1023, 2, 3, 5, 511, 512]
    sn[:5] = spp - 1
    px[:5], py[:5] = w + 1, h + 1  # the largest index there is
    got, idx = sample(p, px, py, sn, dims)
    want = np.zeros(n, np.float32)
    for k in range(n):
        i, v = int(idx[k]), 0
        a, b = int(px[k]) + 1073741823, int(py[k]) + 1073741823
        v ^= ((a + b) * (a + b + 1) // 2 + b) & 0xFFFFFFFF
        v0 = v1 = 0
        for c in range(i.bit_length()):
            if (i >> c) & 1:
                v ^= int(mats[dims[k], c])
                v0 ^= int(mats[0, c])
                v1 ^= int(mats[1, c])
        want[k] = min(np.float32(_u32_to_f32(v) * 2.0 ** -32), ONE_MINUS_EPS)
        assert i >> (2 * m) == sn[k]
        if m:
            assert (v0 >> (32 - m), v1 >> (32 - m)) == (px[k] + 2, py[k] + 2)
    assert np.array_equal(bits(got), bits(want))
    if case == SOBOL_CASES[-1]:
        assert int(idx.max()).bit_length() == 33 and (dims >= 256).sum() > 1000 and (dims < 256).sum() > 300
    # one 8 x 8 block, every sample: distinct indices
    bx, by = min(w - 1, 24), min(h - 1, 8)
    X, Y, S = np.meshgrid(np.arange(bx, bx + 8) - 4, np.arange(by, by + 8) - 4, np.arange(spp), indexing="ij")
    ok = (X >= -2) & (X < w + 2) & (Y >= -2) & (Y < h + 2)
    _, idx = sample(p, X[ok], Y[ok], S[ok], np.full(ok.sum(), 2, np.uint32))
    assert len(np.unique(idx)) == ok.sum() >= 8 * 5 * spp
