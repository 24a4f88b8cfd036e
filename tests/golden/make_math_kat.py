"""Writes tests/golden/math_kat.npz: known answers for the transcendental stand-ins of include/ptrs_detmath.h.

    python tests/golden/make_math_kat.py          (needs mpmath; deterministic: no random numbers, no libm)

For every function the expected result is the exact value (mpmath at 300 bits) rounded ONCE to the binary32 grid, ties to even, with
one ulp = 2^max(e - 23, -149) for a value in [2^e, 2^(e+1)): subnormal results are rounded on their own grid, not to 24 bits and then
cast.  Special arguments (zeros, infinities, NaN) follow C99 Annex F.

What the file holds, per function `f` of FUNCTIONS:
    f_edge_x   the edge arguments as binary32 bit patterns (n_edge x arity): written out because finding them needs mpmath
    f_sha      sha256 of the bit patterns of ALL arguments, grid first, then edges
    f_e        the expected bit patterns of all of them, stored as four byte planes (4 x n, most compressible that way)
The grid arguments -- N_GRID per function, the bulk -- are NOT stored: grid_args() below rebuilds them from integer arithmetic
and correctly rounded binary64 operations alone (+ - * / sqrt ldexp and the cast to binary32), so they are the same on every machine;
f_sha proves it.  The file may be no larger than the largest fixture already here (cornell_hits.npz, 127 756 bytes): the expected
bits alone cost about 2.8 bytes per argument after compression, which is what sets N_GRID; arguments stored literally would halve it.

tests/test_math_kat.py imports this module for grid_args(), extra_args() (arguments outside a function's domain of use, held to the
host build's bits only) and expected_bits(); mpmath is needed only to write the file and for the test that recomputes a subsample.
"""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "math_kat.npz")
N_GRID = 4800
# name -> arity.  sincos takes sin's arguments and must return sin's and cos's expected bits: it has no entries of its own.
FUNCTIONS = {"sin": 1, "cos": 1, "tan": 1, "log": 1, "log2": 1, "exp": 1, "pow": 2, "atan2": 2, "acos": 1}
# Near-ties the header admits (its error is < 2^-48 relative: a true value within 2^-45 relative of a rounding boundary, about 1 in
# 1e7 arguments, may round the other way).  At most one per function, by value, with its mpmath distance to the boundary in ulps of
# the result.  None was met on these sets.
NEAR_TIES = {}

F32_MAX = np.float32(3.4028234663852886e38)
F32_TINY = np.float32(1.401298464324817e-45)
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _weyl(n, salt):
    """n numbers in [0, 1) from integer arithmetic: a Weyl sequence, decorrelated between sets by `salt`."""
    i = np.arange(1, n + 1, dtype=np.uint64)
    return ((i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0


def _linear(lo, hi, n, salt):
    """one jittered point per stratum of [lo, hi], ascending"""
    return (lo + (hi - lo) * ((np.arange(n) + _weyl(n, salt)) / n)).astype(np.float32)


def _binades(k_lo, k_hi, n, salt):
    """(1 + w) * 2^k, k stepping evenly through k_lo .. k_hi - 1: log-spaced over [2^k_lo, 2^k_hi), ascending by binade"""
    k = k_lo + (np.arange(n) * (k_hi - k_lo)) // n
    return np.ldexp(1.0 + _weyl(n, salt), k).astype(np.float32)


def grid_args(name):
    """The bulk arguments of `name` on its domain of use: (N_GRID x arity) binary32."""
    n, h = N_GRID, N_GRID // 2
    if name in ("sin", "cos"):  # [0, 2 pi]
        x = _linear(0.0, 6.283185307179586, n, 1)
    elif name == "tan":  # [-1.5, 1.5]
        x = _linear(-1.5, 1.5, n, 2)
    elif name == "log":  # (0, 1]: linear, and log-spaced down to 2^-34 (6e-11)
        x = np.concatenate([_linear(0.0, 1.0, h, 3), _binades(-34, 0, h, 4)])
        x[x == 0] = np.float32(1.0)
    elif name == "log2":  # [2^-27, 2^14) covers [1e-8, 1e4]
        x = _binades(-27, 14, n, 5)
    elif name == "exp":  # [-104, 2]: every subnormal result, the flush to zero and ordinary values
        x = _linear(-104.0, 2.0, n, 6)
    elif name == "acos":  # [-1, 1]: linear, and 1 - t, -1 + t for t log-spaced down to 2^-27
        t = _binades(-27, -1, h // 2, 8).astype(np.float64)
        x = np.concatenate([_linear(-1.0, 1.0, h, 7), (1.0 - t).astype(np.float32), (-1.0 + t).astype(np.float32)])
    elif name == "atan2":  # (y, x): components of unit vectors, every quadrant
        a, b = 2.0 * _weyl(n, 9) - 1.0, 2.0 * ((np.arange(n) + _weyl(n, 10)) / n) - 1.0
        r = np.sqrt(a * a + b * b)
        r[r == 0] = 1.0
        return np.stack([(a / r).astype(np.float32), (b / r).astype(np.float32)], axis=1)
    elif name == "pow":  # x in (0, 1] (linear, and log-spaced from 2^-20 = 1e-6), y in [2^-7, 2^7) log-spaced
        x = np.concatenate([_linear(0.0, 1.0, h, 11), _binades(-20, 0, h, 12)])
        x[x == 0] = np.float32(0.5)
        y = _binades(-7, 7, n, 13)[(np.arange(n) * 2503) % n]  # (2503 is prime to n: every y once, decorrelated from x)
        return np.stack([x, y], axis=1)
    else:
        raise KeyError(name)
    return x.reshape(-1, 1)


def _around(x, k=2):
    """x as binary32 and its k neighbours on either side"""
    b = np.array([x], dtype=np.float32).view(np.uint32)[0].astype(np.int64)
    return f32([b + d for d in range(-k, k + 1)])


# Arguments outside a function's domain of use.  The header does not promise the correctly rounded result there (the two-term
# Cody-Waite reduction of sin / cos loses bits beyond |x| ~ 1.6e6: 1 ulp off for about 1 argument in 1e4; pow's error grows with
# |y log x|), so these rows are held to the host build's bits only: device and host must agree on them, not correct them.
def extra_args(name):
    if name in ("sin", "cos", "tan"):  # [2^13, 2^24) covers [1e4, 1e7]; the largest finite value
        return np.concatenate([_binades(13, 24, 2000, 21), -_binades(13, 24, 200, 22), [F32_MAX, -F32_MAX]]).astype(np.float32).reshape(-1, 1)
    if name == "exp":  # (2, 89]: ordinary values, and the overflow at 88.72...
        return np.concatenate([_linear(2.0, 89.0, 2000, 23), _around(88.72283935546875, 3), [np.float32(89.0), F32_MAX, -F32_MAX]]).astype(np.float32).reshape(-1, 1)
    if name == "pow":  # y in [2^7, 2^10)
        x = np.concatenate([_linear(0.0, 1.0, 1000, 24), _binades(-20, 0, 1000, 25)])
        x[x == 0] = np.float32(0.5)
        y = _binades(7, 10, 2000, 26)[(np.arange(2000) * 1999) % 2000]
        return np.stack([x, y], axis=1)
    return np.zeros((0, FUNCTIONS[name]), np.float32)


def round_once(v, mp):
    """The mpmath number v rounded once to the binary32 grid, ties to even -> bit pattern (uint32).  v: finite mpf, nonzero or zero."""
    if v == 0:
        return 0
    sign = 0x80000000 if v < 0 else 0
    a = abs(v)
    e = mp.frexp(a)[1] - 1           # a in [2^e, 2^(e+1))
    if e >= 128:
        return sign | 0x7F800000
    q = max(e - 23, -149)            # one ulp = 2^q
    s = mp.ldexp(a, -q)              # exact: a scaling by a power of two
    n = int(mp.floor(s))
    rem = s - n
    if rem > 0.5 or (rem == 0.5 and (n & 1)):
        n += 1
    val = np.ldexp(np.float64(n), q)  # n <= 2^24: exact in binary64
    if val >= 2.0 ** 128:
        return sign | 0x7F800000
    return sign | int(np.array([val], dtype=np.float64).astype(np.float32).view(np.uint32)[0])  # exact: the value is on the binary32 grid


_QNAN, _PINF, _NINF, _NZERO = 0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000


def expected_bits(name, args):
    """The expected bit pattern of `name` at one argument tuple (binary32 values).  NaN is reported as the quiet NaN 0x7fc00000."""
    import mpmath
    mp = mpmath.mp
    mp.prec = 300
    x = float(args[0])
    y = float(args[1]) if len(args) > 1 else 0.0
    neg = lambda t: np.signbit(np.float64(t))
    isinf, isnan = np.isinf, np.isnan
    X = mpmath.mpf(x) if np.isfinite(x) else None
    if name in ("sin", "cos", "tan"):
        if isnan(x) or isinf(x):
            return _QNAN
        if x == 0:
            return 0x3F800000 if name == "cos" else (_NZERO if neg(x) else 0)
        v = {"sin": mp.sin, "cos": mp.cos, "tan": mp.tan}[name](X)
    elif name in ("log", "log2"):
        if isnan(x):
            return _QNAN
        if x == 0:
            return _NINF
        if x < 0:
            return _QNAN
        if isinf(x):
            return _PINF
        v = mp.log(X) if name == "log" else mp.log(X) / mp.log(2)
    elif name == "exp":
        if isnan(x):
            return _QNAN
        if isinf(x):
            return 0 if x < 0 else _PINF
        v = mp.exp(X)
    elif name == "acos":
        if isnan(x) or abs(x) > 1:
            return _QNAN
        v = mp.acos(X)
    elif name == "pow":  # C99 F.9.4.4, whatever the header does there (see pow_restriction)
        y_int = bool(np.isfinite(y)) and y == np.floor(y)
        y_odd = y_int and abs(y) < 2.0 ** 24 and int(y) % 2 == 1  # (a binary32 integer from 2^24 on is even)
        if y == 0 or x == 1:
            return 0x3F800000
        if isnan(x) or isnan(y):
            return _QNAN
        if x == 0:
            sign = _NZERO if (neg(x) and y_odd) else 0
            return sign | (_PINF if y < 0 else 0)
        if isinf(y):
            if x == -1:
                return 0x3F800000
            return _PINF if (abs(x) < 1) == (y < 0) else 0
        if isinf(x):
            sign = _NZERO if (x < 0 and y_odd) else 0
            return sign | (0 if y < 0 else _PINF)
        if x < 0 and not y_int:
            return _QNAN
        v = mp.power(X, int(y)) if x < 0 else mp.power(X, mpmath.mpf(y))
    elif name == "atan2":  # atan2(y = args[0], x = args[1]), C99 F.9.1.4
        yy, xx = x, y
        if isnan(yy) or isnan(xx):
            return _QNAN
        sgn = -1 if neg(yy) else 1
        if yy == 0:
            if not neg(xx):
                return _NZERO if sgn < 0 else 0
            v = sgn * mp.pi
        elif xx == 0:
            v = sgn * mp.pi / 2
        elif isinf(xx):
            if isinf(yy):
                v = sgn * (3 * mp.pi / 4 if xx < 0 else mp.pi / 4)
            elif xx > 0:
                return _NZERO if sgn < 0 else 0
            else:
                v = sgn * mp.pi
        elif isinf(yy):
            v = sgn * mp.pi / 2
        else:
            v = mp.atan2(mpmath.mpf(yy), mpmath.mpf(xx))
    else:
        raise KeyError(name)
    return round_once(v, mp)


def pow_restriction(x, y):
    """What ptd_pow documents for the rows where it is not C99's pow (its comment in include/ptrs_detmath.h), written from that
    comment: the bit pattern it returns there, or None where it follows C99.  The renderer raises non-negative bases only."""
    if y == 0:
        return None
    if np.isnan(x) or np.isnan(y):
        return _QNAN if x == 1 else None                    # pow(1, NaN): NaN, C99 1
    if x == 0 and np.signbit(x):
        return _PINF if y < 0 else 0                        # -0 as +0: C99 keeps the zero's sign for odd integer y
    if x < 0:
        return _QNAN                                        # a negative base, -inf included: NaN whatever y is
    return None


def edge_args(name):
    """The edges of `name`: signed zeros, the smallest subnormal, the largest finite value where the function's domain reaches it,
    both neighbours of every breakpoint of the header, infinities and NaN."""
    import mpmath
    mp = mpmath.mp
    mp.prec = 300
    one = np.float32(1.0)
    common = [np.float32(0.0), np.float32(-0.0), F32_TINY, -F32_TINY, INF, -INF, NAN]
    if name in ("sin", "cos", "tan"):  # quadrant boundaries k pi/2 +- 2 ulp, k = -4 .. 8 (the largest finite value: see EXTRA)
        e = [_around(float(k * mp.pi / 2)) for k in range(-4, 9) if k != 0]
        e += [_around(float(mp.pi / 4)), _around(float(3 * mp.pi / 4)), f32([1, 2, 0x007FFFFF, 0x00800000, 0x80000001])]
        return np.concatenate([np.array(common, np.float32)] + e).reshape(-1, 1)
    if name in ("log", "log2"):  # m next to sqrt(2) in several binades, x next to 1, powers of two, subnormal arguments
        r2 = float(mp.sqrt(2))
        e = [_around(r2 * 2.0 ** k, 3) for k in (-30, -8, -2, -1, 0, 1, 6)] + [_around(1.0, 3), _around(0.5), _around(2.0), _around(2.0 ** -126, 3)]
        e += [f32([1, 2, 3, 0x007FFFFF, 0x00400000]), np.array([F32_MAX, np.float32(1e-38), np.float32(1e-45), np.float32(-1.0)], np.float32)]
        return np.concatenate([np.array(common, np.float32)] + e).reshape(-1, 1)
    if name == "exp":  # where the result crosses 2^-126 (the first subnormal), 2^-149 (the last) and 2^-150 (the flush to zero)
        e = [_around(float(k * mp.log(2)), 4) for k in (-126, -127, -140, -148, -149, -150, -151, -1, 1)]
        e += [_around(0.0, 0), _around(1.0), _around(-1.0), _around(-104.0), _around(2.0), _around(float(mp.log(2) / 2)), _around(float(-mp.log(2) / 2))]
        e += [f32([1, 0x80000001, 0x00800000, 0x33000000, 0xB3000000, 0x33800000, 0xB3800000])]  # tiny arguments: the result is 1 or its neighbour
        return np.concatenate([np.array(common[:4] + [-INF, INF, NAN], np.float32)] + e).reshape(-1, 1)
    if name == "acos":  # x next to +-1 (beyond them: NaN), to 0, to +-0.5 and to the atan breakpoints it reaches
        e = [_around(1.0, 4), _around(-1.0, 4), _around(0.5), _around(-0.5), _around(float(mp.sqrt(2) / 2)), _around(-float(mp.sqrt(2) / 2))]
        for z in (0.125, 0.375, 0.625, 0.875):  # sqrt(1 - x^2) / |x| = z  at  |x| = 1 / sqrt(1 + z^2), and the inverse quotient at z / sqrt(1 + z^2)
            c = float(1 / mp.sqrt(1 + mpmath.mpf(z) ** 2))
            e += [_around(c), _around(-c), _around(z * c), _around(-z * c)]
        e += [np.array([2.0, -2.0, F32_MAX, -F32_MAX, 1e-20, -1e-20], np.float32), f32([0x007FFFFF, 0x00800000])]
        return np.concatenate([np.array(common, np.float32)] + e).reshape(-1, 1)
    if name == "atan2":
        rows = []
        zs, big = [np.float32(0.0), np.float32(-0.0)], [one, -one, F32_TINY, -F32_TINY, F32_MAX, -F32_MAX, INF, -INF]
        for a in zs:  # all four sign combinations of zero, and every axis
            for b in zs:
                rows.append((a, b))
            for b in big:
                rows += [(a, b), (b, a)]
        for a in (INF, -INF):
            for b in (INF, -INF, one, -one):
                rows += [(a, b), (b, a)]
        rows += [(NAN, one), (one, NAN), (NAN, NAN), (NAN, np.float32(0.0)), (INF, NAN)]
        for z in (0.125, 0.375, 0.625, 0.875, 1.0):  # the quotient next to every breakpoint of ptd_atan_pos, both ways up, every quadrant
            for zz in _around(z, 3):
                for sy in (1, -1):
                    for sx in (1, -1):
                        rows += [(np.float32(sy) * zz, np.float32(sx)), (np.float32(sy), np.float32(sx) * zz), (np.float32(sy * 3.0) * zz, np.float32(sx * 3.0))]
        rows += [(F32_TINY, F32_MAX), (F32_MAX, F32_TINY), (F32_TINY, F32_TINY), (F32_MAX, F32_MAX), (-F32_MAX, F32_MAX), (np.float32(1e-30), np.float32(-1e30)),
                 (np.float32(1e-45), np.float32(-1.0)), (np.float32(-1e-45), np.float32(-1.0)), (np.float32(1e30), np.float32(1e-30))]
        return np.array(rows, np.float32)
    if name == "pow":  # positive bases: x = 1 exactly and next to it, y = 0, 1, 2, 0.5, tiny; results that go subnormal and to zero; then
        # every pair of zero, negative, infinite, NaN and ordinary operands (odd, even and non-integer exponents among them)
        xs = [0.0, -0.0, F32_TINY, -F32_TINY, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, -3.0, 1.5, -1.5, F32_MAX, -F32_MAX, INF, -INF, NAN]
        ys = [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 0.5, -0.5, 2.5, -2.5, F32_TINY, -F32_TINY, 16777215.0, -16777215.0, 16777216.0, F32_MAX, -F32_MAX,
              INF, -INF, NAN]
        special = [(a, b) for a in xs for b in ys]
        rows = [(one, 5.0), (one, 0.0), (0.5, 0.0), (0.5, 1.0), (0.5, 2.0), (0.25, 0.5), (0.5, 126.0), (0.5, 127.0), (0.5, 100.5), (1e-6, 6.0), (1e-6, 7.0), (1e-6, 7.5),
                (0.99999994, 100.0), (0.99999994, 1e-2), (1.0000001, 64.0), (1e-6, 1e-2), (0.1, 37.0), (0.1, 38.0), (0.1, 44.0), (0.1, 45.0), (0.1, 46.0), (F32_TINY, 1.0),
                (F32_TINY, 0.5), (2.0 ** -126, 1.0), (0.3, 1e-45), (F32_MAX, 1.0), (F32_MAX, 0.5), (2.0, 10.0), (10.0, 2.0), (3.0, 3.0)]
        return np.array(rows + special, np.float32)
    raise KeyError(name)


def all_args(name, edges):
    return np.concatenate([grid_args(name), np.asarray(edges, np.float32).reshape(-1, FUNCTIONS[name])]).astype(np.float32)


def digest(args):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(args, np.float32).view(np.uint32).tobytes()).digest(), np.uint8)


def planes(bits):
    return np.ascontiguousarray(np.asarray(bits, "<u4").view(np.uint8).reshape(-1, 4).T)


def unplanes(p):
    return np.ascontiguousarray(np.asarray(p, np.uint8).T).view("<u4").reshape(-1)


def main():
    out = {}
    for name in FUNCTIONS:
        edges = edge_args(name)
        args = all_args(name, edges)
        exp = np.array([expected_bits(name, a) for a in args], np.uint32)
        out[name + "_edge_x"] = edges.view(np.uint32)
        out[name + "_sha"] = digest(args)
        out[name + "_e"] = planes(exp)
        if name == "pow":  # the rows where the header documents another answer than C99's, by value, with that answer
            doc = [pow_restriction(a[0], a[1]) for a in args]
            differs = np.array([d is not None and d != e for d, e in zip(doc, exp)])
            out["pow_restricted_x"] = args[differs].view(np.uint32)
            out["pow_restricted_c99"] = exp[differs]
            out["pow_restricted_header"] = np.array([d for d, k in zip(doc, differs) if k], np.uint32)
            print("pow: %d rows where the header is documented not to be C99's pow" % differs.sum())
        print("%-6s %5d grid + %4d edge arguments" % (name, len(args) - len(edges), len(edges)))
    np.savez_compressed(PATH, **out)
    print("wrote %s: %d bytes" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
