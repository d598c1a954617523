"""The short rotation of the row-Newton sweep (csrc/newton_rot.hip.h, used by csrc/wg_sweep_rows.hip.h: newton_rot_step):
for the range R = 2^LOG2_R and the Taylor coefficients the kernel is compiled with — read from the header itself, so
that this cannot check another polynomial — the truncation of

    sin d     ~ d + d^3 (S[0] + z (S[1] + ...))
    cos d - 1 ~ z (C[0] + z (C[1] + ...)),          z = d^2,

stays below 2e-17 (absolute: the trig pairs they turn are of magnitude <= 1) on |d| <= R, in exact rational arithmetic.
sin d and cos d - 1 themselves are taken as Taylor sums carried far enough that their own remainder is below 1e-40 on
the range (alternating series: the remainder is below the first omitted term)."""
import os
import re
from fractions import Fraction
from math import factorial

BOUND = Fraction(2, 10**17)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cgmres_cpp_amd", "csrc", "newton_rot.hip.h")


def _read():
    text = open(HEADER).read()
    log2_r = int(re.search(r"^#define CGM_NEWTON_ROT_LOG2_R \((-?\d+)\)$", text, re.M).group(1))

    def coeffs(name):
        body = re.search(r"^#define %s \{(.*)\}$" % name, text, re.M).group(1)
        out = []
        for term in body.split(","):
            m = re.fullmatch(r"\s*(-?\d+)\.0 / (\d+)\.0\s*", term)
            assert m, (name, term)
            out.append(Fraction(int(m.group(1)), int(m.group(2))))
        return out

    return log2_r, coeffs("CGM_NEWTON_ROT_SIN"), coeffs("CGM_NEWTON_ROT_COS")


def _sin(d, terms=12):
    return sum(Fraction((-1) ** n, factorial(2 * n + 1)) * d ** (2 * n + 1) for n in range(terms))


def _cosm1(d, terms=12):
    return sum(Fraction((-1) ** n, factorial(2 * n)) * d ** (2 * n) for n in range(1, terms))


def _horner(cs, z):
    acc = Fraction(0)
    for c in reversed(cs):
        acc = acc * z + c
    return acc


def test_header_holds_taylor_coefficients():
    log2_r, S, C = _read()
    assert log2_r < 0 and len(S) >= 1 and len(C) >= 1
    assert S == [Fraction((-1) ** n, factorial(2 * n + 1)) for n in range(1, len(S) + 1)]
    assert C == [Fraction((-1) ** n, factorial(2 * n)) for n in range(1, len(C) + 1)]


def test_truncation_below_2e17_on_the_whole_range():
    log2_r, S, C = _read()
    R = Fraction(1, 2 ** -log2_r)
    assert R ** 25 / factorial(25) < Fraction(1, 10**40)  # the reference sums' own remainder
    worst_s = worst_c = Fraction(0)
    grid = [R * Fraction(i, 64) for i in range(-64, 65)] + [R * Fraction(1, 2 ** j) for j in range(7, 40)]
    for d in grid:
        z = d * d
        es = abs(d + d * z * _horner(S, z) - _sin(d))
        ec = abs(z * _horner(C, z) - _cosm1(d))
        worst_s, worst_c = max(worst_s, es), max(worst_c, ec)
        assert es < BOUND and ec < BOUND, (float(d), float(es), float(ec))
    print(f"R = 2^{log2_r}: truncation of sin {float(worst_s):.3e}, of cos - 1 {float(worst_c):.3e}")
    # the errors grow with |d|: the ends of the range carry the maximum
    assert worst_s == abs(R + R**3 * _horner(S, R * R) - _sin(R))


def test_twice_the_range_misses_the_bound():
    """The header's choice is tight: twice the range misses 2e-17 with these terms (so R is the largest power of two they
    serve)."""
    log2_r, S, C = _read()
    d = Fraction(1, 2 ** (-log2_r - 1))
    z = d * d
    es = abs(d + d * z * _horner(S, z) - _sin(d))
    ec = abs(z * _horner(C, z) - _cosm1(d))
    assert es >= BOUND or ec >= BOUND, (float(es), float(ec))
