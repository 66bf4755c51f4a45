"""The BLAS-1 reference (blas1_ref.py) against hand-worked values: the GPU
tests of the vector layer compare with it, so its own typing and rounding
rules are pinned here on the host."""
import math
from fractions import Fraction

import numpy as np
import pytest

import blas1_ref as R


def test_wide_scalar_differs_from_float32_on_a_stated_element():
    """y + 0.1*x over Float32 with y = (0, 1), x = (9, 3).

    Element 0, all Float32: Float32(0.1) = 0x199999a * 2**-28; times 9 is
    0xe66666a * 2**-28, 28 bits, rounded to 24: 0xe66667 * 2**-24 =
    0x1.cccccep-1.  Wide: 0.1 * 9.0 = 0.9 in Float64, rounded once:
    0x1.ccccccp-1.  Element 1: both give 0x1.4cccccp+0."""
    y, x = np.array([0, 1], np.float32), np.array([9, 3], np.float32)
    wide = R.bcast("axpy", y, x, 0.1)
    narrow = R.bcast("axpy", y, x, np.float32(0.1))
    assert wide.dtype == narrow.dtype == np.float32
    assert float(wide[0]).hex() == "0x1.cccccc0000000p-1"
    assert float(narrow[0]).hex() == "0x1.ccccce0000000p-1"
    assert float(wide[1]).hex() == float(narrow[1]).hex() == "0x1.4ccccc0000000p+0"
    assert R.same_bits(R.bcast("axpy", y, x, 0.1, kind="T"), narrow)
    assert not R.same_bits(wide, narrow)


def test_the_five_operations():
    y, x = np.array([2.0, -3.0]), np.array([5.0, 7.0])
    assert np.array_equal(R.bcast("xpby", y, x, 2), [9.0, 1.0])      # x + 2y
    assert np.array_equal(R.bcast("axpy", y, x, 2), [12.0, 11.0])    # y + 2x
    assert np.array_equal(R.bcast("axmy", y, x, 2), [-8.0, -17.0])   # y - 2x
    assert np.array_equal(R.bcast("sub", y, x, None), [-3.0, -10.0])
    assert np.array_equal(R.bcast("rmul", y, None, 2), [4.0, -6.0])
    # complex: (1+2i)(3+4i) = -5 + 10i, Julia's formula
    z = R.bcast("rmul", np.array([3 + 4j], np.complex64), None, np.complex64(1 + 2j))
    assert z.dtype == np.complex64 and z[0] == -5 + 10j
    assert R.bcast("rmul", np.array([3 + 4j]), None, 1 + 2j)[0] == -5 + 10j


def test_scalar_kinds():
    assert R.scalar_kind(2, np.float32) == "T" and R.scalar_kind(np.float32(2), np.float32) == "T"
    assert R.scalar_kind(2.0, np.float32) == "f64" and R.scalar_kind(np.float64(2), np.complex64) == "f64"
    assert R.scalar_kind(1 + 2j, np.complex64) == "c128" and R.scalar_kind(np.complex64(1), np.complex64) == "T"
    assert R.scalar_kind(2 + 0j, np.float32) == "f64"
    with pytest.raises(TypeError):
        R.scalar_kind(2 + 1j, np.float64)
    with pytest.raises(TypeError):
        R.bcast("rmul", np.ones(2, np.float32), None, 1j)


def test_real_scalar_over_complex_is_componentwise():
    """2.0 * (inf + 1i) = inf + 2i; the complex product with 2 + 0i has
    im = 2*1 + 0*inf = NaN"""
    for T in (np.complex64, np.complex128):
        z = np.array([complex(np.inf, 1.0)], T)
        r = R.bcast("rmul", z, None, 2.0)
        assert r.dtype == T and r[0].real == np.inf and r[0].imag == 2.0
        c = R.bcast("rmul", z, None, 2.0, kind="c128")
        assert c[0].real == np.inf and math.isnan(c[0].imag)
        t = R.bcast("rmul", z, None, 2)  # an int is a complex T: the full product too
        assert math.isnan(t[0].imag)


def test_signed_zero_and_same_bits():
    assert R.same_bits(np.array([-0.0, np.nan]), np.array([-0.0, np.nan]))
    assert not R.same_bits(np.array([-0.0]), np.array([0.0]))
    assert not R.same_bits(np.array([1.0], np.float32), np.array([1.0]))
    # -0.0 - 0.0 = -0.0, 0.0 * -1 = -0.0
    assert np.signbit(R.bcast("sub", np.array([-0.0]), np.array([0.0]), None)[0])
    assert np.signbit(R.bcast("rmul", np.array([0.0]), None, -1)[0])


def test_conjugate_is_on_the_first_argument():
    """dot(i, 1) = conj(i) * 1 = -i; dot(1, i) = i"""
    for T in (np.complex64, np.complex128):
        a, b = np.array([1j], T), np.array([1 + 0j], T)
        assert R.exact_dot([a], [b], T) == -1j
        assert R.exact_dot([b], [a], T) == 1j
        re, im, S = R.fraction_dot(a, b)
        assert (re, im) == (0, -1) and abs(S - 1) < Fraction(1, 1 << 40) and S <= 1
    # (1+2i)/1024 and (3-1i)/1024: conj(a) b = (3 - 2) + (-1 - 6)i, over 2**20
    a, b = np.array([(1 + 2j) / 1024]), np.array([(3 - 1j) / 1024])
    assert R.exact_dot([a], [b], np.complex128) == complex(1, -7) / 2 ** 20
    assert R.fraction_dot(a, b)[:2] == (Fraction(1, 1 << 20), Fraction(-7, 1 << 20))


def test_float32_part_values_are_rounded_before_they_are_added():
    """part 1 sums to (2**24 + 1) * 2**-10, which Float32 rounds (tie, to
    even) to 16384; adding part 2's 2**-10 is a tie again: 16384.  The same
    values on one part sum to 16384 + 2**-9, a Float32."""
    one = np.float32(2.0 ** -10)
    p1 = np.concatenate([np.ones(16384, np.float32), [one]])
    p2 = np.array([one], np.float32)
    assert R.exact_sum([p1, p2], np.float32) == 16384.0
    assert R.exact_sum([np.concatenate([p1, p2])], np.float32) == 16384.0 + 2.0 ** -9
    assert R.exact_sum([p1.astype(np.float64), p2.astype(np.float64)], np.float64) == 16384.0 + 2.0 ** -9
    # norm: sqrt of the Float32 sum as a Float64; 3 parts of one value 1/2: sqrt(0.75)
    h = [np.array([0.5], np.float32)] * 3
    assert R.exact_norm(h, np.float32) == math.sqrt(0.75)
    assert R.exact_norm([np.array([(3 + 4j) / 1024], np.complex64)], np.complex64) == 5 / 1024
    assert R.exact_sum([np.array([], np.float32)], np.float32) == 0.0


def test_round_to_rounds_once():
    """1 + 2**-24 + 2**-60 is above the Float32 tie: 1 + 2**-23, although the
    nearest double is the tie itself"""
    fr = 1 + Fraction(1, 1 << 24) + Fraction(1, 1 << 60)
    assert float(fr) == 1 + 2.0 ** -24
    assert R.round_to(fr, np.float32) == np.float32(1 + 2.0 ** -23)
    assert R.round_to(1 + Fraction(1, 1 << 24), np.float32) == np.float32(1)            # tie: to even
    assert R.round_to(1 + Fraction(3, 1 << 24), np.float32) == np.float32(1 + 2.0 ** -22)  # tie: to even
    assert R.round_to(Fraction(1, 3), np.float64) == 1 / 3


def test_exact_family_precondition():
    with pytest.raises(AssertionError):
        R.exact_ints(np.array([0.1]))
    with pytest.raises(AssertionError):
        R.exact_ints(np.array([2.0]))
    assert R.exact_ints(np.array([1.0, -0.5 + 2j / 1024])) == ([1024, -512], [0, 2])


def test_bounds():
    assert R.sum_bound(70001, 4, np.float32) == Fraction(70001, 1 << 53) + Fraction(8, 1 << 24)
    assert R.sum_bound(3, 1, np.complex128) == Fraction(8, 1 << 53)
    re, im, S = R.fraction_sum(np.array([0.5, -0.25, 0.125]))
    assert (re, im, S) == (Fraction(3, 8), 0, Fraction(7, 8))
    b = Fraction(1, 1 << 20)
    assert R.within(0.375 + 0.875 * 2.0 ** -20, re, im, S, b)
    assert not R.within(0.375 + 0.875 * 2.0 ** -20 + 2.0 ** -40, re, im, S, b)
    assert not R.within(math.nan, re, im, S, b) and not R.within(math.inf, re, im, S, b)
    assert R.norm_within(3.0, Fraction(9), Fraction(0))
    assert R.norm_within(3.0 * (1 + 2.0 ** -21), Fraction(9), b)
    assert not R.norm_within(3.0 * (1 + 2.0 ** -19), Fraction(9), b)
    assert not R.norm_within(math.nan, Fraction(9), b)
