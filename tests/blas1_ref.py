"""A plain numpy / Python reference of the BLAS-1 vector layer: the named
broadcasts (xpby_, axpy_, axmy_, sub_, rmul_) and the reductions dot, norm
and psum.  It imports nothing from the package.

Elementwise.  The scalar decides the type an element is evaluated in, as
Julia's broadcast does:

* a scalar of the element type T, or an int: converted to T, arithmetic in T
  (over complex T the scalar is a complex T, the product the full formula);
* a Python float / np.float64: a Float64.  Elements are widened, a real
  scalar times a complex element is componentwise (a*re, a*im), the result
  is rounded to T once;
* a Python complex / np.complex128 over complex T: a ComplexF64, elements
  widened, the full product, one rounding.  Over real T a complex with a zero
  imaginary part is its real part as a Float64; any other is a TypeError.

Complex values are carried as separate real arrays and multiplied with
Julia's formula (re = ar*br - ai*bi, im = ar*bi + ai*br); numpy's complex
multiply is never used.

Reductions.  Two references: exact integers for inputs k * 2**-10 with
|k| <= 1024 (every term exact in Float32, every partial sum of up to 2**20
terms exact in Float64, so the summation order cannot show), and exact
rationals (fractions.Fraction over the stored values) for arbitrary inputs.
The exact family finishes as the library documents: each part's value is
rounded to T, the part values are added in T in part order, norm is the sqrt
of the real sum as a Float64."""
import math
from fractions import Fraction

import numpy as np

OPS = ("xpby", "axpy", "axmy", "sub", "rmul")


# ---------------------------------------------------------------------------
# elementwise

def scalar_kind(a, dtype):
    """'T', 'f64' or 'c128': the type a broadcast with scalar a over vectors
    of dtype is evaluated in (None, sub_'s missing scalar: 'T')"""
    cplx = np.dtype(dtype).kind == "c"
    if a is None or isinstance(a, (int, np.integer)):
        return "T"
    if isinstance(a, (float, np.float64)):
        return "f64"
    if isinstance(a, (complex, np.complex128)):
        if cplx:
            return "c128"
        if complex(a).imag != 0:
            raise TypeError("a complex scalar into a real vector (InexactError)")
        return "f64"
    if np.dtype(type(a)) == np.dtype(dtype):
        return "T"
    raise TypeError(f"scalar of type {type(a).__name__} next to {np.dtype(dtype)}")


def _split(v, P):
    """(re, im) of an array in precision P (im None: real)"""
    v = np.asarray(v)
    if v.dtype.kind == "c":
        return v.real.astype(P), v.imag.astype(P)
    return v.astype(P), None


def _scalar(a, kind, dtype):
    """(re, im) of the scalar in the evaluation precision; im None: a real
    scalar (componentwise over complex elements)"""
    T = np.dtype(dtype)
    R = np.zeros(1, T).real.dtype.type
    if kind == "T":
        if T.kind == "c":
            s = T.type(a)
            return R(s.real), R(s.imag)
        return R(a), None
    if kind == "f64":
        return np.float64(complex(a).real), None
    return np.float64(complex(a).real), np.float64(complex(a).imag)


def _mul(s, v):
    sr, si = s
    vr, vi = v
    if vi is None:
        return sr * vr, None
    if si is None:
        return sr * vr, sr * vi
    return sr * vr - si * vi, sr * vi + si * vr


def _add(u, v, sign=1):
    ur, ui = u
    vr, vi = v
    if sign > 0:
        return ur + vr, (None if ui is None else ui + vi)
    return ur - vr, (None if ui is None else ui - vi)


def bcast(op, y, x, a, kind=None):
    """the new values of y after op (one of OPS) with operand x (None for
    rmul) and scalar a (None for sub), as an array of y's dtype.  `kind`
    overrides the scalar's kind, to compute what another typing would give."""
    y = np.asarray(y)
    T = y.dtype
    kind = kind or scalar_kind(a, T)
    P = np.zeros(1, T).real.dtype if kind == "T" else np.dtype(np.float64)
    s = None if a is None else _scalar(a, kind, T)
    Y = _split(y, P)
    X = None if x is None else _split(np.asarray(x, dtype=T), P)
    with np.errstate(all="ignore"):
        if op == "xpby":      # u .= r .+ beta .* u
            r = _add(X, _mul(s, Y))
        elif op == "axpy":    # x .+= alpha .* u
            r = _add(Y, _mul(s, X))
        elif op == "axmy":    # r .-= alpha .* c
            r = _add(Y, _mul(s, X), -1)
        elif op == "sub":     # r .-= c
            r = _add(Y, X, -1)
        elif op == "rmul":    # rmul!(a, v)
            r = _mul(s, Y)
        else:
            raise ValueError(op)
        out = np.empty(y.shape, T)  # rounded to T once
        if T.kind == "c":
            out.real = r[0].astype(out.real.dtype)
            out.imag = r[1].astype(out.real.dtype)
        else:
            out[...] = r[0].astype(T)
    return out


def same_bits(got, want):
    """bit-exact, the sign of zero included, up to NaN signs and payloads"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "c":
        return same_bits(got.real.copy(), want.real.copy()) and same_bits(got.imag.copy(), want.imag.copy())
    num = ~np.isnan(want)
    return bool(np.array_equal(got, want, equal_nan=True)
                and np.array_equal(np.signbit(got[num]), np.signbit(want[num])))


# ---------------------------------------------------------------------------
# reductions: rounding helpers

def _real_type(dtype):
    return np.zeros(1, dtype).real.dtype.type


def round_to(fr, R):
    """the Fraction fr rounded to the real type R (np.float32 / np.float64),
    to nearest, ties to even"""
    fr = Fraction(fr)
    d = float(fr)  # Python rounds a Fraction to a double correctly
    if R is np.float64:
        return np.float64(d)
    with np.errstate(over="ignore"):
        f = np.float32(d)  # may be a double rounding: look at the neighbours
    if not np.isfinite(f):
        return f
    best = f
    for c in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        if not np.isfinite(c):
            continue
        dc, db = abs(Fraction(float(c)) - fr), abs(Fraction(float(best)) - fr)
        if dc < db or (dc == db and (int(c.view(np.uint32)) & 1) == 0):
            best = c
    return best


def fold_parts(vals, dtype, real_only=False):
    """reduce(+, part values; init = zero(T)) in T, in part order; vals:
    (re, im) Fractions per part"""
    R = _real_type(dtype)
    re, im = R(0), R(0)
    for vr, vi in vals:
        re = R(re + round_to(vr, R))
        if not real_only:
            im = R(im + round_to(vi, R))
    return re, im


def _result(re, im, dtype):
    return complex(float(re), float(im)) if np.dtype(dtype).kind == "c" else float(re)


# ---------------------------------------------------------------------------
# reductions, exact family: values k * 2**-10, Python integers

SCALE = 1 << 10


def exact_ints(a):
    """(re, im) lists of the Python integers k with a = k * 2**-10; asserts
    the family's precondition"""
    a = np.asarray(a)
    re = a.real.astype(np.float64) * SCALE
    im = a.imag.astype(np.float64) * SCALE if a.dtype.kind == "c" else np.zeros(len(a))
    for c in (re, im):
        assert np.all(c == np.rint(c)) and np.all(np.abs(c) <= SCALE), "not of the exact family"
    return [int(k) for k in re.tolist()], [int(k) for k in im.tolist()]


def _part_dot_int(a, b):
    ar, ai = exact_ints(a)
    br, bi = exact_ints(b)
    assert len(ar) == len(br) <= 1 << 20
    # conj(a) * b = (ar*br + ai*bi) + (ar*bi - ai*br) i
    re = sum(p * q for p, q in zip(ar, br)) + sum(p * q for p, q in zip(ai, bi))
    im = sum(p * q for p, q in zip(ar, bi)) - sum(p * q for p, q in zip(ai, br))
    return Fraction(re, SCALE * SCALE), Fraction(im, SCALE * SCALE)


def exact_dot_parts(parts_a, parts_b):
    """each part's exact dot as (re, im) Fractions; parts_*: the parts' owned
    values in part order.  The values do not depend on the element type (the
    family is exact in Float32), so one result serves every dtype."""
    return [_part_dot_int(a, b) for a, b in zip(parts_a, parts_b)]


def exact_sum_parts(parts_a):
    vals = []
    for a in parts_a:
        re, im = exact_ints(a)
        assert len(re) <= 1 << 20
        vals.append((Fraction(sum(re), SCALE), Fraction(sum(im), SCALE)))
    return vals


def finish(vals, dtype):
    """dot / psum from the parts' exact values, as the library documents"""
    re, im = fold_parts(vals, dtype)
    return _result(re, im, dtype)


def finish_norm(vals, dtype):
    """norm from the parts' exact sums of squares (exact_dot_parts(a, a))"""
    assert all(v[1] == 0 for v in vals)
    re, _ = fold_parts(vals, dtype, real_only=True)
    return math.sqrt(float(re))


def exact_dot(parts_a, parts_b, dtype):
    return finish(exact_dot_parts(parts_a, parts_b), dtype)


def exact_norm(parts_a, dtype):
    return finish_norm(exact_dot_parts(parts_a, parts_a), dtype)


def exact_sum(parts_a, dtype):
    return finish(exact_sum_parts(parts_a), dtype)


# ---------------------------------------------------------------------------
# reductions, random family: exact rationals

def _fractions(a):
    a = np.asarray(a)
    re = [Fraction(v) for v in a.real.astype(np.float64).tolist()]
    im = [Fraction(v) for v in a.imag.astype(np.float64).tolist()] if a.dtype.kind == "c" else None
    return re, im


def _fsum(terms):
    """the exact sum of Fractions, over their common denominator"""
    terms = list(terms)
    if not terms:
        return Fraction(0)
    D = math.lcm(*{t.denominator for t in terms})
    return Fraction(sum(t.numerator * (D // t.denominator) for t in terms), D)


def _abs_lower(re, im):
    """a Fraction not above |re + im i| (a double sqrt shrunk by 2**-50)"""
    if im is None or im == 0:
        return abs(re)
    return Fraction(math.sqrt(float(re * re + im * im)) * (1.0 - 2.0 ** -50))


def fraction_dot(a, b):
    """(re, im, S): the exact dot(a, b) = sum conj(a_i) b_i over the stored
    values and S, a lower bound of sum |t_i| over the exact terms t_i (exact
    for real vectors)"""
    (ar, ai), (br, bi) = _fractions(a), _fractions(b)
    if ai is None:
        t = [p * q for p, q in zip(ar, br)]
        return _fsum(t), Fraction(0), _fsum(abs(v) for v in t)
    tr = [p * q + r * s for p, q, r, s in zip(ar, br, ai, bi)]
    ti = [p * s - r * q for p, q, r, s in zip(ar, br, ai, bi)]
    return (_fsum(tr), _fsum(ti),
            _fsum(_abs_lower(u, v) for u, v in zip(tr, ti)))


def fraction_sum(a):
    """(re, im, S) of sum(a): the terms are the values themselves"""
    re, im = _fractions(a)
    if im is None:
        return _fsum(re), Fraction(0), _fsum(abs(v) for v in re)
    return (_fsum(re), _fsum(im),
            _fsum(_abs_lower(u, v) for u, v in zip(re, im)))


def eps_of(dtype):
    return Fraction(1, 1 << 24) if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)) \
        else Fraction(1, 1 << 53)


def sum_bound(n, nparts, dtype):
    """the relative bound (to sum |t_i|) that holds for every summation
    order: n * 2**-53 for the Float64 accumulation, 4 eps_T for each term's
    rounding in T (at most two products and an add), P eps_T for the per-part
    rounding to T and the adds across parts"""
    return Fraction(n, 1 << 53) + (4 + nparts) * eps_of(dtype)


def within(got, re, im, S, bound):
    """|got - (re + im i)| <= bound * S, in exact arithmetic"""
    g = complex(got)
    if not (math.isfinite(g.real) and math.isfinite(g.imag)):
        return False
    dr, di = Fraction(g.real) - re, Fraction(g.imag) - im
    lim = bound * S
    return dr * dr + di * di <= lim * lim


def norm_within(got, sumsq, bound):
    """|got - sqrt(sumsq)| <= (bound + 2**-52) * sqrt(sumsq), decided on the
    squares in exact arithmetic"""
    if not math.isfinite(got) or got < 0:
        return False
    r = bound + Fraction(1, 1 << 52)
    g2 = Fraction(got) ** 2
    return sumsq * (1 - r) ** 2 <= g2 <= sumsq * (1 + r) ** 2
