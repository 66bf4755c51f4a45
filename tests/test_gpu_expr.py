"""Broadcast expressions and mapped reductions on the device (pa_vec_eval,
pa_reduce_expr_all) against numpy, node by node in the inferred type.

Elementwise results are bit-exact: IEEE + - * / without contraction leave no
room for a tolerance.  The reference below (`Ref`) restates Julia's broadcast
typing on its own: a node is evaluated in Float32 unless an operand is a
Float64 / ComplexF64 scalar or a wide node (`astype` at each boundary), and
complex arithmetic works on separate real and imaginary arrays with Julia's
formulas (no numpy complex multiply)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20250114
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


# ---------------------------------------------------------------------------
# the numpy reference

class Ref:
    """re / im: real arrays of the node's precision (im None: real valued)"""

    __array_ufunc__ = None  # numpy scalars on the left defer to __rmul__ etc.

    def __init__(self, re, im=None):
        self.re, self.im = np.asarray(re), (None if im is None else np.asarray(im))

    @staticmethod
    def of(a):
        a = np.asarray(a)
        return Ref(a.real.copy(), a.imag.copy()) if a.dtype.kind == "c" else Ref(a.copy())

    @staticmethod
    def lift(x, like):
        """a scalar operand as Julia types it next to a vector of like's element type"""
        if isinstance(x, Ref):
            return x
        if isinstance(x, complex):  # ComplexF64
            return Ref(np.float64(x.real), np.float64(x.imag))
        if isinstance(x, float):  # Float64
            return Ref(np.float64(x))
        T = like.elt  # ints and numpy scalars of T's width: a real of real(T), a complex one of T
        if np.iscomplexobj(x):
            return Ref(T(x.real), T(x.imag))
        return Ref(T(x))

    def _pair(self, o, swap=False):
        o = Ref.lift(o, self)
        p = np.result_type(self.re.dtype, o.re.dtype)
        a, b = self._as(p), o._as(p)
        a.elt = b.elt = self.elt
        a.cplx = b.cplx = self.cplx
        return (b, a) if swap else (a, b)

    def _as(self, p):
        return Ref(self.re.astype(p), None if self.im is None else self.im.astype(p))

    def _out(self, re, im):
        r = Ref(re, im)
        r.elt, r.cplx = self.elt, self.cplx
        return r

    def _add(a, b):  # Real + Complex keeps the imaginary part
        if a.im is None or b.im is None:
            return a._out(a.re + b.re, b.im if a.im is None else a.im)
        return a._out(a.re + b.re, a.im + b.im)

    def _sub(a, b):
        if b.im is None:
            return a._out(a.re - b.re, a.im)
        return a._out(a.re - b.re, -b.im if a.im is None else a.im - b.im)

    def _mul(a, b):
        if a.im is None and b.im is None:
            return a._out(a.re * b.re, None)
        if a.im is None:
            return a._out(a.re * b.re, a.re * b.im)
        if b.im is None:
            return a._out(a.re * b.re, a.im * b.re)
        return a._out(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re)

    def _div(a, b):
        assert a.im is None and b.im is None
        return a._out(a.re / b.re, None)

    def _cmp(a, b, f):
        t = f(a.re, b.re)
        if f in (np.equal, np.not_equal) and not (a.im is None and b.im is None):
            ai = a.im if a.im is not None else np.zeros_like(a.re)
            bi = b.im if b.im is not None else np.zeros_like(b.re)
            t = (a.re == b.re) & (ai == bi)
            t = t if f is np.equal else ~t
        return a._out(np.asarray(t).astype(a.elt), None)  # Julia's Bool: the other operand's type decides

    def __add__(self, o): return Ref._add(*self._pair(o))
    def __radd__(self, o): return Ref._add(*self._pair(o, True))
    def __sub__(self, o): return Ref._sub(*self._pair(o))
    def __rsub__(self, o): return Ref._sub(*self._pair(o, True))
    def __mul__(self, o): return Ref._mul(*self._pair(o))
    def __rmul__(self, o): return Ref._mul(*self._pair(o, True))
    def __truediv__(self, o): return Ref._div(*self._pair(o))
    def __rtruediv__(self, o): return Ref._div(*self._pair(o, True))
    def __lt__(self, o): return Ref._cmp(*self._pair(o), np.less)
    def __le__(self, o): return Ref._cmp(*self._pair(o), np.less_equal)
    def __gt__(self, o): return Ref._cmp(*self._pair(o), np.greater)
    def __ge__(self, o): return Ref._cmp(*self._pair(o), np.greater_equal)
    def __neg__(self): return self._out(-self.re, None if self.im is None else -self.im)

    def __abs__(self):
        assert self.im is None
        return self._out(np.abs(self.re), None)

    def store(self):
        """rounded to the element type once"""
        T = np.dtype(self.elt)
        if not self.cplx:
            return self.re.astype(T)
        out = np.empty(self.re.shape, np.result_type(T, np.complex64))
        out.real = self.re
        out.imag = 0 if self.im is None else self.im
        return out


class RefFns:
    @staticmethod
    def abs2(a):
        return a._out(a.re * a.re if a.im is None else a.re * a.re + a.im * a.im, None)

    @staticmethod
    def conj(a):
        return a._out(a.re, None if a.im is None else -a.im)

    @staticmethod
    def eq(a, b):
        return Ref._cmp(*a._pair(b), np.equal)

    @staticmethod
    def ne(a, b):
        return Ref._cmp(*a._pair(b), np.not_equal)


def _ref(a):
    r = Ref.of(a)
    r.cplx = np.asarray(a).dtype.kind == "c"
    r.elt = np.asarray(a).real.dtype.type
    return r


def _expected(f, *arrays):
    """f over host arrays, as an array of the element type"""
    r = f(RefFns, *[_ref(a) for a in arrays])
    out = r.store()
    return np.broadcast_to(out, arrays[0].shape).copy() if out.shape != arrays[0].shape else out


def _same(got, want):
    """bit-exact, the sign of zero included, up to NaN payloads"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "c":
        return _same(got.real.copy(), want.real.copy()) and _same(got.imag.copy(), want.imag.copy())
    num = ~np.isnan(want)  # a NaN's sign is not specified
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got[num]), np.signbit(want[num]))


# ---------------------------------------------------------------------------
# data

def _rand(rng, n, dtype, lo=-1.0, hi=1.0):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rng.uniform(lo, hi, n) + 1j * rng.uniform(lo, hi, n)).astype(dtype)
    return rng.uniform(lo, hi, n).astype(dtype)


def _pv(pamd, rng, rows, dtype, lo=-1.0, hi=1.0):
    """(PVector, {part: host values})"""
    host = {s.part: _rand(rng, s.num_lids, dtype, lo, hi) for s in rows.partition.parts}
    return pamd.PVector.from_host(pamd.map_parts(lambda s: host[s.part], rows.partition), rows, dtype), host


def _own(rows, p):
    return rows.partition.local(p).oid_to_lid - 1


def _hid(rows, p):
    return rows.partition.local(p).hid_to_lid - 1


def _check_full(got: "pamd.PVector", f, hosts):
    """all lids computed: every part's whole array"""
    g = got.to_host()
    for p in g.part_ids:
        want = _expected(f, *[h[p] for h in hosts])
        assert _same(g.local(p), want), f"part {p}"


def _check_owned(got, f, ops, before):
    """owned values computed through each operand's own index set, the
    result's ghosts left as they were (`before`)"""
    g = got.to_host()
    for p in g.part_ids:
        want = _expected(f, *[h[p][_own(v.rows, p)] for v, h in ops])
        assert _same(g.local(p)[_own(got.rows, p)], want), f"part {p}: owned values"
        hid = _hid(got.rows, p)
        assert _same(g.local(p)[hid], before[p][hid]), f"part {p}: a ghost was written"


# the expressions of test_interfaces.jl:504-577; F: the functions namespace
# (pamd or RefFns); the label names the operands used
EXPRS = [
    ("2*v", lambda F, v, u, w: 2 * v),
    ("v+u", lambda F, v, u, w: v + u),
    ("v-u", lambda F, v, u, w: v - u),
    ("1+v", lambda F, v, u, w: 1 + v),
    ("v+1", lambda F, v, u, w: v + 1),
    ("v+w-u", lambda F, v, u, w: v + w - u),
    ("v+1-u", lambda F, v, u, w: v + 1 - u),
]
ASSIGNS = [
    ("w.=v-1-u", lambda F, v, u, w: v - 1 - u),
    ("w.=u", lambda F, v, u, w: u),
]


@pytest.fixture(scope="module")
def stencil(be, pamd):
    parts = be.get_part_ids((2, 2, 1))
    rows, cols = pamd.drivers.stencil_partition(parts, (5, 5, 3), 27)
    assert sorted(s.num_oids for s in cols.partition.parts) == [12, 18, 18, 27]
    assert not rows.ghost or all(s.num_hids == 0 for s in rows.partition.parts)
    assert all(s.num_hids > 0 for s in cols.partition.parts)
    return parts, rows, cols


def _run_exprs(pamd, rng, dtype, rv, ru, rw):
    """EXPRS through materialize and ASSIGNS through assign_ with v, u, w on
    the PRanges rv, ru, rw; ghosts are computed iff the PVector operands of the
    expression (and w, for assign_) share one rows object"""
    rows_of = {"v": rv, "u": ru, "w": rw}
    (v, hv), (u, hu), (w0, hw) = _pv(pamd, rng, rv, dtype), _pv(pamd, rng, ru, dtype), _pv(pamd, rng, rw, dtype)
    ops = [(v, hv), (u, hu), (w0, hw)]
    for label, f in EXPRS:
        used = [c for c in "vuw" if c in label]
        got = pamd.materialize(f(pamd, v, u, w0))
        assert got.rows is rows_of[used[0]] and got.dtype == np.dtype(dtype)
        if all(rows_of[c] is rows_of[used[0]] for c in used):
            _check_full(got, f, [hv, hu, hw])
        else:  # a fresh vector: its ghosts stay zero
            zero = {p: np.zeros(s.num_lids, dtype) for p, s in zip(got.values.part_ids, got.rows.partition.parts)}
            _check_owned(got, f, ops, zero)
    for label, f in ASSIGNS:
        used = [c for c in "vuw" if c in label.split("=")[1]]
        sentinel = {p: np.full(s.num_lids, 7.5, dtype) for p, s in zip(w0.values.part_ids, rw.partition.parts)}
        w = pamd.PVector.from_host(pamd.map_parts(lambda s: sentinel[s.part], rw.partition), rw, dtype)
        assert pamd.assign_(w, f(pamd, v, u, w)) is w
        if all(rows_of[c] is rw for c in used):
            _check_full(w, f, [hv, hu, sentinel])
        else:
            _check_owned(w, f, [(v, hv), (u, hu), (w, sentinel)], sentinel)


@pytest.mark.parametrize("dtype", DTYPES)
def test_interface_expressions_shared_rows(be, pamd, stencil, dtype):
    """every operand on cols: all lids, ghosts included (16 B steps; owned +
    ghost counts leave tails of 0-3 elements)"""
    _, rows, cols = stencil
    _run_exprs(pamd, np.random.default_rng(SEED), dtype, cols, cols, cols)


@pytest.mark.parametrize("dtype", DTYPES)
def test_interface_expressions_owned_only(be, pamd, stencil, dtype):
    """u on rows, v and w on cols (test_interfaces.jl:558-580): owned values
    only — counts 27 and 18 leave tails of 3 and 2 after whole Float32 steps,
    27 a tail of 1 in Float64 — and w's ghosts keep their sentinel"""
    _, rows, cols = stencil
    _run_exprs(pamd, np.random.default_rng(SEED + 1), dtype, cols, rows, cols)


TYPE_RULE = [
    (np.float32, "(v+u)*2.0", lambda F, v, u: (v + u) * 2.0),
    (np.float32, "(v+u)*f32(2)", lambda F, v, u: (v + u) * np.float32(2)),
    (np.float32, "(v+u)*0.1", lambda F, v, u: (v + u) * 0.1),
    (np.float32, "(v+u)*f32(0.1)", lambda F, v, u: (v + u) * np.float32(0.1)),
    (np.float32, "(v*u)*3.0", lambda F, v, u: (v * u) * 3.0),
    (np.float32, "0.1*v+u*u", lambda F, v, u: 0.1 * v + u * u),
    (np.complex64, "2.0*v+(1+2j)*u", lambda F, v, u: 2.0 * v + (1 + 2j) * u),
    (np.complex64, "abs2(v)*u-0.5*v", lambda F, v, u: F.abs2(v) * u - 0.5 * v),
    (np.complex128, "2.0*v+(1+2j)*u", lambda F, v, u: 2.0 * v + (1 + 2j) * u),
    (np.complex128, "v*u-conj(u)*3", lambda F, v, u: v * u - F.conj(u) * 3),
    (np.float32, "v/u", lambda F, v, u: v / u),
    (np.float64, "v/u", lambda F, v, u: v / u),
    (np.float32, "1.0/u", lambda F, v, u: 1.0 / u),
    (np.float32, "f32(3)/u-v", lambda F, v, u: np.float32(3) / u - v),
    (np.float32, "abs(v)", lambda F, v, u: abs(v)),
    (np.float64, "abs(v-u)", lambda F, v, u: abs(v - u)),
    (np.complex64, "abs2(v)", lambda F, v, u: F.abs2(v)),
    (np.complex128, "abs2(v)", lambda F, v, u: F.abs2(v)),
    (np.float32, "abs2(v)", lambda F, v, u: F.abs2(v)),
    (np.float32, "-v", lambda F, v, u: -v),
    (np.complex64, "-v", lambda F, v, u: -v),
    (np.complex64, "conj(v)", lambda F, v, u: F.conj(v)),
    (np.float64, "conj(v)", lambda F, v, u: F.conj(v)),
    (np.float64, "(v>u)*v", lambda F, v, u: (v > u) * v),
    (np.float32, "(v<=0.25)+(u>=v)", lambda F, v, u: (v <= 0.25) + (u >= v)),
    (np.complex64, "eq(v,u)+ne(v,v)", lambda F, v, u: F.eq(v, u) + F.ne(v, v)),
    (np.float64, "v-(u-(v-(u-(v-u))))", lambda F, v, u: v - (u - (v - (u - (v - u))))),
    (np.float32, "((v+u)*(v-u))-((u*v)*(u+0.5))", lambda F, v, u: ((v + u) * (v - u)) - ((u * v) * (u + 0.5))),
]


@pytest.mark.parametrize("dtype,label,f", TYPE_RULE, ids=[f"{np.dtype(d).name}:{s}" for d, s, _ in TYPE_RULE])
def test_type_rule(be, pamd, stencil, dtype, label, f):
    """each node in its inferred type: a Float32 op in Float32, an op with a
    Float64 / ComplexF64 scalar or a wide operand in the wide type, one
    rounding on the store; Float32 division correctly rounded; u away from 0"""
    _, rows, cols = stencil
    rng = np.random.default_rng(SEED + 2)
    v, hv = _pv(pamd, rng, cols, dtype)
    u, hu = _pv(pamd, rng, cols, dtype, 0.5, 1.5)
    _check_full(pamd.materialize(f(pamd, v, u)), f, [hv, hu])


REAL_SCALAR = [
    ("1+v", lambda F, v: 1 + v),
    ("v-1", lambda F, v: v - 1),
    ("1-v", lambda F, v: 1 - v),
    ("2*v", lambda F, v: 2 * v),
    ("v*f32(2)", lambda F, v: v * np.float32(2)),
    ("2.0*v", lambda F, v: 2.0 * v),
    ("v+0.0", lambda F, v: v + 0.0),
    ("(1+0j)*v", lambda F, v: (1 + 0j) * v),
    ("-v", lambda F, v: -v),
    ("eq(v,2)*v", lambda F, v: F.eq(v, 2) * v),
]


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_real_scalars_over_complex_vectors(be, pamd, stencil, dtype):
    """Julia's Real ∘ Complex methods: 1 + v keeps an imaginary -0.0, 2 * v is
    (2re, 2im) also where a component is Inf; a complex scalar takes the full
    formula (Inf * 0 = NaN).  Signed zeros, Inf and NaN in the data."""
    _, rows, cols = stencil
    rng = np.random.default_rng(SEED + 11)
    v, hv = _pv(pamd, rng, cols, dtype)
    special = np.array([complex(1.5, -0.0), complex(-0.0, 2.0), complex(np.inf, 1.0), complex(2.0, -np.inf),
                        complex(-0.0, -0.0), complex(np.nan, 0.0), complex(2.0, 0.0)], dtype)
    for p in hv:
        hv[p][:len(special)] = special
    v = pamd.PVector.from_host(pamd.map_parts(lambda s: hv[s.part], cols.partition), cols, dtype)
    with np.errstate(invalid="ignore"):
        for label, f in REAL_SCALAR:
            got = pamd.materialize(f(pamd, v)).to_host()
            for p in got.part_ids:
                assert _same(got.local(p), _expected(f, hv[p])), f"{label}, part {p}"
    one = pamd.materialize(1 + v).to_host().local(1)
    assert np.signbit(one[0].imag) and one[0].real == 2.5  # 1 + (1.5 - 0.0im) == 2.5 - 0.0im
    two = pamd.materialize(2 * v).to_host().local(1)
    assert two[2] == complex(np.inf, 2.0) and two[3] == complex(4.0, -np.inf)


def test_wide_scalar_changes_the_bits(be, pamd, stencil):
    """the Float64 scalar's node is evaluated in Float64: 0.1 and Float32(0.1)
    differ, and so do the results somewhere"""
    _, rows, cols = stencil
    rng = np.random.default_rng(SEED + 3)
    v, _ = _pv(pamd, rng, cols, np.float32)
    a = pamd.materialize(v * 0.1).to_host()
    b = pamd.materialize(v * np.float32(0.1)).to_host()
    assert any(not np.array_equal(x, y) for x, y in zip(a.parts, b.parts))


@pytest.mark.parametrize("dtype", DTYPES)
def test_aliasing(be, pamd, stencil, dtype):
    """w on both sides: w .= v .- 1 .- w and w .= w .* w (same-index access)"""
    _, rows, cols = stencil
    rng = np.random.default_rng(SEED + 4)
    v, hv = _pv(pamd, rng, cols, dtype)
    w, hw = _pv(pamd, rng, cols, dtype)
    f = lambda F, v, w: v - 1 - w
    pamd.assign_(w, f(pamd, v, w))
    _check_full(w, f, [hv, hw])
    hw = {p: a.copy() for p, a in zip(w.values.part_ids, w.to_host().parts)}
    g = lambda F, w: w * w
    pamd.assign_(w, g(pamd, w))
    _check_full(w, g, [hw])
    # owned only: u on rows, w on cols on both sides
    u, hu = _pv(pamd, rng, rows, dtype)
    hw = {p: a.copy() for p, a in zip(w.values.part_ids, w.to_host().parts)}
    h = lambda F, u, w: u - w * 2
    pamd.assign_(w, h(pamd, u, w))
    _check_owned(w, h, [(u, hu), (w, hw)], hw)


# ---------------------------------------------------------------------------
# lengths below one 16 B step, an empty part

@pytest.fixture(scope="module")
def tiny(be, pamd):
    parts = be.get_part_ids(3)
    noids = pamd.PData(parts.backend, parts.part_ids, [3, 0, 1], parts.shape)
    return pamd.prange_noids(parts, noids)


def _cat_owned(v, host):
    return np.concatenate([host[p][_own(v.rows, p)] for p in v.values.part_ids])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tiny_and_empty_parts(be, pamd, tiny, dtype):
    rng = np.random.default_rng(SEED + 5)
    v, hv = _pv(pamd, rng, tiny, dtype)
    u, hu = _pv(pamd, rng, tiny, dtype, 0.5, 1.5)
    for f in (lambda F, v, u: v + u * 2.0, lambda F, v, u: v / u - 1, lambda F, v, u: F.abs2(v) - u):
        _check_full(pamd.materialize(f(pamd, v, u)), f, [hv, hu])
    allv = _cat_owned(v, hv)
    assert pamd.maximum(v) == allv.max() and pamd.minimum(v) == allv.min()
    assert pamd.maximum(abs(v)) == np.abs(allv).max() == pamd.norm(v, math.inf)
    tol = 1e-12 if np.dtype(dtype) == np.float64 else 1e-6
    want = float(np.sum(_expected(lambda F, v, u: v * u + 2.0, allv, _cat_owned(u, hu)).astype(np.float64)))
    assert abs(pamd.psum(v * u + 2.0) - want) <= tol * abs(want)
    assert pamd.any_(v > -2.0) and not pamd.any_(v > 2.0) and pamd.all_(v < 2.0) and not pamd.all_(v < -2.0)
    assert pamd.isequal(v, v.copy())
    # one owned element of the last part differs (its only one, behind the empty part)
    hw = {p: a.copy() for p, a in hv.items()}
    hw[3][0] += 1
    w = pamd.PVector.from_host(pamd.map_parts(lambda s: hw[s.part], tiny.partition), tiny, dtype)
    assert pamd.isequal(v, w) is False and pamd.isequal(w, v) is False
    # a NaN in an owned slot (the tail path; the fold crosses the empty part's -Inf / +Inf)
    for part, slot in ((1, 2), (3, 0)):
        hn = {p: a.copy() for p, a in hv.items()}
        hn[part][slot] = np.nan
        wn = pamd.PVector.from_host(pamd.map_parts(lambda s: hn[s.part], tiny.partition), tiny, dtype)
        assert math.isnan(pamd.maximum(wn)) and math.isnan(pamd.minimum(wn)) and math.isnan(pamd.maximum(abs(wn)))
        assert not pamd.isequal(wn, wn.copy())
    # the distances and norms
    allu = _cat_owned(u, hu)
    d2 = float(np.sum(_expected(lambda F, a, b: F.abs2(a - b), allv, allu).astype(np.float64)))
    assert abs(pamd.sqeuclidean(v, u) - d2) <= tol * d2
    assert abs(pamd.euclidean(v, u) - math.sqrt(d2)) <= tol * math.sqrt(d2)
    diff = pamd.materialize(v - u)
    assert abs(pamd.euclidean(v, u) - pamd.norm(diff)) <= tol * pamd.norm(diff)
    n1 = float(np.sum(np.abs(allv).astype(np.float64)))
    assert abs(pamd.norm(v, 1) - n1) <= tol * n1
    assert pamd.minimum(pamd.abs2(v)) == (allv * allv).min()
    # the empty part alone contributes SUM 0, MAX -Inf, MIN +Inf
    parts1 = be.get_part_ids(1)
    empty = pamd.prange_noids(parts1, pamd.PData(parts1.backend, parts1.part_ids, [0], parts1.shape))
    z = pamd.PVector.undef(empty, dtype)
    assert pamd.psum(z + 1) == 0 and pamd.maximum(z) == -math.inf and pamd.minimum(z) == math.inf
    assert pamd.all_(z > 0) and not pamd.any_(z > -1) and pamd.isequal(z, z.copy())


# ---------------------------------------------------------------------------
# mapped path: owned lids interleaved with ghosts

@pytest.fixture(scope="module")
def interleaved(be, pamd):
    parts = be.get_part_ids((2, 2))
    mk = lambda ghost: pamd.prange_cartesian(parts, (5, 5), with_ghost=ghost, isperiodic=(True, False))
    g1, g2, plain = mk(True), mk(True), mk(False)
    assert any(not np.array_equal(s.oid_to_lid, np.arange(1, s.num_oids + 1)) for s in g1.partition.parts)
    assert g1 is not g2 and pamd.oids_are_equal(g1, g2) and pamd.oids_are_equal(g1, plain)
    return g1, g2, plain


@pytest.mark.parametrize("dtype", DTYPES)
def test_mapped_path(be, pamd, interleaved, dtype):
    g1, g2, plain = interleaved
    rng = np.random.default_rng(SEED + 6)
    _run_exprs(pamd, rng, dtype, g1, g1, g1)      # one PRange: all lids
    _run_exprs(pamd, rng, dtype, g1, g2, g1)      # equal owned ids, another object: gathers through every map
    _run_exprs(pamd, rng, dtype, g1, plain, g1)   # a ghostless operand (identity) among mapped ones
    _run_exprs(pamd, rng, dtype, plain, g1, g2)   # the result on the ghostless PRange, w mapped


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex64])
def test_mapped_reductions(be, pamd, interleaved, dtype):
    g1, g2, plain = interleaved
    rng = np.random.default_rng(SEED + 7)
    (a, ha), (b, hb) = _pv(pamd, rng, g1, dtype), _pv(pamd, rng, plain, dtype)
    ca, cb = _cat_owned(a, ha), _cat_owned(b, hb)
    tol = 1e-12 if np.dtype(dtype) == np.float64 else 1e-6
    want = float(np.sum(_expected(lambda F, a, b: F.abs2(a - b), ca, cb).real.astype(np.float64)))
    assert abs(pamd.sqeuclidean(a, b) - want) <= tol * want
    m = _expected(lambda F, a, b: F.abs2(a) - F.abs2(b), ca, cb).real
    assert pamd.maximum(pamd.abs2(a) - pamd.abs2(b)) == m.max()
    assert pamd.minimum(pamd.abs2(a) - pamd.abs2(b)) == m.min()
    assert not pamd.isequal(a, b)
    c = pamd.PVector.undef(g2, dtype)
    pamd.copyto_(c, a)  # owned values only: c's ghosts stay zero, a's are random
    assert pamd.isequal(a, c) and pamd.isequal(c, a)


# ---------------------------------------------------------------------------
# grid-stride: just above one full pass of the fast-path grid

def test_grid_stride(be, pamd):
    """Float64, 8192 blocks x 256 lanes x 2 elements per step, + 3: one whole
    pass of the grid, one lane taking a second step, and one tail element"""
    n = 8192 * 256 * 2 + 3
    parts = be.get_part_ids(1)
    rows = pamd.prange_linear(parts, n)
    rng = np.random.default_rng(SEED + 8)
    (v, hv), (u, hu), (z, hz) = (_pv(pamd, rng, rows, np.float64, 0.5, 1.5) for _ in range(3))
    f = lambda F, v, u, z: v + 2.0 * u - z
    _check_full(pamd.materialize(f(pamd, v, u, z)), f, [hv, hu, hz])
    g = lambda F, v, u, z: v * u + z
    want = float(np.sum(_expected(g, hv[1], hu[1], hz[1])))
    assert abs(pamd.psum(g(pamd, v, u, z)) - want) <= 1e-12 * want
    assert pamd.maximum(g(pamd, v, u, z)) == _expected(g, hv[1], hu[1], hz[1]).max()


# ---------------------------------------------------------------------------
# reductions

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_extrema_predicates_isequal(be, pamd, stencil, dtype):
    _, rows, cols = stencil
    rng = np.random.default_rng(SEED + 9)
    v, hv = _pv(pamd, rng, cols, dtype)
    allv = _cat_owned(v, hv)
    assert pamd.maximum(v) == allv.max() and pamd.minimum(v) == allv.min()
    assert pamd.maximum(abs(v)) == np.abs(allv).max() == pamd.norm(v, math.inf)
    assert pamd.minimum(pamd.abs2(v)) == (allv * allv).min()
    for c in (-2.0, 0.0, 2.0):  # below, inside and above the data's range
        assert pamd.any_(v > c) == bool((allv > c).any())
        assert pamd.all_(v < c) == bool((allv < c).all())
        assert pamd.any_(v <= dtype(c)) == bool((allv <= c).any())
        assert pamd.all_(v >= dtype(c)) == bool((allv >= c).all())
    assert pamd.isequal(v, v.copy())
    last = v.values.part_ids[-1]
    for slot, equal in ((_own(cols, last)[-1], False), (_hid(cols, last)[0], True)):
        hw = {p: a.copy() for p, a in hv.items()}
        hw[last][slot] += 1  # one owned element of one part / one ghost
        w = pamd.PVector.from_host(pamd.map_parts(lambda s: hw[s.part], cols.partition), cols, dtype)
        assert pamd.isequal(v, w) is equal and pamd.isequal(w, v) is equal
    # a NaN in an owned slot gives NaN, a NaN in a ghost slot only does not
    for slot, nan in ((_own(cols, 2)[5], True), (_hid(cols, 2)[-1], False)):
        hw = {p: a.copy() for p, a in hv.items()}
        hw[2][slot] = np.nan
        w = pamd.PVector.from_host(pamd.map_parts(lambda s: hw[s.part], cols.partition), cols, dtype)
        if nan:
            assert math.isnan(pamd.maximum(w)) and math.isnan(pamd.minimum(w)) and math.isnan(pamd.maximum(abs(w)))
            assert not pamd.isequal(w, w.copy())  # NaN != NaN, as Julia's ==
        else:
            assert pamd.maximum(w) == allv.max() and pamd.minimum(w) == allv.min()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_and_distances(be, pamd, stencil, dtype):
    """psum(expr), sqeuclidean, euclidean, norm(a, 1) within the reduction
    tolerance of test_gpu_parity.py's dot / norm / sum"""
    _, rows, cols = stencil
    rng = np.random.default_rng(SEED + 10)
    (a, ha), (b, hb) = _pv(pamd, rng, cols, dtype), _pv(pamd, rng, rows, dtype)
    ca, cb = _cat_owned(a, ha), _cat_owned(b, hb)
    tol = 1e-12 if np.dtype(dtype) in (np.float64, np.complex128) else 1e-6
    f = lambda F, a, b: a * b + 2.0
    want = complex(np.sum(_expected(f, ca, cb).astype(np.complex128)))
    assert abs(pamd.psum(f(pamd, a, b)) - want) <= tol * abs(want)
    d2 = float(np.sum(_expected(lambda F, a, b: F.abs2(a - b), ca, cb).real.astype(np.float64)))
    assert abs(pamd.sqeuclidean(a, b) - d2) <= tol * d2
    assert isinstance(pamd.sqeuclidean(a, b), float)
    assert abs(pamd.euclidean(a, b) - math.sqrt(d2)) <= tol * math.sqrt(d2)
    diff = pamd.materialize(a - b)  # on cols; its ghosts (zero) do not count
    assert abs(pamd.euclidean(a, b) - pamd.norm(diff)) <= tol * pamd.norm(diff)
    if np.dtype(dtype).kind == "f":
        n1 = float(np.sum(np.abs(ca).astype(np.float64)))
        assert abs(pamd.norm(a, 1) - n1) <= tol * n1
        assert pamd.norm(a, math.inf) == np.abs(ca).max()
        assert pamd.norm(a) == pamd.norm(a, 2)
    # the named fast paths and psum of a vector keep their entry points
    assert abs(pamd.psum(a) - complex(np.sum(ca.astype(np.complex128)))) <= tol * max(1.0, abs(np.sum(ca)))
