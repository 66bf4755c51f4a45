"""The named vector operations on the device (xpby_, axpy_, axmy_, sub_,
rmul_, copyto_, copy, fill_ through pa_vec_axpby / pa_vec_copy / pa_vec_fill;
dot, norm, psum through pa_dot_all / pa_norm2_all / pa_sum_all) against the
independent reference of blas1_ref.py.

Elementwise results are bit for bit over each part's whole array, ghost
slots included.  Reductions are exact on the k * 2**-10 family (no summation
order can change a bit there) and within an order-free bound of the exact
rational result on random data."""
import math
from fractions import Fraction

import numpy as np
import pytest

import blas1_ref as R

pytestmark = pytest.mark.gpu

SEED = 20250321
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
_ids = lambda ds: [np.dtype(d).name for d in ds]


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


# ---------------------------------------------------------------------------
# layouts and data

@pytest.fixture(scope="module")
def layouts(be, pamd):
    """The 2x2-part periodic 5x5 grid: g1, g2 two objects with one layout
    (owned lids interleaved with ghosts), plain the ghostless range, and c =
    plain + add_gids of g1's ghosts: g1's lids in another order."""
    parts = be.get_part_ids((2, 2))
    mk = lambda ghost: pamd.prange_cartesian(parts, (5, 5), with_ghost=ghost, isperiodic=(True, False))
    g1, g2, plain = mk(True), mk(True), mk(False)
    ghosts = pamd.map_parts(lambda s: s.lid_to_gid[s.hid_to_lid - 1].copy(), g1.partition)
    c = pamd.add_gids(plain, ghosts)
    nl = lambda r: [s.num_lids for s in r.partition.parts]
    assert any(not np.array_equal(s.oid_to_lid, np.arange(1, s.num_oids + 1)) for s in g1.partition.parts)
    assert g1 is not g2 and g1.partition is not g2.partition
    assert pamd.oids_are_equal(g1, g2) and pamd.lids_are_equal(g1, g2)
    assert pamd.oids_are_equal(g1, c) and not pamd.lids_are_equal(g1, c) and nl(g1) == nl(c) == [12, 15, 16, 20]
    assert pamd.oids_are_equal(g1, plain) and not pamd.lids_are_equal(g1, plain) and nl(plain) == [4, 6, 6, 9]
    assert all(s.num_hids > 0 for s in c.partition.parts) and all(s.num_hids == 0 for s in plain.partition.parts)
    return {"g1": g1, "g2": g2, "c": c, "plain": plain}


# (y's range, x's range, every lid updated?)
LAYOUTS = {
    "a": ("g1", "g1", True),      # the same PRange
    "b": ("g1", "g2", False),     # two objects, one layout
    "c": ("g1", "c", False),      # equal lid counts, another lid order
    "c'": ("c", "g1", False),
    "d": ("plain", "g1", False),  # ghostless against ghosted
    "d'": ("g1", "plain", False),
}


def _real(dtype):
    return np.zeros(1, dtype).real.dtype.type


def _rand(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def _specials(dtype):
    """signed zeros, infinities, NaN and two subnormals of the real type (as
    re with a random im, and as im, for complex types); complex(inf, 1) is
    where a real scalar's componentwise product and the complex product with
    (a, 0) differ"""
    r = _real(dtype)
    tiny = np.finfo(r).smallest_subnormal
    vals = [r(0.0), r(-0.0), r(np.inf), r(-np.inf), r(np.nan), tiny, r(-(2 ** 20 + 1)) * tiny]
    if np.dtype(dtype).kind != "c":
        return np.array(vals + [r(1.0)], dtype)
    out = [complex(v, 0.75) for v in vals[:4]] + [complex(-0.5, v) for v in vals[4:]] + [complex(np.inf, 1.0)]
    return np.array(out, dtype)


def _host(rng, rows, dtype, shift):
    """random values per part with specials in two owned and two ghost slots
    of every part; over the four parts each special lands in an owned slot"""
    sp = _specials(dtype)
    host = {}
    for k, s in enumerate(rows.partition.parts):
        h = _rand(rng, s.num_lids, dtype)
        own, hid = s.oid_to_lid - 1, s.hid_to_lid - 1
        for j in range(min(2, len(own))):
            h[own[-1 - j]] = sp[(2 * k + j + shift) % len(sp)]
        for j in range(min(2, len(hid))):
            h[hid[j]] = sp[(2 * k + j + shift + 3) % len(sp)]
        host[s.part] = h
    return host


def _up(pamd, host, rows, dtype):
    return pamd.PVector.from_host(pamd.map_parts(lambda s: host[s.part].copy(), rows.partition), rows, dtype)


def _own(rows, p):
    return rows.partition.local(p).oid_to_lid - 1


def _scalars(dtype):
    """(label, scalar) of every kind the type allows"""
    T = np.dtype(dtype).type
    if np.dtype(dtype).kind == "c":
        return [("T", T(0.37 + 0.11j)), ("int", 3), ("float", 0.1), ("complex", 0.3 - 0.7j)]
    return [("T", T(0.37)), ("int", 3), ("float", 0.1), ("complex0", complex(0.1, 0.0))]


def _call(pamd, op, y, x, a):
    if op == "xpby":
        return pamd.xpby_(y, x, a)
    if op == "axpy":
        return pamd.axpy_(y, a, x)
    if op == "axmy":
        return pamd.axmy_(y, a, x)
    if op == "sub":
        return pamd.sub_(y, x)
    return pamd.rmul_(y, a)


def _want(op, hy, hx, a, ry, rx, full):
    """per part: the whole expected array of y after op"""
    out = {}
    for p, y in hy.items():
        if full or op == "rmul":  # rmul! always touches all lids
            out[p] = R.bcast(op, y, None if op == "rmul" else hx[p], a)
        else:
            w = y.copy()
            oy = _own(ry, p)
            w[oy] = R.bcast(op, y[oy], hx[p][_own(rx, p)], a)
            out[p] = w
    return out


def _assert_parts(v, want, what):
    got = v.to_host()
    for p in got.part_ids:
        assert R.same_bits(got.local(p), want[p]), f"{what}, part {p}:\n got {got.local(p)}\nwant {want[p]}"


# ---------------------------------------------------------------------------
# elementwise

def test_the_data_tells_the_paths_apart(layouts):
    """host only: over the data below a Float64 scalar's wide evaluation and
    the all-Float32 one differ somewhere, and so do a real scalar's
    componentwise product and the complex product over complex vectors"""
    g1 = layouts["g1"]
    for dtype in (np.float32, np.complex64, np.complex128):
        rng = np.random.default_rng(SEED)
        hy, hx = _host(rng, g1, dtype, 0), _host(rng, g1, dtype, 5)
        for op in ("xpby", "axpy", "axmy", "rmul"):
            wide = [R.bcast(op, hy[p], hx[p], 0.1) for p in hy]
            if dtype != np.complex128:
                narrow = [R.bcast(op, hy[p], hx[p], 0.1, kind="T") for p in hy]
                assert any(not R.same_bits(w, n) for w, n in zip(wide, narrow)), (dtype, op)
            if np.dtype(dtype).kind == "c":
                full = [R.bcast(op, hy[p], hx[p], 0.1, kind="c128") for p in hy]
                assert any(not R.same_bits(w, f) for w, f in zip(wide, full)), (dtype, op)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_named_broadcasts(be, pamd, layouts, dtype, layout):
    ny, nx, full = LAYOUTS[layout]
    ry, rx = layouts[ny], layouts[nx]
    rng = np.random.default_rng(SEED)
    hy, hx = _host(rng, ry, dtype, 0), _host(rng, rx, dtype, 5)
    x = _up(pamd, hx, rx, dtype)
    for op in R.OPS:
        for label, a in ([("none", None)] if op == "sub" else _scalars(dtype)):
            y = _up(pamd, hy, ry, dtype)
            assert _call(pamd, op, y, x, a) is y
            _assert_parts(y, _want(op, hy, hx, a, ry, rx, full), f"{op} with {label} scalar {a!r}")
    _assert_parts(x, hx, "the operand x")
    if np.dtype(dtype).kind != "c":  # a complex scalar with an imaginary part into a real vector
        for op in ("xpby", "axpy", "axmy", "rmul"):
            y = _up(pamd, hy, ry, dtype)
            with pytest.raises(TypeError):
                _call(pamd, op, y, x, complex(0.1, 0.5))
            _assert_parts(y, hy, f"{op} after the TypeError")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_aliasing(be, pamd, layouts, dtype):
    """axpy_(x, a, x) and xpby_(u, u, b): y and x are one vector"""
    g1 = layouts["g1"]
    hx = _host(np.random.default_rng(SEED + 1), g1, dtype, 2)
    for label, a in _scalars(dtype):
        x = _up(pamd, hx, g1, dtype)
        pamd.axpy_(x, a, x)
        _assert_parts(x, {p: R.bcast("axpy", h, h, a) for p, h in hx.items()}, f"axpy_(x, {a!r}, x)")
        u = _up(pamd, hx, g1, dtype)
        pamd.xpby_(u, u, a)
        _assert_parts(u, {p: R.bcast("xpby", h, h, a) for p, h in hx.items()}, f"xpby_(u, u, {a!r})")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_tiny_and_empty_parts(be, pamd, dtype):
    """parts of 3, 0 and 1 owned values"""
    parts = be.get_part_ids(3)
    rows = pamd.prange_noids(parts, pamd.PData(parts.backend, parts.part_ids, [3, 0, 1], parts.shape))
    rng = np.random.default_rng(SEED + 2)
    hy = {s.part: _rand(rng, s.num_lids, dtype) for s in rows.partition.parts}
    hx = {s.part: _rand(rng, s.num_lids, dtype) for s in rows.partition.parts}
    hx[1][1] = _specials(dtype)[1]
    hy[3][0] = _specials(dtype)[5]
    x = _up(pamd, hx, rows, dtype)
    for op in R.OPS:
        for label, a in ([("none", None)] if op == "sub" else _scalars(dtype)):
            y = _up(pamd, hy, rows, dtype)
            _call(pamd, op, y, x, a)
            _assert_parts(y, _want(op, hy, hx, a, rows, rows, True), f"{op} with {label} scalar")


@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=_ids([np.float64, np.complex64]))
def test_grid_stride(be, pamd, dtype):
    """8192 blocks x 256 lanes + 3 values on one part: one full pass of
    k_axpby's grid, one lane's second step and a tail"""
    n = 8192 * 256 + 3
    parts = be.get_part_ids(1)
    rows = pamd.prange_linear(parts, n)
    rng = np.random.default_rng(SEED + 3)
    hy, hx = {1: _rand(rng, n, dtype)}, {1: _rand(rng, n, dtype)}
    x = _up(pamd, hx, rows, dtype)
    for op, a in (("axpy", 0.1), ("xpby", _scalars(dtype)[0][1])):
        y = _up(pamd, hy, rows, dtype)
        _call(pamd, op, y, x, a)
        got = y.to_host().local(1)
        want = R.bcast(op, hy[1], hx[1], a)
        assert R.same_bits(got, want), f"{op}: first differing index {np.flatnonzero(got != want)[:4]} of {n}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_copy_and_fill(be, pamd, layouts, dtype):
    g1 = layouts["g1"]
    rng = np.random.default_rng(SEED + 4)
    hb = _host(rng, g1, dtype, 1)
    b = _up(pamd, hb, g1, dtype)
    # the same partition: all lids
    a = _up(pamd, _host(rng, g1, dtype, 4), g1, dtype)
    assert pamd.copyto_(a, b) is a
    _assert_parts(a, hb, "copyto_ on one partition")
    cp = b.copy()
    assert cp is not b and cp.rows is b.rows and cp.dtype == np.dtype(dtype)
    _assert_parts(cp, hb, "copy")
    _assert_parts(b, hb, "the source")
    # across layouts: owned values only, the destination's ghosts as they were
    for nd, ns in (("g2", "g1"), ("g1", "c"), ("c", "g1"), ("plain", "g1"), ("g1", "plain")):
        rd, rs = layouts[nd], layouts[ns]
        hd, hs = _host(rng, rd, dtype, 3), _host(rng, rs, dtype, 6)
        d, s = _up(pamd, hd, rd, dtype), _up(pamd, hs, rs, dtype)
        pamd.copyto_(d, s)
        want = {}
        for p in hd:
            want[p] = hd[p].copy()
            want[p][_own(rd, p)] = hs[p][_own(rs, p)]
        _assert_parts(d, want, f"copyto_ {nd} <- {ns}")
        _assert_parts(s, hs, "the source")
    # fill!: all lids; a Python float into Float32 is rounded once
    T = np.dtype(dtype).type
    kinds = [T(0.37), 3, 0.1] + ([0.3 - 0.7j, T(0.37 + 0.11j)] if np.dtype(dtype).kind == "c" else [])
    for v in kinds:
        f = _up(pamd, hb, g1, dtype)
        assert f.fill_(v) is f
        _assert_parts(f, {p: np.full(len(h), T(v), dtype) for p, h in hb.items()}, f"fill_({v!r})")
    if dtype == np.float32:
        got = pamd.PVector.full(0.1, g1, dtype).to_host().local(1)
        assert float(T(0.1)) != 0.1 and got.dtype == np.float32 and float(got[0]) == float(np.float32(0.1))
    z = _up(pamd, hb, g1, dtype).fill_(-0.0)
    assert all(np.signbit(h.real).all() for h in z.to_host().parts)


def test_argument_errors(be, pamd, layouts):
    """what the C entries reject, each with its message; y stays as it was"""
    L, PAError = pamd._lib, pamd._lib.PAError
    g1 = layouts["g1"]
    rng = np.random.default_rng(SEED + 5)
    hy, hx = _host(rng, g1, np.float64, 0), _host(rng, g1, np.float64, 1)
    hz = _host(rng, g1, np.complex128, 0)
    y, x = _up(pamd, hy, g1, np.float64), _up(pamd, hx, g1, np.float64)
    x32 = _up(pamd, {p: h.astype(np.float32) for p, h in hx.items()}, g1, np.float32)
    z = _up(pamd, hz, g1, np.complex128)
    idx = pamd.device_index(y.values.parts[0].ctx, g1.partition.local(1)).h
    buf = np.array([0.5, 0.25])  # 16 bytes: a scalar of any kind
    bp = buf.ctypes.data
    dy, dx = y.values.parts[0], x.values.parts[0]

    def axpby(yv, xv, mode, all_lids=1):
        L.call("pa_vec_axpby", yv.h, xv.h if xv is not None else None, idx, bp, mode, all_lids)

    with pytest.raises(PAError, match="invalid axpby mode"):
        axpby(dy, dx, 5)
    with pytest.raises(PAError, match="invalid axpby mode"):
        axpby(dy, dx, 5 | L.PA_BCAST_F64)
    with pytest.raises(PAError, match="one scalar kind"):
        axpby(dy, dx, 1 | L.PA_BCAST_F64 | L.PA_BCAST_C128)
    with pytest.raises(PAError, match="ComplexF64 scalar into a real vector"):
        axpby(dy, dx, 1 | L.PA_BCAST_C128)
    with pytest.raises(PAError, match="x must match y"):
        axpby(dy, x32.values.parts[0], 1)
    with pytest.raises(PAError, match="x must match y"):
        axpby(dy, None, 1)
    with pytest.raises(PAError, match="copyto!: element types differ"):
        L.call("pa_vec_copy", dy.h, idx, x32.values.parts[0].h, idx, 1)
    with pytest.raises(PAError, match="copyto!: element types differ"):
        pamd.copyto_(y, z)
    _assert_parts(y, hy, "y after the rejected calls")
    _assert_parts(x, hx, "x after the rejected calls")
    # the accepted neighbours of the rejected modes still work
    axpby(dy, dx, 1 | L.PA_BCAST_F64)
    assert R.same_bits(dy.download(), R.bcast("axpy", hy[1], hx[1], 0.5))
    axpby(z.values.parts[0], z.values.parts[0], 1 | L.PA_BCAST_C128)
    assert R.same_bits(z.values.parts[0].download(), R.bcast("axpy", hz[1], hz[1], 0.5 + 0.25j))
    # dot over different owned counts
    parts = be.get_part_ids(1)
    r5, r6 = pamd.prange_linear(parts, 5), pamd.prange_linear(parts, 6)
    h5, h6 = {1: np.arange(5.0)}, {1: np.arange(6.0)}
    a, b = _up(pamd, h5, r5, np.float64), _up(pamd, h6, r6, np.float64)
    with pytest.raises(PAError, match="dot: owned counts differ"):
        pamd.dot(a, b)
    _assert_parts(a, h5, "a")
    _assert_parts(b, h6, "b")
    assert pamd.dot(a, a) == 30.0


# ---------------------------------------------------------------------------
# reductions: ranges whose owned lids interleave with ghost slots

def _mapped_range(be, pamd, counts, every=3):
    """counts[p] owned ids on part p+1 with a ghost slot in front and one
    after every `every` owned lids.  The ghost ids stand for a neighbour held
    by another process (a part id past the local ones), so the range has no
    exchanger; only the owned / ghost maps matter here."""
    parts = be.get_part_ids(len(counts))
    nown = int(sum(counts))
    first, gfirst, sets = 1, nown + 1, []
    for p, n in enumerate(counts, 1):
        nh = n // every + 1
        ghost = np.zeros(n + nh, bool)
        ghost[np.arange(nh) * (every + 1)] = True
        gid = np.empty(n + nh, np.int64)
        gid[~ghost] = np.arange(first, first + n)
        gid[ghost] = np.arange(gfirst, gfirst + nh)
        sets.append(pamd.IndexSet(p, gid, np.where(ghost, len(counts) + 1, p)))
        assert sets[-1].num_oids == n and sets[-1].num_hids == nh
        first, gfirst = first + n, gfirst + nh
    part = pamd.PData(parts.backend, parts.part_ids, sets, parts.shape)
    return pamd.prange_from_partition(gfirst - 1, part, ghost=False)


def _nan(dtype):
    return complex(np.nan, np.nan) if np.dtype(dtype).kind == "c" else np.nan


def _with_nan_ghosts(rows, owned, dtype):
    """per part: the owned values in their lids, NaN in every ghost slot"""
    host = {}
    for s, v in zip(rows.partition.parts, owned):
        h = np.full(s.num_lids, _nan(dtype), dtype)
        h[s.oid_to_lid - 1] = v
        host[s.part] = h
    return host


def _exact_values(rng, counts, cplx=True):
    """the exact family as complex128: re and im are k * 2**-10, |k| <= 1024"""
    out = []
    for n in counts:
        k = rng.integers(-1024, 1025, (2, n))
        out.append((k[0] + (1j * k[1] if cplx else 0)) / 1024.0)
    return out


def _as(values, dtype):
    """the family's values in dtype (real types take the real parts): exact"""
    if np.dtype(dtype).kind == "c":
        return [v.astype(dtype) for v in values]
    return [v.real.astype(dtype) for v in values]


_EXACT = {}


def _exact_case(be, pamd, counts, seed):
    """(rows, a, b, the parts' exact dot(a,b), dot(b,a), |a|^2 and sum(a), for
    complex and for real types) of one set of owned counts, computed once"""
    key = tuple(counts)
    if key not in _EXACT:
        rng = np.random.default_rng(seed)
        a, b = _exact_values(rng, counts), _exact_values(rng, counts)
        ref = {}
        for cplx in (True, False):
            pa, pb = (a, b) if cplx else ([v.real for v in a], [v.real for v in b])
            ref[cplx] = {"dot": R.exact_dot_parts(pa, pb), "tod": R.exact_dot_parts(pb, pa),
                         "sq": R.exact_dot_parts(pa, pa), "sum": R.exact_sum_parts(pa)}
        _EXACT[key] = (_mapped_range(be, pamd, counts), a, b, ref)
    return _EXACT[key]


def _check_exact(pamd, rows, a, b, ref, dtype):
    cplx = np.dtype(dtype).kind == "c"
    r = ref[cplx]
    va = _up(pamd, _with_nan_ghosts(rows, _as(a, dtype), dtype), rows, dtype)
    vb = _up(pamd, _with_nan_ghosts(rows, _as(b, dtype), dtype), rows, dtype)
    d, t = pamd.dot(va, vb), pamd.dot(vb, va)
    assert d == R.finish(r["dot"], dtype), "dot(a, b)"
    assert t == R.finish(r["tod"], dtype), "dot(b, a)"
    if cplx:
        assert d == t.conjugate() and d.imag != 0
    else:
        assert d == t
    assert pamd.norm(va) == R.finish_norm(r["sq"], dtype), "norm(a)"
    assert pamd.psum(va) == R.finish(r["sum"], dtype), "psum(a)"
    return va, vb


SMALL_COUNTS = [1, 63, 0, 64, 65, 255, 256, 257]  # around one wave and one block; an empty part in between


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_exact_reductions_small_parts(be, pamd, dtype):
    rows, a, b, ref = _exact_case(be, pamd, SMALL_COUNTS, SEED + 10)
    _check_exact(pamd, rows, a, b, ref, dtype)


LARGE = [1024 * 256 - 1, 1024 * 256, 1024 * 256 + 1, 2 * 1024 * 256 + 3]


@pytest.mark.parametrize("n", LARGE)
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_exact_reductions_one_part(be, pamd, dtype, n):
    """around the 1024-block cap of the reduction grid: every block full but
    one lane, every block full, one lane's grid-stride second step, and two
    full passes with a tail; the last block folds 1024 partials"""
    rows, a, b, ref = _exact_case(be, pamd, [n], SEED + 11)
    _check_exact(pamd, rows, a, b, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_exact_dot_over_two_maps(be, pamd, layouts, dtype):
    """dot(a, b) with a and b on ranges of equal owned ids and different lid
    layouts: each operand is read through its own map"""
    rng = np.random.default_rng(SEED + 12)
    counts = [s.num_oids for s in layouts["g1"].partition.parts]
    a, b = _exact_values(rng, counts), _exact_values(rng, counts)
    pa, pb = _as(a, dtype), _as(b, dtype)
    want, tnaw = R.exact_dot(pa, pb, dtype), R.exact_dot(pb, pa, dtype)
    for na, nb in (("g1", "c"), ("c", "g1"), ("plain", "g1"), ("g1", "plain"), ("c", "plain")):
        ra, rb = layouts[na], layouts[nb]
        va = _up(pamd, _with_nan_ghosts(ra, pa, dtype), ra, dtype)
        vb = _up(pamd, _with_nan_ghosts(rb, pb, dtype), rb, dtype)
        assert pamd.dot(va, vb) == want, f"dot over {na}, {nb}"
        assert pamd.dot(vb, va) == tnaw, f"dot over {nb}, {na}"
        if np.dtype(dtype).kind == "c":
            assert want == tnaw.conjugate() and want.imag != 0


def test_scratch_reuse(be, pamd):
    """the per-context partials and result slot after a larger call: the
    largest dot, a 65-value dot, a ComplexF64 psum and a Float64 norm on one
    context, each against its reference; then the first call again, to the bit"""
    rows, a, b, ref = _exact_case(be, pamd, [LARGE[-1]], SEED + 11)
    T = np.complex128
    va = _up(pamd, _with_nan_ghosts(rows, _as(a, T), T), rows, T)
    vb = _up(pamd, _with_nan_ghosts(rows, _as(b, T), T), rows, T)
    first = pamd.dot(va, vb)
    assert first == R.finish(ref[True]["dot"], T) and first.imag != 0
    r65, a65, b65, ref65 = _exact_case(be, pamd, [65], SEED + 13)
    for dt in (np.float32, np.complex128):
        u = _up(pamd, _with_nan_ghosts(r65, _as(a65, dt), dt), r65, dt)
        w = _up(pamd, _with_nan_ghosts(r65, _as(b65, dt), dt), r65, dt)
        assert pamd.dot(u, w) == R.finish(ref65[np.dtype(dt).kind == "c"]["dot"], dt), np.dtype(dt).name
    assert pamd.psum(w) == R.finish(R.exact_sum_parts(_as(b65, T)), T)
    rs, as_, bs, refs = _exact_case(be, pamd, [LARGE[0]], SEED + 11)  # 1024 blocks again, 8-byte partials
    v64 = _up(pamd, _with_nan_ghosts(rs, _as(as_, np.float64), np.float64), rs, np.float64)
    assert pamd.norm(v64) == R.finish_norm(refs[False]["sq"], np.float64)
    assert all(v.values.parts[0].ctx is va.values.parts[0].ctx for v in (u, w, v64))  # one context's scratch
    again = pamd.dot(va, vb)
    assert (again.real.hex(), again.imag.hex()) == (first.real.hex(), first.imag.hex())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_nan_and_inf_in_the_last_owned_value(be, pamd, dtype):
    rows, a, b, ref = _exact_case(be, pamd, SMALL_COUNTS, SEED + 10)
    pa, pb = _as(a, dtype), _as(b, dtype)
    vb = _up(pamd, _with_nan_ghosts(rows, pb, dtype), rows, dtype)

    def last(v):
        q = [x.copy() for x in pa]
        q[-1][-1] = v
        return _up(pamd, _with_nan_ghosts(rows, q, dtype), rows, dtype)
    nan = lambda z: math.isnan(complex(z).real) or math.isnan(complex(z).imag)
    vn = last(np.nan)
    assert nan(pamd.dot(vn, vb)) and nan(pamd.dot(vb, vn)) and math.isnan(pamd.norm(vn)) and nan(pamd.psum(vn))
    vi = last(np.inf)
    assert complex(pamd.psum(vi)).real == math.inf and pamd.norm(vi) == math.inf
    # the unchanged vectors still reduce to their references
    va = _up(pamd, _with_nan_ghosts(rows, pa, dtype), rows, dtype)
    assert pamd.psum(va) == R.finish(ref[np.dtype(dtype).kind == "c"]["sum"], dtype)


# ---------------------------------------------------------------------------
# reductions, random family: uniform values with full mantissas against the
# exact rational result

N_RANDOM = 70001
_RANDOM = {}


def _random_case(dtype):
    """(a, b, {n: exact (re, im, S) of dot, sum and the sum of squares}) for
    n = 70 000 (the four-part layout: a prefix) and 70 001, computed once"""
    key = np.dtype(dtype)
    if key not in _RANDOM:
        rng = np.random.default_rng(SEED + 20 + key.num)
        a, b = _rand(rng, N_RANDOM, dtype), _rand(rng, N_RANDOM, dtype)
        m = N_RANDOM - 1
        add = lambda u, v: tuple(p + q for p, q in zip(u, v))
        ref = {m: {"dot": R.fraction_dot(a[:m], b[:m]), "sq": R.fraction_dot(a[:m], a[:m]),
                   "sum": R.fraction_sum(a[:m])}}
        ref[N_RANDOM] = {"dot": add(ref[m]["dot"], R.fraction_dot(a[m:], b[m:])),
                         "sq": add(ref[m]["sq"], R.fraction_dot(a[m:], a[m:])),
                         "sum": add(ref[m]["sum"], R.fraction_sum(a[m:]))}
        _RANDOM[key] = (a, b, ref)
    return _RANDOM[key]


@pytest.mark.parametrize("counts", [[N_RANDOM], [17500] * 4], ids=["1x70001", "4x17500"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids(DTYPES))
def test_random_reductions(be, pamd, dtype, counts):
    """|got - exact| <= (n 2**-53 + (4 + P) eps_T) sum|t_i| (blas1_ref.
    sum_bound: it holds for every summation order); norm: the same relative
    bound against sqrt(exact), plus 2**-52"""
    a, b, ref = _random_case(dtype)
    n, P = sum(counts), len(counts)
    ref = ref[n]
    cut = np.cumsum([0] + counts)
    rows = _mapped_range(be, pamd, counts, every=5)
    split = lambda v: [v[cut[i]:cut[i + 1]] for i in range(P)]
    va = _up(pamd, _with_nan_ghosts(rows, split(a), dtype), rows, dtype)
    vb = _up(pamd, _with_nan_ghosts(rows, split(b), dtype), rows, dtype)
    bound = R.sum_bound(n, P, dtype)
    assert bound < Fraction(1, 1 << 19)
    got = {"dot": pamd.dot(va, vb), "sum": pamd.psum(va), "norm": pamd.norm(va)}
    for k in ("dot", "sum"):
        re, im, S = ref[k]
        err = abs(complex(got[k]) - complex(float(re), float(im)))
        print(f"{np.dtype(dtype).name} {P} part(s) {k}: |got - exact| = {err:.3e}, bound {float(bound * S):.3e}")
        assert R.within(got[k], re, im, S, bound), k
    sq = ref["sq"][0]
    print(f"{np.dtype(dtype).name} {P} part(s) norm: |got - exact| = {abs(got['norm'] - math.sqrt(float(sq))):.3e}, "
          f"bound {float(bound + Fraction(1, 1 << 52)) * math.sqrt(float(sq)):.3e}")
    assert ref["sq"][1] == 0 and R.norm_within(got["norm"], sq, bound)
