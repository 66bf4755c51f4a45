"""Jacobi-preconditioned CG on the device: diag(A) off the SELL layout
(pa_mat_diag), Pl \\ r fused with ρ (pa_pcg_apply_all), the fused tail and
head of an iteration (pa_pcg_update_all) and cg_(…, Pl=Jacobi(A)) end to end,
against tests/pcg_ref.py (pinned on the CPU by test_pcg_ref_host.py)."""
import numpy as np
import pytest

import blas1_ref
import pcg_ref
from matrix_cases import SEED, _knobs, long_row_coo, tridiag, unsorted_csr, with_ghost_coo
from pcg_ref import ERR_TOL, HISTORY_RTOL

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 65, 257, 1031)  # owned lids per part: below a wave, across a wave, across a block, an odd tail
RED_TOL = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}  # test_gpu_drivers.py::test_fused_cg_kernels


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


# ---------------------------------------------------------------------------
# 1. diag

def _pdata(pamd, parts, d):
    return pamd.PData(parts.backend, parts.part_ids, [d[p] for p in parts.part_ids], parts.shape)


def _check_diag(pamd, A, host):
    """diag(A) bit-equal to diag_ref of the host matrices (host[p]: part p's
    CSC / CSR in lids), ghosts equal to their owners' values; no entry table"""
    before = [M.entry_table() for M in A.values.parts]
    d = pamd.diag(A).to_host()
    assert [M.entry_table() for M in A.values.parts] == before == [(0, 0)] * len(before)
    ref = {p: pcg_ref.diag_ref(host[p], A.rows.partition.local(p), A.cols.partition.local(p), A.dtype)
           for p in A.values.part_ids}
    by_gid = {}
    for p in A.values.part_ids:
        s = A.cols.partition.local(p)
        o = np.asarray(s.oid_to_lid) - 1
        by_gid.update(zip(np.asarray(s.lid_to_gid)[o].tolist(), ref[p][o]))
    hits = 0
    for p in A.values.part_ids:
        s = A.cols.partition.local(p)
        h = np.asarray(s.hid_to_lid, np.int64) - 1
        ref[p][h] = [by_gid[g] for g in np.asarray(s.lid_to_gid)[h].tolist()]
        assert blas1_ref.same_bits(d.local(p), ref[p]), f"part {p}: diag differs"
        hits += int(np.count_nonzero(ref[p][np.asarray(s.oid_to_lid) - 1]))
    return hits, ref


@pytest.mark.parametrize("fmt", [1, 0])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_diag_stencil(be, pamd, O, dtype, fmt):
    """27-point operator on (2,2,1) parts: pattern slices and, for Float32,
    the delta16 interleave of 4 rows per lane"""
    shape, N = (2, 2, 1), (12, 10, 9)
    with _knobs(pamd, spmv_format=fmt):
        A = pamd.drivers.stencil_operator(be.get_part_ids(shape), N, 27, dtype)
        OA = O.stencil_problem(O.get_part_ids(shape), N, 27, dtype)
        hits, _ = _check_diag(pamd, A, {p: OA.values[p] for p in A.values.part_ids})
    assert hits == len(A.rows)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_diag_irregular(be, pamd, O, dtype):
    """Voronoi parts: side rows and the triple SELL"""
    N, nparts = (24, 22, 20), 8
    with _knobs(pamd, pattern_min_regular=40):
        A = pamd.drivers.irregular_problem(be.get_part_ids(nparts), N, 27, dtype)
    info = A.info().parts
    side, tri = sum(i["side_rows"] for i in info), sum(i["triple_sell_slices"] for i in info)
    print(f"side rows {side}, triple SELL slices {tri}")
    assert side + tri > 0
    OA = O.irregular_problem(O.get_part_ids(nparts), N, 27, dtype)
    hits, _ = _check_diag(pamd, A, {p: OA.values[p] for p in A.values.part_ids})
    assert hits == len(A.rows)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_diag_long_rows(be, pamd, dtype):
    """rows far longer than the rest live in the long CSR, their diagonal too"""
    parts = be.get_part_ids((2, 2, 1))
    _, part = pamd.drivers.stencil_partition(parts, (20, 18, 16), 27)
    rng = np.random.default_rng(SEED + 31)
    coo, longs = {}, {}
    for p in parts.part_ids:
        I, J, V, longs[p] = long_row_coo(rng, part, p, dtype, [600, 1000, 4000, 70])
        own = part.partition.local(p).oid_to_lid.astype(I.dtype)
        keep = own[(own % 5 != 0) | np.isin(own, longs[p])]  # a diagonal entry for sure: the long rows, 4 rows in 5
        coo[p] = (np.concatenate([I, keep]), np.concatenate([J, keep]),
                  np.concatenate([V, rng.uniform(1, 2, len(keep)).astype(dtype)]))
    mk = lambda k: _pdata(pamd, parts, {p: coo[p][k] for p in parts.part_ids})
    A = pamd.PSparseMatrix.from_coo(mk(0), mk(1), mk(2), part, part, ids="local")
    host = {}
    for p in parts.part_ids:
        assert A.values.local(p).info()["long_rows"] == 3
        n = part.partition.local(p).num_lids
        host[p] = pamd.compresscoo(*coo[p], n, n)
    _, ref = _check_diag(pamd, A, host)
    for p in parts.part_ids:  # the long rows' own diagonals are among what was compared
        assert all(ref[p][l - 1] != 0 for l in longs[p]), (p, longs[p])


@pytest.mark.parametrize("nparts", [4, (2, 2)])
def test_diag_fem_sa(be, pamd, O, nparts):
    """stored ghost rows must not leak in"""
    A, _, _, _ = pamd.drivers.fem_sa_problem(be.get_part_ids(nparts), 10)
    OA, _, _, _ = O.fem_sa_problem(O.get_part_ids(nparts), 10)
    assert any(len(s.hid_to_lid) for s in A.rows.partition.parts)
    hits, _ = _check_diag(pamd, A, {p: OA.values[p] for p in A.values.part_ids})
    assert hits == len(A.rows)


def _lids(s, gids):
    g2l = {g: l + 1 for l, g in enumerate(np.asarray(s.lid_to_gid).tolist())}
    return np.array([g2l[g] for g in np.asarray(gids).tolist()], np.int64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_diag_interleaved_lids(be, pamd, dtype):
    """PRange with ghosts and periodic dimensions: owned and ghost lids
    interleave, so the row's own column goes through oid_to_lid"""
    shape, ngids, periodic = (2, 2, 1), (16, 14, 6), (True, False, True)
    parts = be.get_part_ids(shape)
    rows = pamd.prange_cartesian(parts, ngids, with_ghost=True, isperiodic=periodic)
    assert any(s.oid_to_lid[-1] != s.num_oids for s in rows.partition.parts)
    I, J, V = with_ghost_coo(rows, parts, ngids, periodic, np.random.default_rng(SEED + 32))
    V = {p: V[p].astype(dtype) for p in V}
    host = {}
    for p in parts.part_ids:
        s = rows.partition.local(p)
        host[p] = pamd.compresscoo(_lids(s, I[p]), _lids(s, J[p]), V[p], s.num_lids, s.num_lids)
    cp = lambda d: _pdata(pamd, parts, {p: d[p].copy() for p in parts.part_ids})
    A = pamd.PSparseMatrix.from_coo(cp(I), cp(J), cp(V), rows, rows, ids="global")
    hits, _ = _check_diag(pamd, A, host)
    assert hits == int(np.prod(ngids))


@pytest.mark.parametrize("order", ["diag_first", "descending"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_diag_unsorted_csr_parent(be, pamd, dtype, order):
    n, Bi = 390, 0
    rowptr, colval, V, _, _, _ = unsorted_csr(n, (-7, -1, 0, 1, 2, 9), Bi, order, dtype)
    parts = be.get_part_ids(1)
    rows = pamd.prange_linear(parts, n)
    M = pamd.CSR(Bi, n, n, rowptr, colval, V)
    A = pamd.PSparseMatrix.from_csr(_pdata(pamd, parts, {1: M}), rows, rows)
    hits, _ = _check_diag(pamd, A, {1: M})
    assert hits == n


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_diag_absent_entries_stay_zero(be, pamd, dtype):
    """a tridiagonal matrix whose every third diagonal entry is not in the pattern"""
    n, nparts = 700, 3
    parts = be.get_part_ids(nparts)
    rows = pamd.prange_linear(parts, n)
    coo = {}
    for p in parts.part_ids:
        s = rows.partition.local(p)
        I, J, V = tridiag(n, s.lid_to_gid[s.oid_to_lid - 1])
        keep = ~((I == J) & (I % 3 == 0))
        coo[p] = (I[keep], J[keep], V[keep].astype(dtype))
    mk = lambda k: _pdata(pamd, parts, {p: coo[p][k].copy() for p in parts.part_ids})
    cols = pamd.add_gids(rows, mk(1))
    host = {}
    for p in parts.part_ids:
        r, c = rows.partition.local(p), cols.partition.local(p)
        host[p] = pamd.compresscoo(_lids(r, coo[p][0]), _lids(c, coo[p][1]), coo[p][2], r.num_lids, c.num_lids)
    A = pamd.PSparseMatrix.from_coo(mk(0), mk(1), mk(2), rows, cols, ids="global")
    hits, ref = _check_diag(pamd, A, host)
    assert hits == n - n // 3
    d = pamd.diag(A).to_host()
    for p in parts.part_ids:
        c = cols.partition.local(p)
        absent = np.asarray(c.lid_to_gid) % 3 == 0
        assert np.all(d.local(p)[absent] == 0) and not np.any(np.signbit(d.local(p)[absent]))


# ---------------------------------------------------------------------------
# 2., 3. the fused kernels

def _layout(pamd, be, name):
    """sizes: five parts owning SIZES lids, no ghosts; ghosts: the columns of
    a 27-point operator on (2,2,1) parts (contiguous owned lids, then ghosts);
    interleaved: owned and ghost lids mixed (the reductions run on their own)"""
    if name == "sizes":
        parts = be.get_part_ids(len(SIZES))
        return parts, pamd.prange_noids(parts, _pdata(pamd, parts, dict(zip(parts.part_ids, SIZES))))
    if name == "ghosts":
        parts = be.get_part_ids((2, 2, 1))
        return parts, pamd.drivers.stencil_partition(parts, (12, 10, 9), 27)[1]
    parts = be.get_part_ids((2, 2, 1))
    return parts, pamd.prange_cartesian(parts, (16, 14, 6), with_ghost=True, isperiodic=(True, False, True))


def _vectors(pamd, parts, rng_seed, rows, dtype, names):
    rng = np.random.default_rng(rng_seed)
    vals = {k: {p: rng.uniform(-1, 1, rows.partition.local(p).num_lids).astype(dtype) for p in parts.part_ids}
            for k in names}
    if "d" in vals:
        vals["d"] = {p: rng.uniform(0.5, 2.0, rows.partition.local(p).num_lids).astype(dtype) for p in parts.part_ids}
    mk = lambda k: pamd.PVector.from_host(pamd.map_parts(lambda s: vals[k][s.part], rows.partition), rows)
    return vals, mk


def _ref_dot(rows, a, b, dtype):
    """Σ over the owned lids of a_i*b_i (the product in T), Float64 per part,
    rounded to T, the parts added in T in part order"""
    T = np.dtype(dtype).type
    tot = T(0)
    for s in rows.partition.parts:
        o = np.asarray(s.oid_to_lid) - 1
        tot = T(tot + T(np.sum((a[s.part][o] * b[s.part][o]).astype(np.float64))))
    return float(tot)


@pytest.mark.parametrize("layout", ["sizes", "ghosts", "interleaved"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ldiv_jacobi(be, pamd, dtype, layout):
    """ldiv_(c, Jacobi(d), r) / pa_pcg_apply_all: c bit-equal to numpy's r / d
    in T over all lids, ρ within the fused-reduction tolerance of the
    reference dot; a zero in d gives ±Inf / NaN at that lid and nowhere else.
    A DeviceVector owns its allocation (pa_vec_create aligns it; the ABI has
    no offset views of a vector), so the 16 B path cannot be refused from
    here and the one-element instantiations (V = 1: every element through the
    pack loop, no tail) are not run by any test; the odd sizes run the 16 B
    instantiations' scalar tail."""
    parts, rows = _layout(pamd, be, layout)
    vals, mk = _vectors(pamd, parts, [SEED, 41], rows, dtype, "rd")
    r, d, c = mk("r"), mk("d"), pamd.PVector.undef(rows, dtype)
    rho = pamd.pcg_apply_(c, r, d)
    assert isinstance(rho, np.dtype(dtype).type)
    want = {p: vals["r"][p] / vals["d"][p] for p in parts.part_ids}
    for p in parts.part_ids:
        assert blas1_ref.same_bits(c.to_host().local(p), want[p]), p
    ref = _ref_dot(rows, want, vals["r"], dtype)
    print(f"rho {float(rho)!r} reference {ref!r}")
    assert abs(float(rho) - ref) <= RED_TOL[np.dtype(dtype)] * abs(ref)
    c2 = pamd.PVector.undef(rows, dtype)
    assert pamd.ldiv_(c2, pamd.Jacobi(d), r) is c2
    for p in parts.part_ids:
        assert blas1_ref.same_bits(c2.to_host().local(p), want[p]), p
    # zeros in d: r / 0 = ±Inf, 0 / 0 = NaN, at those lids only
    p0 = parts.part_ids[2]
    s = rows.partition.local(p0)
    z = [int(s.oid_to_lid[0]) - 1, int(s.oid_to_lid[-1]) - 1, s.num_lids // 2]
    vals["d"][p0][z] = 0
    vals["r"][p0][z[1]] = 0
    with np.errstate(all="ignore"):
        want0 = vals["r"][p0] / vals["d"][p0]
    assert np.isnan(want0[z[1]]) and np.isinf(want0[z[0]])
    pamd.ldiv_(c2, pamd.Jacobi(mk("d")), mk("r"))
    got = c2.to_host()
    assert blas1_ref.same_bits(got.local(p0), want0)
    assert sum(int(np.count_nonzero(~np.isfinite(got.local(p)))) for p in parts.part_ids) == len(set(z))


def test_ldiv_jacobi_diagonal_on_another_prange(be, pamd):
    """Jacobi(d) with d on another PRange object that owns the same ids: the
    owned values are copied over and the ghosts exchanged from their owners,
    so c's owned values are r / d and its ghosts r / (the owner's d)"""
    parts, rows = _layout(pamd, be, "ghosts")
    _, rows2 = _layout(pamd, be, "ghosts")
    assert rows2 is not rows
    vals, mk = _vectors(pamd, parts, [SEED, 43], rows, np.float64, "rd")
    d2 = pamd.PVector.from_host(pamd.map_parts(lambda s: vals["d"][s.part], rows2.partition), rows2)
    c = pamd.PVector.undef(rows, np.float64)
    pamd.ldiv_(c, pamd.Jacobi(d2), mk("r"))
    by_gid = {}
    for s in rows.partition.parts:
        o = np.asarray(s.oid_to_lid) - 1
        by_gid.update(zip(np.asarray(s.lid_to_gid)[o].tolist(), vals["d"][s.part][o]))
    for s in rows.partition.parts:
        d = np.array([by_gid[g] for g in np.asarray(s.lid_to_gid).tolist()])
        assert blas1_ref.same_bits(c.to_host().local(s.part), vals["r"][s.part] / d), s.part


@pytest.mark.parametrize("layout", ["sizes", "ghosts", "interleaved"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_pcg_update_kernel(be, pamd, dtype, layout):
    """pa_pcg_update_all with a T-typed α (contiguous owned lids; interleaved
    ones are an error with a message): x, r, c bit-equal to the unfused
    composition on the device and to the independent reference
    (blas1_ref.bcast with a T scalar, then numpy's division); norm(r) and
    dot(c, r) within the fused-reduction tolerance."""
    T = np.dtype(dtype).type
    parts, rows = _layout(pamd, be, layout)
    vals, mk = _vectors(pamd, parts, [SEED, 42], rows, dtype, "xrucd")
    alpha = T(0.37)
    x, r, u, c, d = (mk(k) for k in "xrucd")
    if layout == "interleaved":  # the reductions ride over lids 0..noids-1: refused, nothing written
        with pytest.raises(pamd.PAError, match="contiguous"):
            pamd.pcg_update_(x, r, u, c, d, alpha)
        for k, v in zip("xrc", (x, r, c)):
            for p in parts.part_ids:
                assert np.array_equal(v.to_host().local(p), vals[k][p])
        return
    nr, rho = pamd.pcg_update_(x, r, u, c, d, alpha)
    assert isinstance(nr, float) and isinstance(rho, T)
    x2, r2, c2 = mk("x"), mk("r"), mk("c")
    pamd.axpy_(x2, alpha, u)
    pamd.axmy_(r2, alpha, c2)
    pamd.assign_(c2, r2 / d)
    nr2, rho2 = pamd.norm(r2), pamd.dot(c2, r2)
    tol = RED_TOL[np.dtype(dtype)]
    print(f"norm {nr!r} / {nr2!r}, rho {float(rho)!r} / {rho2!r}")
    assert abs(nr - nr2) <= tol * nr2 and abs(float(rho) - rho2) <= tol * abs(rho2)
    want_r, want_c = {}, {}
    for p in parts.part_ids:
        want_x = blas1_ref.bcast("axpy", vals["x"][p], vals["u"][p], alpha)
        want_r[p] = blas1_ref.bcast("axmy", vals["r"][p], vals["c"][p], alpha)
        want_c[p] = want_r[p] / vals["d"][p]
        for got, got2, want in ((x, x2, want_x), (r, r2, want_r[p]), (c, c2, want_c[p])):
            assert np.array_equal(got.to_host().local(p), got2.to_host().local(p)), p
            assert blas1_ref.same_bits(got.to_host().local(p), want), p
        assert np.array_equal(u.to_host().local(p), vals["u"][p]) and np.array_equal(d.to_host().local(p), vals["d"][p])
    ref_n = _ref_dot(rows, want_r, want_r, dtype) ** 0.5
    ref_rho = _ref_dot(rows, want_c, want_r, dtype)
    assert abs(nr - ref_n) <= tol * ref_n and abs(float(rho) - ref_rho) <= tol * abs(ref_rho)


# ---------------------------------------------------------------------------
# 4. end to end

def _oracle_copy(O, v, dtype=None):
    return O.PVector(O.map_parts(lambda a: np.asarray(a, dtype or a.dtype).copy(), v.values), v.rows)


def _device_runs(pamd, A, b, x0, **kw):
    P = pamd.Jacobi(A)
    out = {}
    for fused in (True, False):
        x, hist = x0.copy(), []
        assert pamd.cg_(x, A, b, history=hist, fused=fused, Pl=P, **kw) is x
        out[fused] = (x, hist)
    return out


def _error(x, xh):
    return pcg_ref.owned_error(x.rows.partition.parts, x.to_host(), xh.to_host())


@pytest.mark.parametrize("problem,nparts", [("fdm_problem", (2, 2, 2)), ("fem_sa_problem", 4),
                                            ("fem_sa_problem", (2, 2))])
def test_pcg_end_to_end(be, pamd, O, problem, nparts):
    """cg_(…, Pl=Jacobi(A)) fused and unfused: the same iteration count, and
    histories that agree with each other and with pcg_ref to rtol 1e-8 — the
    figure of the existing CG tests; pcg_ref's own history moves by 5.4e-15
    (fdm) / 1.4e-14 (fem_sa) between pairwise and sequential dots
    (test_pcg_ref_host.py), below the 1e-9 at which the tolerance would have
    to widen.  The solution meets the reference's 1e-5."""
    A, b, x0, xh = getattr(pamd.drivers, problem)(be.get_part_ids(nparts), 10)
    OA, ob, ox0, _ = getattr(O, problem)(O.get_part_ids(nparts), 10)
    ox, ohist = _oracle_copy(O, ox0), []
    pcg_ref.pcg_ref(O, ox, OA, ob, pcg_ref.diag_pvector(O, OA), log=ohist)
    runs = _device_runs(pamd, A, b, x0)
    (xf, hf), (xu, hu) = runs[True], runs[False]
    print(f"{problem} {nparts}: {len(hf)} / {len(hu)} / {len(ohist)} iterations")
    assert len(hf) == len(hu) == len(ohist) > 0
    np.testing.assert_allclose(hf, hu, rtol=HISTORY_RTOL)
    np.testing.assert_allclose(hf, ohist, rtol=HISTORY_RTOL)
    np.testing.assert_allclose(hu, ohist, rtol=HISTORY_RTOL)
    assert _error(xf, xh) < ERR_TOL and _error(xu, xh) < ERR_TOL


def test_pcg_scaled_system(be, pamd, O):
    """S·A·S of test_pcg_ref_host.py (s from 1 to 10): PCG on the device stops
    in the reference's iteration count, cg_ without Pl needs more, and the
    solution meets 1e-5.  Histories to rtol 1e-8 (pcg_ref's spread on this
    system between pairwise and sequential dots: 5.9e-10 < 1e-9)."""
    shape = (2, 2, 2)
    A, b, x0, xh = pcg_ref.scaled_device_fdm(pamd, be.get_part_ids(shape), 10)
    OA, ob, ox0, _ = pcg_ref.scaled_oracle_fdm(O, O.get_part_ids(shape), 10)
    ox, ohist = _oracle_copy(O, ox0), []
    pcg_ref.pcg_ref(O, ox, OA, ob, pcg_ref.diag_pvector(O, OA), log=ohist)
    runs = _device_runs(pamd, A, b, x0)
    for fused, (x, hist) in runs.items():
        assert len(hist) == len(ohist), fused
        np.testing.assert_allclose(hist, ohist, rtol=HISTORY_RTOL)
        assert _error(x, xh) < ERR_TOL
    xc, hc = x0.copy(), []
    pamd.cg_(xc, A, b, history=hc)
    print(f"scaled fdm: PCG {len(ohist)} iterations, CG {len(hc)}")
    assert len(hc) > len(ohist)


def test_pcg_float32(be, pamd, O):
    """test_fdm.jl in Float32 with Pl, compared as
    test_gpu_drivers.py::test_fdm_cg_float32_julia_scalars compares the plain
    loop: against the reference's Float32 run the same iteration count, the
    first three residuals bit for bit — the check that pins the scalar type:
    with Float64 ρ, β, α the history differs from the first iterations on
    (by up to 9.0e-07, inside the bound below: test_pcg_ref_host.py) — and the whole history within
    5e-6 relative (the local dot / norm summation order is unpinned in the
    reference).  The reference runs with pcg_ref.t_dot, whose products are
    Float32 as Julia's dot forms them and as the device does; the oracle's own
    dot multiplies in Float64, which moves the history by 1.256e-06.  Likewise
    pcg_ref.t_norm squares in Float32, as the library documents its norm; with
    the oracle's Float64 squares the iterates are the same but the third
    residual is one Float32 rounding of Σr² away (3.8e-08, measured on the
    MI355X and reproduced on the CPU by test_pcg_ref_host.py)."""
    shape = (2, 2, 2)
    A, b, x0, _ = pamd.drivers.fdm_problem(be.get_part_ids(shape), 10, np.float32)
    OA, ob, ox0, _ = O.fdm_problem(O.get_part_ids(shape), 10)
    vals = O.map_parts(lambda M: O.CSC(M.m, M.n, M.colptr, M.rowval, O._convert_values(M.nzval, np.float32)),
                       OA.values)
    OA32 = O.PSparseMatrix(vals, OA.rows, OA.cols)
    ox, ohist = _oracle_copy(O, ox0, np.float32), []
    pcg_ref.pcg_ref(O, ox, OA32, _oracle_copy(O, ob, np.float32), pcg_ref.diag_pvector(O, OA32), log=ohist,
                    dot=pcg_ref.t_dot(O), norm=pcg_ref.t_norm(O))
    for fused, (x, hist) in _device_runs(pamd, A, b, x0).items():
        assert len(hist) == len(ohist) and len(hist) > 5, (fused, len(hist), len(ohist))
        rel = max(abs(a - b) / abs(b) for a, b in zip(hist, ohist))
        same = sum(a == b for a, b in zip(hist, ohist))
        print(f"Float32 PCG fused={fused}: {len(hist)} iterations, max relative history difference {rel:.3e}, "
              f"{same} residuals bit-equal")
        assert hist[:3] == ohist[:3], fused
        assert rel <= 5e-6


# ---------------------------------------------------------------------------
# 5. guards

def test_guards_and_the_default_path(be, pamd):
    parts = be.get_part_ids((2, 2, 2))
    A, b, x0, _ = pamd.drivers.fdm_problem(parts, 10)
    P = pamd.Jacobi(A)
    with pytest.raises(NotImplementedError):
        pamd.cg_(x0.copy(), A, b, Pl=P, device=True)
    Ac, bc, xc, _ = pamd.drivers.fdm_problem(parts, 10, np.complex128)
    with pytest.raises(NotImplementedError):
        pamd.diag(Ac)
    with pytest.raises(NotImplementedError):
        pamd.cg_(xc.copy(), Ac, bc, Pl=P)
    with pytest.raises(NotImplementedError):
        pamd.Jacobi(xc)
    # the three entries refuse complex handles themselves
    dv, iv = xc.values.parts[0], pamd.pvector._idx(xc)[0]
    L, P1 = pamd._lib, lambda h: pamd._lib.ptr_array([h])
    out = np.zeros(2)
    op = out.ctypes.data
    with pytest.raises(pamd.PAError, match="complex"):
        L.call("pa_pcg_apply_all", 1, P1(dv.h), P1(dv.h), P1(dv.h), P1(iv), op)
    with pytest.raises(pamd.PAError, match="complex"):
        import ctypes
        L.call("pa_pcg_update_all", 1, P1(dv.h), P1(dv.h), P1(dv.h), P1(dv.h), P1(dv.h), P1(iv), op,
               ctypes.byref(ctypes.c_double()), op)
    # Pl=None is the call without the keyword, bit for bit
    h1, h2 = [], []
    x1, x2 = x0.copy(), x0.copy()
    pamd.cg_(x1, A, b, history=h1)
    pamd.cg_(x2, A, b, history=h2, Pl=None)
    assert h1 == h2 and len(h1) > 0
    for p in parts.part_ids:
        assert np.array_equal(x1.to_host().local(p), x2.to_host().local(p))
