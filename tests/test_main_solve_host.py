"""The gather-to-MAIN block on the host (no GPU): the sequential restatement
of tests/main_solve_ref.py on the reference's own known-answer matrix
(test_interfaces.jl:686-733, tests/golden/interfaces_kats.json), and the
host factorisation `_main_lu` behind pamd.solve / pamd.lu — its scipy and
dense paths on that matrix."""
import json
import os
import sys

import numpy as np
import pytest

import main_solve_ref as R

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "interfaces_kats.json")))


@pytest.fixture(scope="module")
def kat(O):
    """the 4-part 10 x 10 matrix, its dense form built as
    test_irregular_coo_kat builds it, and y = PVector(1.0, A.rows)"""
    k = GOLD["irregular_coo"]
    parts = O.get_part_ids(4)
    I = O.PData([list(v) for v in k["I"]])
    J = O.PData([list(v) for v in k["J"]])
    V = O.PData([np.array(v) for v in k["V"]])
    rows = O.prange_linear(parts, k["n"])
    O.add_gids_(rows, I)
    cols = O.prange_linear(parts, k["n"])
    O.add_gids_(cols, J)
    A = O.psparse_from_coo(I, J, V, rows, cols, ids="global")
    D = np.zeros((k["n"], k["n"]))
    for M, r, c in zip(A.values.parts, rows.partition.parts, cols.partition.parts):
        for j in range(M.n):
            for p in range(M.colptr[j] - 1, M.colptr[j + 1] - 1):
                i = M.rowval[p]
                if r.lid_to_part[i - 1] == r.part:
                    D[r.lid_to_gid[i - 1] - 1, c.lid_to_gid[j] - 1] += M.nzval[p]
    y = O.pvector_undef(rows)
    O.map_parts(lambda v: v.fill(1.0), y.values)
    return k, A, D, y


def _dense(m, n, colptr, rowval, nzval):
    a = np.zeros((m, n), dtype=nzval.dtype)
    a[rowval - 1, np.repeat(np.arange(n), np.diff(colptr))] = nzval
    return a


def _residual(O, A, x, y):
    """norm(A*x - y) over the owned rows"""
    ax = O.pvector_undef(A.rows)
    O.mul_(ax, A, x)
    r2 = 0.0
    for v, w, s in zip(ax.values.parts, y.values.parts, A.rows.partition.parts):
        own = np.asarray(s.oid_to_lid) - 1
        r2 += float(np.sum((v[own] - w[own]) ** 2))
    return np.sqrt(r2)


def test_to_main_ranges(O, kat):
    k, A, _, _ = kat
    m = R.to_main(A.cols)
    assert m.ngids == k["n"]
    for s, t in zip(A.cols.partition.parts, m.partition.parts):
        own = [s.lid_to_gid[l - 1] for l in s.oid_to_lid]
        assert t.lid_to_gid == (list(range(1, k["n"] + 1)) if s.part == R.MAIN else own)
        assert set(t.lid_to_part) <= {R.MAIN}
        assert t.num_oids == (k["n"] if s.part == R.MAIN else 0)


def test_gathered_matrix_is_the_dense_matrix(O, kat):
    k, A, D, _ = kat
    a_in_main = R.gather_matrix(A)
    M = a_in_main.values.parts[R.MAIN - 1]
    assert (M.m, M.n) == (k["n"], k["n"])
    assert np.array_equal(_dense(*R.canonical_csc(M)), D)
    for p, other in enumerate(a_in_main.values.parts[1:], start=2):
        assert len(other.nzval) == 0, p
        assert (other.m, other.n) == (A.rows.partition.parts[p - 1].num_oids, A.cols.partition.parts[p - 1].num_oids)


def test_gather_and_scatter_of_a_vector(O, kat):
    k, A, _, _ = kat
    b = O.pvector_undef(A.cols)
    for v, s in zip(b.values.parts, A.cols.partition.parts):
        v[:] = [100.0 + g for g in s.lid_to_gid]
    keep = [v.copy() for v in b.values.parts]
    bm = R.gather_vector(b)
    assert np.array_equal(bm.values.parts[0], 100.0 + np.arange(1, k["n"] + 1))
    assert all(not v.any() for v in bm.values.parts[1:])  # ghosts zeroed by assemble!
    c = O.pvector_undef(A.cols)
    for v in c.values.parts:
        v[:] = -7.0
    R.scatter(c, bm)
    for v, w, s in zip(c.values.parts, keep, A.cols.partition.parts):
        own = np.asarray(s.oid_to_lid) - 1
        gh = np.asarray(s.hid_to_lid, dtype=np.int64) - 1
        assert np.array_equal(v[own], w[own])
        assert (v[gh] == -7.0).all()  # scatter! leaves the ghosts


def test_restated_solve_meets_the_reference_tolerance(O, pamd, kat):
    k, A, _, y = kat
    lu = lambda m, n, colptr, rowval, nzval: pamd.pvector._main_lu(pamd.CSC(m, n, colptr, rowval, nzval))
    x = R.solve(A, y, lu)
    res = _residual(O, A, x, y)
    print(f"norm(A*x - y) = {res:.3e} (bound {k['residual_tol']:.1e})")
    assert res < k["residual_tol"]


def test_main_lu_scipy_and_dense_paths_agree(O, pamd, kat, monkeypatch):
    k, A, D, _ = kat
    csc = pamd.CSC(*R.canonical_csc(R.gather_matrix(A).values.parts[R.MAIN - 1]))
    rhs = np.ones(k["n"])
    F = pamd.pvector._main_lu(csc)
    assert not isinstance(F, pamd.pvector._DenseLU), "scipy is on the image: the sparse path is expected"
    xs = F.solve(rhs)
    # the import is made to fail, nothing else: the dense path takes the same CSC
    monkeypatch.setitem(sys.modules, "scipy.sparse.linalg", None)
    G = pamd.pvector._main_lu(csc)
    assert isinstance(G, pamd.pvector._DenseLU)
    xd = G.solve(rhs)
    monkeypatch.undo()
    for name, x in (("scipy", xs), ("dense", xd)):
        res = np.linalg.norm(D @ x - rhs)
        print(f"{name}: norm(D*x - 1) = {res:.3e}")
        assert res < k["residual_tol"], name
    assert np.linalg.norm(xs - xd) < k["residual_tol"]


def test_main_lu_names_what_is_missing_above_the_dense_limit(pamd, monkeypatch):
    n = 8193
    one = np.arange(1, n + 2, dtype=np.int64)
    csc = pamd.CSC(n, n, one, one[:-1], np.ones(n))
    monkeypatch.setitem(sys.modules, "scipy.sparse.linalg", None)
    with pytest.raises(pamd.PAError, match="scipy"):
        pamd.pvector._main_lu(csc)
    monkeypatch.undo()
    assert np.array_equal(pamd.pvector._main_lu(csc).solve(np.full(n, 3.0)), np.full(n, 3.0))


def test_main_lu_keeps_float32(pamd):
    csc = pamd.CSC(2, 2, [1, 2, 3], [1, 2], np.array([2.0, 4.0], np.float32))
    assert pamd.pvector._main_lu(csc).solve(np.array([1.0, 1.0], np.float32)).dtype == np.float32


def test_host_ranges_and_to_gids(pamd):
    """to_main and to_gids_ on the sequential backend (the host paths)"""
    parts = pamd.sequential.get_part_ids(4)
    rows = pamd.prange_linear(parts, 2)  # MAIN and part 2 own nothing: part 2 has no lid in the range in MAIN
    m = pamd.to_main(rows)
    assert [s.num_lids for s in m.partition.parts] == [2] + [s.num_oids for s in rows.partition.parts[1:]]
    assert 0 in [s.num_lids for s in m.partition.parts]
    assert all((s.lid_to_part == pamd.MAIN).all() for s in m.partition.parts)
    cols = pamd.prange_linear(parts, 10)
    pamd.add_gids_(cols, pamd.map_parts(lambda p: np.array([1, 10, 5], np.int64), parts))
    lids = pamd.map_parts(lambda s: np.arange(1, s.num_lids + 1, dtype=np.int64), cols.partition)
    g = pamd.to_gids_(lids, cols)
    assert all(np.array_equal(a, s.lid_to_gid) for a, s in zip(g.parts, cols.partition.parts))
    back = pamd.to_lids_(g, cols)
    assert all(np.array_equal(a, np.arange(1, s.num_lids + 1)) for a, s in zip(back.parts, cols.partition.parts))
    bad = pamd.map_parts(lambda s: np.array([1, s.num_lids + 1], np.int64), cols.partition)
    with pytest.raises(IndexError):
        pamd.to_gids_(bad, cols)
    assert all(np.array_equal(a, [1, s.num_lids + 1]) for a, s in zip(bad.parts, cols.partition.parts))
