"""The reference of the Jacobi-preconditioned CG (tests/pcg_ref.py), pinned
on the CPU before the GPU tests rely on it: it solves the reference's two
driver problems within their own bound, beats the unpreconditioned oracle on
a badly scaled system, and its history does not depend on the summation order
of its dots beyond the tolerance the GPU comparison uses."""
import numpy as np
import pytest

import pcg_ref
from pcg_ref import ERR_TOL, SPREAD_LIMIT


def _copy(O, v):
    return O.PVector(O.map_parts(lambda a: a.copy(), v.values), v.rows)


def _solve(O, A, b, x0, **kw):
    x, hist = _copy(O, x0), []
    pcg_ref.pcg_ref(O, x, A, b, pcg_ref.diag_pvector(O, A), log=hist, **kw)
    return x, hist


def _spread(h1, h2):
    assert len(h1) == len(h2)
    return max(abs(a - b) / abs(b) for a, b in zip(h1, h2))


@pytest.mark.parametrize("problem,nparts", [("fdm_problem", (2, 2, 2)), ("fem_sa_problem", 4),
                                            ("fem_sa_problem", (2, 2))])
def test_pcg_ref_solves_the_driver_problems(O, problem, nparts):
    A, b, x0, xh = getattr(O, problem)(O.get_part_ids(nparts), 10)
    x, hist = _solve(O, A, b, x0)
    err = pcg_ref.owned_error(x.rows.partition.parts, x.values, xh.values)
    print(f"{problem} {nparts}: {len(hist)} iterations, error {err:.3e}")
    assert 0 < len(hist) < 100 and err < ERR_TOL
    _, seq = _solve(O, A, b, x0, dot=pcg_ref.t_dot(O, sequential=True))
    s = _spread(hist, seq)
    print(f"history spread, pairwise against sequential dots: {s:.3e}")
    assert s <= SPREAD_LIMIT


def test_diag_ref_reads_the_owned_diagonal(O):
    A, _, _, _ = O.fem_sa_problem(O.get_part_ids(4), 10)  # stored ghost rows
    for M, r, c in zip(A.values.parts, A.rows.partition.parts, A.cols.partition.parts):
        d = pcg_ref.diag_ref(M, r, c)
        dense = np.zeros((M.m, M.n))
        J = np.repeat(np.arange(M.n), np.diff(M.colptr))
        dense[np.asarray(M.rowval) - 1, J] = M.nzval
        want = np.zeros(M.n)
        for k, (i, j) in enumerate(zip(r.oid_to_lid, c.oid_to_lid)):
            want[j - 1] = dense[i - 1, j - 1]
        assert np.array_equal(d, want) and np.all(d[np.asarray(c.hid_to_lid, int) - 1] == 0)


def test_pcg_ref_beats_cg_on_the_scaled_system(O):
    """S·A·S with s log-spaced from 1 to 10 ** pcg_ref.DECADES = 10 over the
    gids: the range is chosen so that the reference needs at most half of
    O.cg_'s iterations."""
    assert pcg_ref.DECADES == 1.0
    A, b, x0, xh = pcg_ref.scaled_oracle_fdm(O, O.get_part_ids((2, 2, 2)), 10)
    x, hist = _solve(O, A, b, x0)
    xc, hc = _copy(O, x0), []
    O.cg_(xc, A, b, log=hc)
    print(f"scaled fdm: pcg_ref {len(hist)} iterations, O.cg_ {len(hc)}")
    assert 0 < 2 * len(hist) <= len(hc) < A.cols.ngids
    assert pcg_ref.owned_error(x.rows.partition.parts, x.values, xh.values) < ERR_TOL
    _, seq = _solve(O, A, b, x0, dot=pcg_ref.t_dot(O, sequential=True))
    s = _spread(hist, seq)
    print(f"history spread, pairwise against sequential dots: {s:.3e}")
    assert s <= SPREAD_LIMIT


def test_t_dot_is_the_oracle_dot_in_float64_and_pins_float32_scalars(O):
    """Float64: pcg_ref with t_dot is pcg_ref with the oracle's dot, bit for
    bit.  Float32: the history does not depend on the summation order of the
    T products, but it differs from the one the oracle's Float64-product dot
    gives — what the GPU test's bit comparison of the first residuals sees."""
    A, b, x0, _ = O.fdm_problem(O.get_part_ids((2, 2, 2)), 10)
    _, h = _solve(O, A, b, x0)
    _, ht = _solve(O, A, b, x0, dot=pcg_ref.t_dot(O), norm=pcg_ref.t_norm(O))
    assert h == ht
    vals = O.map_parts(lambda M: O.CSC(M.m, M.n, M.colptr, M.rowval, O._convert_values(M.nzval, np.float32)), A.values)
    A32 = O.PSparseMatrix(vals, A.rows, A.cols)
    f32 = lambda v: O.PVector(O.map_parts(lambda a: np.asarray(a, np.float32).copy(), v.values), v.rows)
    _, h32 = _solve(O, A32, f32(b), f32(x0), dot=pcg_ref.t_dot(O))
    _, s32 = _solve(O, A32, f32(b), f32(x0), dot=pcg_ref.t_dot(O, sequential=True))
    _, o32 = _solve(O, A32, f32(b), f32(x0))
    assert h32 == s32 and len(h32) == len(o32) > 5
    assert h32 != o32
    # Float64 scalars (not the specification): the same iteration count and a
    # history inside the GPU test's 5e-6, but not the same first residuals
    _, w32 = _solve(O, A32, f32(b), f32(x0), dot=pcg_ref.t_dot(O), scalar=np.float64)
    rel = max(abs(a - c) / abs(c) for a, c in zip(w32, h32))
    print(f"Float64 against Float32 scalars: {len(w32)} / {len(h32)} iterations, largest relative difference {rel:.3e}")
    assert len(w32) == len(h32) and rel <= 5e-6 and w32[:3] != h32[:3]
    # squares in Float32 (t_norm) instead of the oracle's Float64 squares: the
    # iterates are the same, a residual can differ by one Float32 rounding of Σr²
    _, n32 = _solve(O, A32, f32(b), f32(x0), dot=pcg_ref.t_dot(O), norm=pcg_ref.t_norm(O))
    rel = max(abs(a - c) / abs(c) for a, c in zip(n32, h32))
    print(f"t_norm against the oracle's norm: {sum(a == c for a, c in zip(n32, h32))} of {len(h32)} residuals "
          f"bit-equal, largest relative difference {rel:.3e}")
    assert len(n32) == len(h32) and rel <= 2.0 ** -23
