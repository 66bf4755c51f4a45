"""A reference of the Jacobi-preconditioned CG composed from the oracle's own
operations (mul_, dot, norm, bcast_, copyto_) and numpy's division in T:
diag_ref reads a host matrix's diagonal, pcg_ref runs IterativeSolvers 0.9's
preconditioned iterate.  scaled_* build the badly scaled test system S·A·S
from test_fdm.jl's operator, for the oracle and for the device."""
import numpy as np

ERR_TOL = 1e-5  # test_fdm.jl:118, test_fem_sa.jl:137
# The GPU tests compare residual histories at rtol 1e-8, the figure of the
# existing CG tests.  It stands while the reference's own history moves by at
# most 1e-9 when its dots are summed one term after the other instead of
# pairwise; measured: 5.4e-15 (fdm), 1.4e-14 (fem_sa), 5.9e-10 (scaled fdm).
HISTORY_RTOL = 1e-8
SPREAD_LIMIT = 1e-9


def diag_ref(M, rows, cols, dtype=None):
    """diag of one part: num_lids(cols) values, zero(T) everywhere, then for
    every owned row the stored entry in its own column (owned id k of rows is
    owned id k of cols).  M: a host CSC (colptr, rowval, nzval; 1-based) or
    CSR (Bi, rowptr, colval, nzval); rows, cols: its index sets."""
    nz = np.asarray(M.nzval)
    d = np.zeros(cols.num_lids, dtype or nz.dtype)
    ro, co = np.asarray(rows.oid_to_lid, np.int64), np.asarray(cols.oid_to_lid, np.int64)
    assert len(ro) == len(co)
    if hasattr(M, "rowptr"):
        rp = np.asarray(M.rowptr, np.int64) - M.Bi
        I = np.repeat(np.arange(1, M.m + 1), np.diff(rp))
        J = np.asarray(M.colval, np.int64) - M.Bi + 1
    else:
        cp = np.asarray(M.colptr, np.int64) - 1
        I = np.asarray(M.rowval, np.int64)
        J = np.repeat(np.arange(1, M.n + 1), np.diff(cp))
    own_col = np.zeros(M.m + 1, np.int64)  # row lid -> the lid of its own column (0: a ghost row)
    own_col[ro] = co
    hit = own_col[I] == J
    assert len(np.unique(J[hit])) == int(hit.sum())
    d[J[hit] - 1] = nz[hit].astype(d.dtype)
    return d


def diag_pvector(O, A, dtype=None):
    """diag(A) of an oracle PSparseMatrix as an oracle PVector on A.cols,
    ghosts exchanged from their owners"""
    vals = O.map_parts(lambda M, r, c: diag_ref(M, r, c, dtype), A.values, A.rows.partition, A.cols.partition)
    return O.exchange_pvector_(O.PVector(vals, A.cols))


def t_dot(O, sequential=False):
    """dot as Julia's dot of two PVectors forms it: each product in the
    element type T (the oracle's own dot widens Float32 operands first and
    multiplies in Float64), the part's terms accumulated in Float64 — numpy's
    pairwise np.sum, or one after the other (np.cumsum) when `sequential` —
    the part's value rounded to T, the parts added in T in part order.  For
    Float64 the pairwise form is the oracle's dot; for Float32 it is the dot
    whose scalars ρ, β, α the device recurrence has to reproduce."""
    def dot(a, b):
        T = a.values.parts[0].dtype.type
        s = T(0)
        for x, y, sa, sb in zip(a.values.parts, b.values.parts, a.rows.partition.parts, b.rows.partition.parts):
            t = (O._owned(x, sa) * O._owned(y, sb)).astype(np.float64)
            s = T(s + T((np.cumsum(t)[-1] if sequential else np.sum(t)) if len(t) else 0.0))
        return s
    return dot


def t_norm(O):
    """norm with each square formed in the element type T, as the library
    documents its norm (abs2 in T, the part's sum accumulated in Float64 and
    rounded to T, the parts added in T, the square root in Float64); the
    oracle's own norm widens Float32 values before it squares them.  The same
    function as the oracle's for Float64."""
    def norm(a):
        T = a.values.parts[0].dtype.type
        s = T(0)
        for x, sa in zip(a.values.parts, a.rows.partition.parts):
            xo = O._owned(x, sa)
            s = T(s + T(np.sum((xo * xo).astype(np.float64)) if len(xo) else 0.0))
        return float(s) ** 0.5
    return norm


def pcg_ref(O, x, A, b, d, reltol=None, abstol=0.0, maxiter=None, log=None, dot=None, scalar=None, norm=None):
    """u = 0; r = b - A*x; residual = norm(r); ρ = one(T); per iteration
    c = r ./ d; ρ_prev = ρ; ρ = dot(c, r); β = ρ/ρ_prev; u .= c .+ β.*u;
    c = A*u; α = ρ/dot(u, c); x .+= α.*u; r .-= α.*c; residual = norm(r) —
    ρ, β, α of the element type T, the residual a Float64.  d: an oracle
    PVector on x.rows' partition holding the diagonal on every lid.  `scalar`
    (np.float64) runs the recurrence with scalars of that type instead, what
    the specification rules out: the host test shows that the first residuals
    tell the two apart."""
    dot, norm = dot or O.dot, norm or O.norm
    E = x.values.parts[0].dtype.type
    T = scalar or E
    if reltol is None:
        reltol = float(np.sqrt(np.finfo(E).eps))
    if maxiter is None:
        maxiter = A.cols.ngids
    mk = lambda: O.PVector(O.map_parts(lambda v: np.zeros_like(v), x.values), x.rows)
    u, r, c = mk(), mk(), mk()
    O.copyto_(r, b)
    O.mul_(c, A, x)
    O.bcast_(r, c, None, 3)
    residual = norm(r)
    tol = max(reltol * norm(b), abstol)
    rho = T(1)
    it = 0
    with np.errstate(all="ignore"):
        while not (it >= maxiter or residual <= tol):
            for cv, rv, dv in zip(c.values.parts, r.values.parts, d.values.parts):
                cv[:] = rv / dv
            rho_prev, rho = rho, T(dot(c, r))
            beta = T(rho / rho_prev)
            O.bcast_(u, c, beta, 0)
            O.mul_(c, A, u)
            alpha = T(rho / T(dot(u, c)))
            O.bcast_(x, u, alpha, 1)
            O.bcast_(r, c, alpha, 2)
            residual = norm(r)
            it += 1
            if log is not None:
                log.append(residual)
    return x


# ---------------------------------------------------------------------------
# the badly scaled system: S·A·S x' = S b with S = diag(s), s log-spaced over
# the gids from 1 to 10**DECADES, x' = x ./ s

# s runs from 1 to 10: chosen on the CPU (test_pcg_ref_host.py) so that pcg_ref
# needs at most half of O.cg_'s iterations (30 against 130 at nx = 10; two
# decades: 29 against 556, three: O.cg_ does not converge in 1000)
DECADES = 1.0


def scale_of(gids, n, decades=DECADES):
    return 10.0 ** (decades * (np.asarray(gids, np.float64) - 1.0) / (n - 1.0))


def scaled_oracle_fdm(O, parts, nx=10, decades=DECADES):
    """(A', b', x0', x̂') of the oracle's fdm_problem, scaled"""
    A, b, x0, xh = O.fdm_problem(parts, nx)
    n = nx ** 3

    def mat(M, r, c):
        sr, sc = scale_of(r.lid_to_gid, n, decades), scale_of(c.lid_to_gid, n, decades)
        I = np.asarray(M.rowval, np.int64)
        J = np.repeat(np.arange(1, M.n + 1), np.diff(np.asarray(M.colptr, np.int64)))
        return O.CSC(M.m, M.n, M.colptr, M.rowval, (sr[I - 1] * np.asarray(M.nzval)) * sc[J - 1])
    vals = O.map_parts(mat, A.values, A.rows.partition, A.cols.partition)
    As = O.PSparseMatrix(vals, A.rows, A.cols, A.exchanger)
    mul = lambda v: O.PVector(O.map_parts(lambda a, s: a * scale_of(s.lid_to_gid, n, decades), v.values,
                                          v.rows.partition), v.rows)
    div = lambda v: O.PVector(O.map_parts(lambda a, s: a / scale_of(s.lid_to_gid, n, decades), v.values,
                                          v.rows.partition), v.rows)
    return As, mul(b), div(x0), div(xh)


def scaled_device_fdm(pamd, parts, nx=10, decades=DECADES, dtype=np.float64):
    """the same system on the device, from test_fdm.jl's host COO"""
    rows, cols, I, J, V, bh, xh, x0h = pamd.drivers.fdm_host(parts, nx)
    n = nx ** 3
    Vs = pamd.map_parts(lambda i, j, v, r, c: ((scale_of(r.lid_to_gid[i - 1], n, decades) * v)
                                               * scale_of(c.lid_to_gid[j - 1], n, decades)).astype(dtype),
                        I, J, V, rows.partition, cols.partition)
    A = pamd.PSparseMatrix.from_coo(I, J, Vs, rows, cols, ids="local")
    sc = lambda s: scale_of(s.lid_to_gid, n, decades)
    b = pamd.PVector.from_host(pamd.map_parts(lambda v, s: (v * sc(s)).astype(dtype), bh, rows.partition), rows)
    xhat = pamd.PVector.from_host(pamd.map_parts(lambda v, s: (v / sc(s)).astype(dtype), xh, rows.partition), rows)
    x0 = pamd.PVector.from_host(pamd.map_parts(lambda v, s: (v / sc(s)).astype(dtype), x0h, cols.partition), cols)
    return A, b, x0, xhat


def owned_error(index_sets, x, xh):
    """norm(x - x̂) over the owned values; x, xh: the parts' host values (a
    host PData or an oracle PVector's values), index_sets: their IndexSets"""
    tot = 0.0
    for a, b, s in zip(x.parts, xh.parts, index_sets):
        o = np.asarray(s.oid_to_lid, np.int64) - 1
        tot += float(np.sum((np.asarray(a)[o].astype(np.float64) - np.asarray(b)[o]) ** 2))
    return tot ** 0.5
