"""Sequential restatement of the gather-to-MAIN block of the reference
(Interfaces.jl:2664-2748) over the oracle's types: `_to_main`, `gather` of a
PVector and of a PSparseMatrix, and `scatter!`, loop for loop, on top of the
oracle's assemble_, exchange_pvector_, assemble_coo_, psparse_from_coo and
nz_entries.  The expected values of tests/test_gpu_main_solve.py and
tests/test_main_solve_host.py (no GPU here, and nothing of the product)."""
import numpy as np

import pa_oracle as O

MAIN = 1


def as_array(vs):
    """the values of a part as one numpy array (a Cx pair becomes complex,
    signs of zero kept)"""
    if isinstance(vs, O.Cx):
        out = np.empty(len(vs.re), dtype=np.complex64 if vs.re.dtype == np.float32 else np.complex128)
        out.real, out.imag = vs.re, vs.im
        return out
    return np.asarray(vs)


def _dtype(vs):
    return as_array(vs).dtype.type


def to_main(rows):
    """_to_main(rows) (2734-2748)"""
    ngids = rows.ngids

    def mk(s):
        if s.part == MAIN:
            lid_to_gid = list(range(1, ngids + 1))
        else:
            lid_to_gid = [s.lid_to_gid[l - 1] for l in s.oid_to_lid]
        return O.IndexSet(s.part, lid_to_gid, [MAIN] * len(lid_to_gid))
    return O.prange(ngids, O.map_parts(mk, rows.partition))


def gather_vector(b, rows_in_main=None):
    """gather(b::PVector, rows_in_main) (2706-2719)"""
    rows_in_main = rows_in_main if rows_in_main is not None else to_main(b.rows)
    b_in_main = O.pvector_undef(rows_in_main, _dtype(b.values.parts[0]))  # PVector(zero(T), rows_in_main)

    def fill(bv, mv, rows):
        if rows.part == MAIN:
            for l in rows.oid_to_lid:
                O._set(mv, rows.lid_to_gid[l - 1] - 1, O._get(bv, l - 1))
        else:
            for k, l in enumerate(rows.oid_to_lid):
                O._set(mv, k, O._get(bv, l - 1))
    O.map_parts(fill, b.values, b_in_main.values, b.rows.partition)
    return O.assemble_(b_in_main)


def scatter(c, c_in_main):
    """scatter!(c, c_in_main) (2721-2732)"""
    O.exchange_pvector_(c_in_main)

    def take(cv, mv, rows):
        if rows.part == MAIN:
            for l in rows.oid_to_lid:
                O._set(cv, l - 1, O._get(mv, rows.lid_to_gid[l - 1] - 1))
        else:
            for k, l in enumerate(rows.oid_to_lid):
                O._set(cv, l - 1, O._get(mv, k))
    O.map_parts(take, c.values, c_in_main.values, c.rows.partition)
    return c


def owned_coo(A):
    """the (I, J, V) of 2669-2689: the stored entries of the owned rows in
    nziterator order, with global ids"""
    def coo(M, rows, cols):
        nz = as_array(M.nzval)
        I, J, K = [], [], []
        for k, i, j in O.nz_entries(M):
            if rows.lid_to_part[i - 1] == rows.part:
                I.append(rows.lid_to_gid[i - 1])
                J.append(cols.lid_to_gid[j - 1])
                K.append(k - 1)
        return I, J, nz[np.asarray(K, dtype=np.int64)].copy()
    return O.unzip(O.map_parts(coo, A.values, A.rows.partition, A.cols.partition), 3)


def gather_matrix(A, rows_in_main=None, cols_in_main=None):
    """gather(a::PSparseMatrix, rows_in_main, cols_in_main) (2664-2704); the
    parent kind (CSC, or CSR{Bi}) of A's local matrices is kept"""
    rows_in_main = rows_in_main if rows_in_main is not None else to_main(A.rows)
    cols_in_main = cols_in_main if cols_in_main is not None else to_main(A.cols)
    I, J, V = owned_coo(A)
    dt = V.parts[0].dtype
    I, J, V = O.assemble_coo_(I, J, V, rows_in_main)
    parts = [s.part for s in A.rows.partition.parts]
    I = O.PData([i if p == MAIN else [] for i, p in zip(I.parts, parts)], I.shape)
    J = O.PData([j if p == MAIN else [] for j, p in zip(J.parts, parts)], J.shape)
    V = O.PData([np.asarray(v, dtype=dt) if p == MAIN else np.zeros(0, dt) for v, p in zip(V.parts, parts)], V.shape)
    first = A.values.parts[0]
    init = None
    if isinstance(first, O.CSR):
        init = lambda i, j, v, m, n, Bi=first.Bi: O.sparse_csr(Bi, i, j, v, m, n)
    a_in_main = O.psparse_from_coo(I, J, V, rows_in_main, cols_in_main, ids="global", init=init)
    a_in_main.exchanger = O.empty_exchanger(rows_in_main.partition)
    return a_in_main


def entries(M):
    """(I, J, V) of a local matrix in nziterator order, 1-based lids"""
    nz = as_array(M.nzval)
    e = O.nz_entries(M)
    return (np.array([i for _, i, _ in e], np.int64), np.array([j for _, _, j in e], np.int64),
            nz[np.array([k - 1 for k, _, _ in e], np.int64)])


def canonical_csc(M):
    """(m, n, colptr, rowval, nzval) of a local matrix as the CSC with rows
    ascending in every column (1-based), whatever the parent kind"""
    I, J, V = entries(M)
    o = np.lexsort((I, J))
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(J - 1, minlength=M.n))]).astype(np.int64)
    return M.m, M.n, colptr, I[o], V[o]


def solve(A, b, main_lu, dtype=None):
    """A \\ b (2626-2638) with `main_lu(m, n, colptr, rowval, nzval)`, an
    object with solve(rhs), standing for the `\\` on MAIN"""
    a_in_main = gather_matrix(A)
    b_in_main = gather_vector(b, a_in_main.rows)
    m, n, colptr, rowval, nzval = canonical_csc(a_in_main.values.parts[MAIN - 1])
    dtype = dtype or np.result_type(nzval.dtype, as_array(b.values.parts[0]).dtype)
    x = main_lu(m, n, colptr, rowval, nzval.astype(dtype)).solve(as_array(b_in_main.values.parts[MAIN - 1]).astype(dtype))
    c = O.pvector_undef(A.cols, np.dtype(dtype).type)
    c_in_main = O.pvector_undef(a_in_main.cols, np.dtype(dtype).type)
    for k in range(n):
        O._set(c_in_main.values.parts[MAIN - 1], k, O.Cx(x[k].real, x[k].imag) if np.iscomplexobj(x) else x[k])
    return scatter(c, c_in_main)
