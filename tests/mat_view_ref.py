"""Sequential numpy restatement of the entry views of a PSparseMatrix
(local_view / global_view, Interfaces.jl:2277-2298 over the getindex /
setindex! of 2004-2069) over one part's local matrix with a fixed pattern:
`nzval[nzindex(i, j)] += V[k]` / `= V[k]` in input order, in the element
type, and reads that give zero(T) for entries the pattern does not store.
The expected values of tests/test_gpu_mat_view.py (no GPU here)."""
import numpy as np


class Pattern:
    """The pattern of a local CSC (`major="col"`: ptr = colptr, idx = rowval)
    or CSR (`major="row"`: ptr = rowptr, idx = colval) matrix of m x n, with
    indices in base `base` (1 for a SparseMatrixCSC, Bi for a CSR).  Entries
    of a row / column need not be sorted."""

    def __init__(self, m, n, ptr, idx, major="col", base=1):
        assert major in ("col", "row")
        self.m, self.n, self.major = int(m), int(n), major
        ptr = np.asarray(ptr, dtype=np.int64) - base
        self.minor = np.asarray(idx, dtype=np.int64) - base  # 0-based rows (CSC) / cols (CSR) in storage order
        self.majorv = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
        self.nnz = len(self.minor)
        w = self.m if major == "col" else self.n
        self._w = w
        key = self.majorv * w + self.minor
        self._order = np.argsort(key, kind="stable")
        self._key = key[self._order]

    def rows_cols(self):
        """0-based (row, col) of the nonzeros in storage order"""
        return (self.minor, self.majorv) if self.major == "col" else (self.majorv, self.minor)

    def nzindex(self, I, J):
        """0-based storage position of each (I[k], J[k]) (1-based ids), -1
        where the pattern does not store it or an id is out of range"""
        I, J = np.asarray(I, dtype=np.int64) - 1, np.asarray(J, dtype=np.int64) - 1
        ok = (I >= 0) & (I < self.m) & (J >= 0) & (J < self.n)
        q = (J * self._w + I) if self.major == "col" else (I * self._w + J)
        pos = np.searchsorted(self._key, q)
        hit = ok & (pos < self.nnz)
        hit[hit] = self._key[pos[hit]] == q[hit]
        out = np.full(len(I), -1, dtype=np.int64)
        out[hit] = self._order[pos[hit]]
        return out


def scatter_add(nzval, pat, I, J, V):
    """nzval[nzindex(I[k], J[k])] += V[k] for k in input order; every (i, j)
    must be stored.  Returns nzval (modified in place)."""
    V = np.asarray(V, dtype=nzval.dtype)
    p = pat.nzindex(I, J)
    assert (p >= 0).all(), "a write to an entry the pattern does not store"
    for k, q in enumerate(p):
        nzval[q] = nzval[q] + V[k]
    return nzval


def scatter_set(nzval, pat, I, J, V):
    """nzval[nzindex(I[k], J[k])] = V[k] in input order: the last entry of an
    (i, j) stays"""
    V = np.asarray(V, dtype=nzval.dtype)
    p = pat.nzindex(I, J)
    assert (p >= 0).all(), "a write to an entry the pattern does not store"
    for k, q in enumerate(p):
        nzval[q] = V[k]
    return nzval


def gather(nzval, pat, I, J):
    """nzval[nzindex(I[k], J[k])], or zero(T) where (i, j) is not stored (or
    an id is < 1: the LocalView read of an absent lid, 2019-2026)"""
    p = pat.nzindex(I, J)
    out = np.zeros(len(p), dtype=nzval.dtype)
    out[p >= 0] = nzval[p[p >= 0]]
    return out


def bits(a):
    """the values as unsigned integers: equality of these is bit identity
    (sign of zero and NaN payloads included)"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.real.dtype.itemsize == 4 else np.uint64)
