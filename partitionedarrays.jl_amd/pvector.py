"""PVector / PSparseMatrix on HIP parts and the hot path (Interfaces.jl:1576-2757).

Values live in HBM (one pa_vec / pa_mat per part); every operation below is
a libpa_hip.so call — there is no host fallback.  Host arrays appear only at
construction (upload of the reference's local CSC / initial values) and when
the caller asks for them (`to_host`).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
import math
import sys
import weakref

import numpy as np

from . import _lib
from .backends import MAIN, PData, exchange, get_part_ids, map_parts, unzip
from .backends import gather as _gather_pdata
from .device import (DeviceArray, DeviceCOO, DeviceIndex, DeviceMatrix, DeviceMatrixExchanger, DeviceTable,
                     DeviceVector, Task, contexts, device_exchanger, device_index, device_index_gids)
from .helpers import Table, counts_to_ptrs, trace_setup
from .prange import (Exchanger, PRange, _cached_eq, add_gids_, empty_exchanger, hids_are_equal, lids_are_equal,
                     oids_are_equal, prange_linear, to_main)


# ---------------------------------------------------------------------------
# Local CSC (setup): SparseArrays.sparse semantics, SparseUtils.jl:80-94

class CSC:
    """SparseMatrixCSC{T,Int64}: 1-based colptr/rowval."""

    def __init__(self, m, n, colptr, rowval, nzval):
        self.m, self.n = int(m), int(n)
        self.colptr = np.asarray(colptr, dtype=np.int64)
        self.rowval = np.asarray(rowval, dtype=np.int64)
        self.nzval = np.asarray(nzval)

    @property
    def nnz(self):
        return int(self.colptr[-1] - 1)


def compresscoo(I, J, V, m, n) -> CSC:
    """sparse(I, J, V, m, n, +): duplicates combined with `+` in input order
    (left fold from the first occurrence), rows ascending within columns."""
    I = np.asarray(I, dtype=np.int64).ravel()
    J = np.asarray(J, dtype=np.int64).ravel()
    V = np.asarray(V).ravel()
    k = len(I)
    if k and (I.min() < 1 or I.max() > m or J.min() < 1 or J.max() > n):
        raise IndexError("compresscoo: index out of bounds")
    order = np.lexsort((np.arange(k), I, J))
    Is, Js, Vs = I[order], J[order], V[order]
    new = np.ones(k, dtype=bool)
    new[1:] = (Is[1:] != Is[:-1]) | (Js[1:] != Js[:-1])
    starts = np.flatnonzero(new)
    sizes = np.diff(np.append(starts, k))
    acc = Vs[starts].copy()
    for t in range(1, int(sizes.max()) if k else 1):
        sel = sizes > t
        acc[sel] = acc[sel] + Vs[starts[sel] + t]
    cols = Js[starts]
    colptr = np.concatenate([[1], 1 + np.cumsum(np.bincount(cols - 1, minlength=n))]).astype(np.int64)
    return CSC(m, n, colptr, Is[starts], acc)


class CSR:
    """SparseMatrixCSR{Bi,T,Int64} (SparseUtils.jl:189-300): rowptr and
    colval hold Bi-based indices (Bi = 0 or 1), nzval in row order."""

    def __init__(self, Bi, m, n, rowptr, colval, nzval):
        if Bi not in (0, 1):
            raise ValueError("SparseMatrixCSR: Bi must be 0 or 1")
        self.Bi, self.m, self.n = int(Bi), int(m), int(n)
        self.rowptr = np.asarray(rowptr, dtype=np.int64)
        self.colval = np.asarray(colval, dtype=np.int64)
        self.nzval = np.asarray(nzval)

    @property
    def nnz(self):
        return int(self.rowptr[-1] - self.Bi)


def sparsecsr(Bi, I, J, V, m, n) -> CSR:
    """compresscoo(SparseMatrixCSR{Bi}, I, J, V, m, n) (SparseUtils.jl:
    193-208) → sparsecsr(Val(Bi), I, J, V, m, n, +): the CSC of the
    transposed triplets read as rows (duplicates combined with + in input
    order, columns ascending within rows), indices shifted to base Bi."""
    t = compresscoo(J, I, V, n, m)
    return CSR(Bi, m, n, t.colptr - 1 + Bi, t.rowval - 1 + Bi, t.nzval)


class csr_init:
    """init for PSparseMatrix.from_coo: sparsecsr with index base Bi (the
    compress then runs on the device, pa_mat_from_coo_csr); called as
    init(I, J, V, m, n) it is the host sparsecsr."""

    def __init__(self, Bi):
        if Bi not in (0, 1):
            raise ValueError("SparseMatrixCSR: Bi must be 0 or 1")
        self.Bi = int(Bi)

    def __call__(self, I, J, V, m, n):
        return sparsecsr(self.Bi, I, J, V, m, n)


# ---------------------------------------------------------------------------
# PVector

class _ExprOps:
    """The operators that build a lazy Broadcasted node (Julia's dotted
    operators on PVectors, Interfaces.jl:1722-1765); shared by PVector and
    Broadcasted.  No __eq__ / __ne__: identity and hashing stay the
    default (use eq / ne / isequal)."""

    __array_ufunc__ = None  # numpy scalars on the left defer to __radd__ etc.

    def __add__(self, o):
        return _node("add", self, o)

    def __radd__(self, o):
        return _node("add", o, self)

    def __sub__(self, o):
        return _node("sub", self, o)

    def __rsub__(self, o):
        return _node("sub", o, self)

    def __mul__(self, o):
        return _node("mul", self, o)

    def __rmul__(self, o):
        return _node("mul", o, self)

    def __truediv__(self, o):
        return _node("div", self, o)

    def __rtruediv__(self, o):
        return _node("div", o, self)

    def __neg__(self):
        return _node("neg", self)

    def __abs__(self):
        return _node("abs", self)

    def __lt__(self, o):
        return _node("lt", self, o)

    def __le__(self, o):
        return _node("le", self, o)

    def __gt__(self, o):
        return _node("gt", self, o)

    def __ge__(self, o):
        return _node("ge", self, o)


class PVector(_ExprOps):
    """PVector{T}(values, rows) (Interfaces.jl:1576-1587): values = PData of
    DeviceVector (num_lids(rows) entries per part)."""

    def __init__(self, values: PData, rows: PRange):
        self.values = values
        self.rows = rows

    @property
    def dtype(self):
        return self.values.parts[0].dtype if self.values.parts else np.dtype(np.float64)

    def __len__(self):
        return len(self.rows)

    @staticmethod
    def undef(rows: PRange, dtype=np.float64) -> "PVector":
        """PVector{T}(undef, rows) (Interfaces.jl:1869-1878); zero-initialised."""
        ctxs = contexts(rows.partition)
        vals = [DeviceVector(c, dtype, s.num_lids) for c, s in zip(ctxs, rows.partition.parts)]
        return PVector(PData(rows.partition.backend, rows.partition.part_ids, vals, rows.partition.shape), rows)

    @staticmethod
    def full(v, rows: PRange, dtype=None) -> "PVector":
        """PVector(v::Number, rows) (Interfaces.jl:1880-1884)"""
        dtype = dtype or np.asarray(v).dtype
        a = PVector.undef(rows, dtype)
        a.fill_(v)
        return a

    @staticmethod
    def from_host(host: PData, rows: PRange, dtype=None) -> "PVector":
        dtype = dtype or np.asarray(host.parts[0]).dtype
        a = PVector.undef(rows, dtype)
        for dv, h in zip(a.values.parts, host.parts):
            dv.upload(h)
        return a

    @staticmethod
    def from_coo(I: PData, V: PData, rows_or_n, ids, dtype=None) -> "PVector":
        """PVector(I, V, rows; ids=:global|:local) (Interfaces.jl:1887-1918):
        values[lid] += V[i] from zero, in input order, on the device
        (pa_vec_scatter); with ids="global" the Int64 arrays of I are
        translated to lids in place, as to_lids! does there.  With a number n
        instead of rows it is PVector(I, V, n; ids=:global) (1920-1932):
        rows = PRange(parts, n) and add_gids!(rows, I) first.  I, V: PData of
        host arrays, or of DeviceArray (rows form only)."""
        if ids not in ("global", "local"):
            raise ValueError("PVector(I, V, rows; ids): ids must be 'global' or 'local'")
        if isinstance(rows_or_n, PRange):
            rows = rows_or_n
        else:
            if ids != "global":
                raise ValueError("PVector(I, V, n; ids): ids must be 'global'")
            rows = prange_linear(get_part_ids(I), int(rows_or_n))
            add_gids_(rows, I)
        if dtype is None:
            v0 = V.parts[0]
            dtype = v0.dtype if isinstance(v0, DeviceArray) else np.asarray(v0).dtype
        if np.dtype(dtype) not in _lib.DTYPES:
            raise TypeError(f"PVector(I, V, rows): element type {np.dtype(dtype)} is not held on the device; pass dtype")
        a = PVector.undef(rows, dtype)
        _scatter_parts(a, I, V, ids, _lib.PA_SCATTER_ADD, zero_first=True)
        return a

    def to_host(self) -> PData:
        return map_parts(lambda v: v.download(), self.values)

    def owned_values(self) -> PData:
        """owned_values view (Interfaces.jl:1589-1593), as host copies"""
        return map_parts(lambda v, s: v.download()[s.oid_to_lid - 1], self.values, self.rows.partition)

    def ghost_values(self) -> PData:
        return map_parts(lambda v, s: v.download()[s.hid_to_lid - 1], self.values, self.rows.partition)

    def similar(self, dtype=None, rows=None) -> "PVector":
        """similar(a[, T][, axes]) (Interfaces.jl:1615-1633)"""
        return PVector.undef(rows or self.rows, dtype or self.dtype)

    def fill_(self, v):
        """fill!(a, v) (Interfaces.jl:1966-1971)"""
        for dv in self.values.parts:
            dv.fill(v)
        return self

    def copy(self) -> "PVector":
        """copy(b) (Interfaces.jl:1669-1673)"""
        a = self.similar()
        copyto_(a, self)
        return a


def _index_sets(rng: PRange, glob=False):
    """the device index sets of a range's parts (with their gid tables when glob)"""
    mk = device_index_gids if glob else device_index
    return [mk(c, s) for c, s in zip(contexts(rng.partition), rng.partition.parts)]


def _idx(v: PVector):
    return [x.h for x in _index_sets(v.rows)]


def copyto_(a: PVector, b: PVector) -> PVector:
    """copyto!(a, b) (Interfaces.jl:1659-1667): all lids when both share the
    partition, owned values otherwise."""
    same = a.rows.partition is b.rows.partition
    if not same and not oids_are_equal(a.rows, b.rows):
        raise AssertionError("copyto!: owned ids differ")
    ia, ib = _idx(a), _idx(b)
    for da, db, xa, xb in zip(a.values.parts, b.values.parts, ia, ib):
        _lib.call("pa_vec_copy", da.h, xa, db.h, xb, 1 if same else 0)
    return a


def _scatter_parts(v: PVector, I: PData, V: PData, ids, op, zero_first=False):
    if I.part_ids != v.values.part_ids or V.part_ids != v.values.part_ids:
        raise ValueError("PVector(I, V, rows): partitioned data over different parts")
    glob = ids == "global"
    for dv, x, i, w in zip(v.values.parts, _index_sets(v.rows, glob), I.parts, V.parts):
        dv.scatter(x, i, w, ids_global=glob, op=op, zero_first=zero_first)
    return v


def add_coo_(v, I: PData, *args, ids="global"):
    """add_coo_(v, I, V, ids): the batched `view[I] .+= V` over
    global_view(v, v.rows) (ids="global") or local_view(v, v.rows)
    (ids="local"): v[I[k]] += V[k] in input order on every part, on the
    device (test_fem_sa.jl:86-101 as one call per part).  Int64 arrays of
    global ids are translated to lids in place, as in PVector.from_coo.

    add_coo_(A, I, J, V, ids) for a PSparseMatrix A: `view[I, J] .+= V` over
    global_view(A, A.rows, A.cols) / local_view(A, A.rows, A.cols), the
    re-assembly loop of a fixed pattern (test_fem_sa.jl:74-84 after
    fillstored!(A, 0)): A[I[k], J[k]] += V[k] over the stored entries in
    input order, owned and ghost rows (pa_mat_scatter).  I and J stay as
    they are; an (i, j) the pattern does not store is an error.  Returns its
    first argument."""
    nfix = 2 if isinstance(v, PSparseMatrix) else 1  # J, V or V; then ids may follow positionally
    if len(args) == nfix + 1:
        args, ids = args[:nfix], args[nfix]
    if len(args) != nfix:
        raise TypeError("add_coo_(v, I, V, ids) for a PVector, add_coo_(A, I, J, V, ids) for a PSparseMatrix")
    if ids not in ("global", "local"):
        raise ValueError("add_coo_: ids must be 'global' or 'local'")
    if nfix == 1:
        return _scatter_parts(v, I, args[0], ids, _lib.PA_SCATTER_ADD)
    J, V = args
    if any(x.part_ids != v.values.part_ids for x in (I, J, V)):
        raise ValueError("add_coo_(A, I, J, V): partitioned data over different parts")
    glob = ids == "global"
    for M, (r, c), i, j, w in zip(v.values.parts, _mat_index(v, glob), I.parts, J.parts, V.parts):
        M.scatter(r, c, i, j, w, ids_global=glob, op=_lib.PA_SCATTER_ADD)
    return v


def _mat_index(A, glob: bool):
    """per part, the device index sets of A's rows and cols (with their gid
    tables when glob)"""
    return list(zip(_index_sets(A.rows, glob), _index_sets(A.cols, glob)))


def _mapped_ids(ids, gids):
    """the lids `ids` of a mapped view's range as gids (gids: its lid_to_gid)"""
    ids = np.asarray(ids).astype(np.int64).ravel()
    if len(ids) and (ids.min() < 1 or ids.max() > len(gids)):
        raise _lib.PAError("local_view: a local id is out of range (BoundsError)")
    return gids[ids - 1]


class VectorView:
    """One part's GlobalView / LocalView of a PVector (Interfaces.jl:
    2004-2069) with batched access: get(ids) = view[ids], set_(ids, vals) =
    `view[ids] = vals` (a repeated id keeps its last value), add_(ids, vals)
    = `view[ids] .+= vals` in input order.  The caller's ids stay as they are.

    kind "local": ids are lids of the vector's own range (out of range: an
    error).  kind "global": ids are gids; a read of a gid that is not a
    local id is an error (gid_to_lid[g], 2062-2065).  kind "mapped"
    (local_view over another range): ids are lids of that range, `gids` its
    lid_to_gid; an id the vector does not store reads zero(T) (2019-2026) and
    cannot be written (2027-2031)."""

    def __init__(self, dv: DeviceVector, idx, kind, gids=None):
        self.dv, self.idx, self.kind, self.gids = dv, idx, kind, gids

    def _ids(self, ids):
        return _mapped_ids(ids, self.gids) if self.kind == "mapped" else np.array(ids)

    def get(self, ids):
        return self.dv.gather(self.idx, self._ids(ids), ids_global=self.kind != "local",
                              absent_zero=self.kind == "mapped")

    def set_(self, ids, vals):
        self.dv.scatter(self.idx, self._ids(ids), vals, ids_global=self.kind != "local", op=_lib.PA_SCATTER_SET)
        return self

    def add_(self, ids, vals):
        self.dv.scatter(self.idx, self._ids(ids), vals, ids_global=self.kind != "local", op=_lib.PA_SCATTER_ADD)
        return self


class MatrixView:
    """One part's GlobalView / LocalView of a PSparseMatrix (Interfaces.jl:
    2277-2298 over 2004-2069) with batched access over the stored entries:
    get(I, J) = view[I[k], J[k]], set_(I, J, V) = `view[i, j] = v` (a repeated
    (i, j) keeps its last value), add_(I, J, V) = `view[i, j] += v` in input
    order.  An (i, j) the pattern does not store reads zero(T) and cannot be
    written (the reference would insert it; the device pattern is fixed).

    kind "local": lids of the matrix's own rows and cols.  kind "global":
    gids.  kind "mapped" (local_view over other ranges): lids of those
    ranges, mapped to gids on the host (`rgids`, `cgids`: their lid_to_gid)
    and looked up on the device; a lid the matrix's ranges do not hold reads
    zero(T) (2019-2026) and cannot be written (2027-2031)."""

    def __init__(self, M: DeviceMatrix, ridx, cidx, kind, rgids=None, cgids=None):
        self.M, self.ridx, self.cidx, self.kind, self.rgids, self.cgids = M, ridx, cidx, kind, rgids, cgids

    def _ids(self, ids, gids):
        return _mapped_ids(ids, gids) if self.kind == "mapped" else ids

    def get(self, I, J):
        return self.M.gather(self.ridx, self.cidx, self._ids(I, self.rgids), self._ids(J, self.cgids),
                             ids_global=self.kind != "local", absent_zero=self.kind == "mapped")

    def _write(self, I, J, V, op):
        self.M.scatter(self.ridx, self.cidx, self._ids(I, self.rgids), self._ids(J, self.cgids), V,
                       ids_global=self.kind != "local", op=op)
        return self

    def set_(self, I, J, V):
        return self._write(I, J, V, _lib.PA_SCATTER_SET)

    def add_(self, I, J, V):
        return self._write(I, J, V, _lib.PA_SCATTER_ADD)


def _mat_views(A, rows, cols, glob: bool):
    p = A.values
    own = (rows is None or rows is A.rows) and (cols is None or cols is A.cols)
    if glob:
        if not own:
            raise NotImplementedError("global_view(a, rows, cols): only for rows === a.rows and cols === a.cols "
                                      "(Interfaces.jl:2291-2292)")
        views = [MatrixView(M, r, c, "global") for M, (r, c) in zip(p.parts, _mat_index(A, True))]
    elif own:
        views = [MatrixView(M, r, c, "local") for M, (r, c) in zip(p.parts, _mat_index(A, False))]
    else:
        rows, cols = A.rows if rows is None else rows, A.cols if cols is None else cols
        if rows.partition.part_ids != p.part_ids or cols.partition.part_ids != p.part_ids:
            raise ValueError("local_view: rows / cols over different parts")
        views = [MatrixView(M, r, c, "mapped", np.asarray(s.lid_to_gid, dtype=np.int64),
                            np.asarray(t.lid_to_gid, dtype=np.int64))
                 for M, (r, c), s, t in zip(p.parts, _mat_index(A, True), rows.partition.parts, cols.partition.parts)]
    return PData(p.backend, p.part_ids, views, p.shape)


def global_view(v, rows: PRange = None, cols: PRange = None) -> PData:
    """global_view(a, rows) (Interfaces.jl:2037-2043): per part, the values
    indexed by global ids; only over the vector's own rows (2038).
    global_view(A, rows, cols) for a PSparseMatrix (2290-2298): MatrixView
    per part, only over the matrix's own rows and cols."""
    if isinstance(v, PSparseMatrix):
        return _mat_views(v, rows, cols, True)
    if cols is not None:
        raise TypeError("global_view(a, rows): a PVector has no cols")
    if rows is not None and rows is not v.rows:
        raise NotImplementedError("global_view(a, rows): only for rows === a.rows (Interfaces.jl:2038)")
    views = [VectorView(dv, x, "global") for dv, x in zip(v.values.parts, _index_sets(v.rows, True))]
    return PData(v.values.backend, v.values.part_ids, views, v.values.shape)


def local_view(v, rows: PRange = None, cols: PRange = None) -> PData:
    """local_view(a, rows) (Interfaces.jl:1994-2002): per part, the values
    indexed by the local ids of rows.  Over the vector's own rows these are
    its lids; over another range each lid is mapped to its gid on the host
    (find_lid_map's role) and looked up in the vector's gid table on the
    device.  local_view(A, rows, cols) for a PSparseMatrix (2277-2288):
    MatrixView per part, over the matrix's own ranges or, mapped the same
    way, over others."""
    if isinstance(v, PSparseMatrix):
        return _mat_views(v, rows, cols, False)
    if cols is not None:
        raise TypeError("local_view(a, rows): a PVector has no cols")
    p = v.values
    if rows is None or rows is v.rows:
        views = [VectorView(dv, x, "local") for dv, x in zip(p.parts, _index_sets(v.rows))]
    else:
        if rows.partition.part_ids != p.part_ids:
            raise ValueError("local_view: rows over different parts")
        views = [VectorView(dv, x, "mapped", np.asarray(s.lid_to_gid, dtype=np.int64))
                 for dv, x, s in zip(p.parts, _index_sets(v.rows, True), rows.partition.parts)]
    return PData(p.backend, p.part_ids, views, p.shape)


def _scalar_kind(a, dtype):
    """the scalar of a broadcast as Julia types it: a Python float is a
    Float64 and a Python complex a ComplexF64 (np.float64 / np.complex128
    likewise) — the elements are then evaluated in Float64 / ComplexF64 and
    rounded once (pa_vec_axpby PA_BCAST_*); ints and scalars of narrower or
    equal type are converted to the element type."""
    cplx = np.dtype(dtype).kind == "c"
    if isinstance(a, (complex, np.complex128)) and not isinstance(a, (float, np.floating)):
        if not cplx:
            if complex(a).imag != 0:
                raise TypeError("broadcast: a complex scalar into a real vector (InexactError)")
            return np.float64(complex(a).real), _lib.PA_BCAST_F64
        return np.complex128(a), _lib.PA_BCAST_C128
    if isinstance(a, (float, np.float64)):
        return np.float64(a), _lib.PA_BCAST_F64
    return a, 0


def _bcast_expr(y: PVector, x: PVector, a, kind, mode):
    """the named broadcast `mode` as an expression over y and x; the scalar
    keeps pa_vec_axpby's typing (kind 0: converted to the element type)"""
    if kind == 0:
        a = np.dtype(y.dtype).type(a)
    if mode == 0:
        return x + a * y
    if mode == 1:
        return y + a * x
    return y - a * x if mode == 2 else y - x


def _bcast(y: PVector, x: PVector, a, mode):
    all_lids = 1 if (x is None or y.rows is x.rows) else 0
    if x is not None and not all_lids and not oids_are_equal(y.rows, x.rows):
        raise AssertionError("broadcast: owned ids differ")
    a, kind = _scalar_kind(a if a is not None else 0, y.dtype)
    if x is not None and not all_lids and not lids_are_equal(y.rows, x.rows):
        # pa_vec_axpby reads x through y's index set: only for one lid layout.
        # Equal owned ids in another lid order (or next to other ghosts) go
        # through the expression path, which carries one map per operand.
        return assign_(y, _bcast_expr(y, x, a, kind, mode))
    iy = _idx(y)
    mode |= kind
    buf, bp = _lib.scalar_buf(a, a.dtype if kind else y.dtype)
    xs = x.values.parts if x is not None else [None] * len(y.values.parts)
    for dy, dx, i in zip(y.values.parts, xs, iy):
        _lib.call("pa_vec_axpby", dy.h, dx.h if dx is not None else None, i, bp, mode, all_lids)
    return y


def xpby_(u: PVector, r: PVector, beta):
    """u .= r .+ β .* u"""
    return _bcast(u, r, beta, 0)


def axpy_(x: PVector, alpha, u: PVector):
    """x .+= α .* u"""
    return _bcast(x, u, alpha, 1)


def axmy_(r: PVector, alpha, c: PVector):
    """r .-= α .* c"""
    return _bcast(r, c, alpha, 2)


def sub_(r: PVector, c: PVector):
    """r .-= c"""
    return _bcast(r, c, None, 3)


def rmul_(a: PVector, v):
    """rmul!(a, v) (Interfaces.jl:1675-1680)"""
    return _bcast(a, None, v, 4)


def _hs(objs):
    return _lib.ptr_array([o.h if o is not None else None for o in objs])


def exchange_(v, rows: PRange = None):
    """exchange!(v) (Interfaces.jl:453-458, 2071-2075): owner → ghost values.
    For a PSparseMatrix: exchange!(A) over nonzeros(A) (2375-2381).  For a
    COO and its rows: exchange!(I, J, V, rows) (2494-2592) on the device."""
    if isinstance(v, COO):
        if rows is None:
            raise TypeError("exchange!(I, J, V, rows): the rows PRange is required")
        return _coo_all("pa_coo_exchange_all", v, rows)
    if isinstance(v, PSparseMatrix):
        return _mat_exchange(v, _lib.PA_REPLACE, 0, 0)
    ctxs = contexts(v.values)
    xg = [device_exchanger(c, v.rows.exchanger, p) for c, p in zip(ctxs, v.values.part_ids)]
    n = len(ctxs)
    _lib.call("pa_exchange_all", n, _hs(v.values.parts), _hs(xg), _lib.ptr_array(_idx(v)),
              _lib.PA_REPLACE, 0, 0)
    return v


class COO:
    """The (I, J, V) triplets of a PSparseMatrix before `sparse`, on the
    device: one pa_coo per part, I and J global ids (test_fem_sa.jl:60-131,
    ids=:global)."""

    def __init__(self, values: PData):
        self.values = values

    @staticmethod
    def from_host(I: PData, J: PData, V: PData, rows: PRange) -> "COO":
        ctxs = contexts(rows.partition)
        parts = [DeviceCOO(c, i, j, v) for c, i, j, v in zip(ctxs, I.parts, J.parts, V.parts)]
        p = rows.partition
        return COO(PData(p.backend, p.part_ids, parts, p.shape))

    def to_host(self):
        """(I, J, V) as PData of host arrays"""
        return unzip(map_parts(lambda c: c.download(), self.values), 3)

    def global_cols(self) -> PData:
        """J of every part (host), e.g. for add_gids!(cols, J)"""
        return map_parts(lambda c: c.download()[1], self.values)


def _coo_all(entry: str, coo: COO, rows: PRange) -> COO:
    """pa_coo_assemble_all — async_assemble!(I, J, V, rows) + wait
    (Interfaces.jl:2406-2492) on the device: triplets of rows owned elsewhere
    go to the owner (local value set to zero, entry kept), received ones are
    appended in rows.exchanger.parts_snd order — or pa_coo_exchange_all —
    async_exchange!(I, J, V, rows) + wait (2494-2592): triplets of rows that
    other parts hold as ghosts are copied to the last such part in
    rows.exchanger.parts_snd order (local entry kept), unsent ghost rows'
    values become zero, received ones are appended in parts_rcv order."""
    ctxs = contexts(rows.partition)
    pids = rows.partition.part_ids
    idx = [device_index_gids(c, rows.partition.local(p)) for c, p in zip(ctxs, pids)]
    xg = [device_exchanger(c, rows.exchanger, p) for c, p in zip(ctxs, pids)]
    _lib.call(entry, len(ctxs), _hs(coo.values.parts), _hs(idx), _hs(xg))
    return coo


def assemble_(v, rows: PRange = None):
    """assemble!(v) (Interfaces.jl:2084-2106): ghost values added to their
    owners (reverse exchanger, `+`), then ghost values set to zero.  For a
    PSparseMatrix: assemble!(A) (2383-2404), the ghost rows' nonzeros added
    to the owners' and then zeroed.  For a COO and its rows:
    assemble!(I, J, V, rows) (2406-2492) on the device."""
    if isinstance(v, COO):
        if rows is None:
            raise TypeError("assemble!(I, J, V, rows): the rows PRange is required")
        return _coo_all("pa_coo_assemble_all", v, rows)
    if isinstance(v, PSparseMatrix):
        return _mat_exchange(v, _lib.PA_ADD, 1, 1)
    ctxs = contexts(v.values)
    xg = [device_exchanger(c, v.rows.exchanger, p) for c, p in zip(ctxs, v.values.part_ids)]
    _lib.call("pa_exchange_all", len(ctxs), _hs(v.values.parts), _hs(xg), _lib.ptr_array(_idx(v)),
              _lib.PA_ADD, 1, 1)
    return v


def _tasks(like: PData, ctxs, handles) -> PData:
    return PData(like.backend, like.part_ids, [Task(c, h) for c, h in zip(ctxs, handles)], like.shape)


def _async(v, rows, t0, coo_entry, op, reverse, zero):
    """The pa_*_exchange_all_async call behind async_exchange_ and
    async_assemble_: a PData of Tasks, one per part."""
    if isinstance(v, COO):
        # the COO forms size their outputs on the host: they have completed
        # when they return
        if rows is None:
            raise TypeError(f"{coo_entry}: the rows PRange is required")
        if t0 is not None:
            wait_all(t0)
        _coo_all(coo_entry, v, rows)
        ctxs = contexts(v.values)
        return _tasks(v.values, ctxs, [None] * len(ctxs))
    ctxs = contexts(v.values)
    n = len(ctxs)
    if t0 is not None and t0.part_ids != v.values.part_ids:
        raise ValueError("t0: tasks over different parts")
    after = _hs(t0.parts) if t0 is not None else None  # the Tasks of t0 stay alive through the call
    done = (C.c_void_p * n)()
    if isinstance(v, PSparseMatrix):
        _lib.call("pa_mat_exchange_all_async", n, _hs(v.values.parts), _hs(_mat_dev_xchg(v)), op, reverse, zero,
                  after, done)
    else:
        xg = [device_exchanger(c, v.rows.exchanger, p) for c, p in zip(ctxs, v.values.part_ids)]
        _lib.call("pa_exchange_all_async", n, _hs(v.values.parts), _hs(xg), _lib.ptr_array(_idx(v)), op, reverse,
                  zero, after, done)
    return _tasks(v.values, ctxs, [C.c_void_p(h) for h in done])


def async_exchange_(v, t0: PData = None, rows: PRange = None) -> PData:
    """t = async_exchange!(v) (Interfaces.jl:349-401, 2071-2075; a
    PSparseMatrix: 2375-2381): exchange_ that returns at once with a PData of
    Tasks.  Each part's work runs on its comm stream behind everything
    enqueued so far on the part and behind t0 (a PData of Tasks, e.g. of
    record or of another async call; no host wait); compute-stream work
    enqueued afterwards does not wait for it.  From the call until
    Task.wait() / Task.join() the values belong to the call.  A COO (with
    rows) runs the blocking call and returns finished tasks."""
    return _async(v, rows, t0, "pa_coo_exchange_all", _lib.PA_REPLACE, 0, 0)


def async_assemble_(v, t0: PData = None, rows: PRange = None) -> PData:
    """t = async_assemble!(v) (Interfaces.jl:2084-2106; a PSparseMatrix:
    2383-2404): assemble_ as async_exchange_ runs exchange_."""
    return _async(v, rows, t0, "pa_coo_assemble_all", _lib.PA_ADD, 1, 1)


def _table_args(values: PData, exchanger, combine, reverse, zero_sent):
    """the arguments pa_table_exchange_all and its async twin share"""
    if combine not in (None, "+"):
        raise ValueError("exchange!(Table): combine is None (replace) or '+'")
    tabs = values.parts
    if not all(isinstance(t, DeviceTable) for t in tabs):
        raise TypeError("exchange!(Table): values must be a PData of DeviceTable (DeviceTable.from_host)")
    if combine == "+" and any(t.dtype.kind in "iu" for t in tabs):
        raise TypeError("exchange!(+, Table): integer tables travel as bit patterns and cannot be added")
    ctxs = contexts(values)
    xg = [device_exchanger(c, exchanger, p) for c, p in zip(ctxs, values.part_ids)]
    op = _lib.PA_ADD if combine == "+" else _lib.PA_REPLACE
    return ctxs, (len(ctxs), _hs(tabs), _hs(xg), op, 1 if reverse else 0, 1 if zero_sent else 0)


def exchange_table_(values: PData, exchanger, combine=None, reverse=False, zero_sent=False) -> PData:
    """exchange!([combine_op,] values::AbstractPData{<:Table}, exchanger)
    (Interfaces.jl:891-961) over DeviceTables, rows of any length per lid: the
    exchanger derived from `exchanger` and each table's ptrs is built on the
    device on a table's first call and kept on the table.  combine None
    replaces, "+" adds (contributions in the reference's order); reverse uses
    reverse(exchanger); zero_sent zeroes the data of the rows that were sent
    afterwards.  A sender's row and its receiver's row must be equally long."""
    _, args = _table_args(values, exchanger, combine, reverse, zero_sent)
    _lib.call("pa_table_exchange_all", *args)
    return values


def async_exchange_table_(values: PData, exchanger, combine=None, reverse=False, zero_sent=False,
                          t0: PData = None) -> PData:
    """t = async_exchange!([combine_op,] values::AbstractPData{<:Table},
    exchanger, t0): exchange_table_ on the parts' comm streams, a PData of
    Tasks as async_exchange_ returns."""
    ctxs, args = _table_args(values, exchanger, combine, reverse, zero_sent)
    if t0 is not None and t0.part_ids != values.part_ids:
        raise ValueError("t0: tasks over different parts")
    after = _hs(t0.parts) if t0 is not None else None
    done = (C.c_void_p * len(ctxs))()
    _lib.call("pa_table_exchange_all_async", *args, after, done)
    return _tasks(values, ctxs, [C.c_void_p(h) for h in done])


def wait_all(tasks: PData):
    """wait on every task (map_parts(wait, t))"""
    for t in tasks.parts:
        t.wait()
    return tasks


def record(x) -> PData:
    """Tasks for everything enqueued so far on the parts of x (a PVector, a
    PSparseMatrix or a PData over the parts; pa_event_record), e.g. a mul_
    whose result an async_exchange_ takes as t0."""
    like = x if isinstance(x, PData) else x.values
    ctxs = contexts(like)
    hs = []
    for c in ctxs:
        h = C.c_void_p()
        _lib.call("pa_event_record", c.h, C.byref(h))
        hs.append(h)
    return _tasks(like, ctxs, hs)


def _scalar_out(dtype):
    return np.zeros(1, dtype=dtype)


def dot(a: PVector, b: PVector):
    """dot(a, b) (Interfaces.jl:1985-1992)"""
    out = _scalar_out(a.dtype)
    n = len(a.values.parts)
    _lib.call("pa_dot_all", n, _hs(a.values.parts), _lib.ptr_array(_idx(a)), _hs(b.values.parts),
              _lib.ptr_array(_idx(b)), out.ctypes.data_as(C.c_void_p))
    return out[0].item()


def norm(a: PVector, p=2):
    """norm(a, p) (Interfaces.jl:1767-1772): p = 2 (pa_norm2_all), and for
    real vectors p = 1 as sum(abs.(a)) and p = Inf as maximum(abs.(a))"""
    if p == 1 or p == math.inf:
        if np.dtype(a.dtype).kind == "c":
            raise NotImplementedError("norm(a, p) on HIP parts: p = 1 and p = Inf for real vectors only")
        return float(psum(abs(a))) if p == 1 else maximum(abs(a))
    if p != 2:
        raise NotImplementedError("norm(a, p) on HIP parts: p = 1, 2 or Inf")
    out = np.zeros(1, dtype=np.float64)
    _lib.call("pa_norm2_all", len(a.values.parts), _hs(a.values.parts), _lib.ptr_array(_idx(a)),
              out.ctypes.data_as(C.c_void_p))
    return float(out[0])


def psum(a):
    """sum(a) (Interfaces.jl:1981-1983); of a Broadcasted: the expression
    summed over the owned values in one pass (pa_reduce_expr_all)"""
    if isinstance(a, Broadcasted):
        return _reduce_expr(a, _lib.REDUCE_SUM)
    out = _scalar_out(a.dtype)
    _lib.call("pa_sum_all", len(a.values.parts), _hs(a.values.parts), _lib.ptr_array(_idx(a)),
              out.ctypes.data_as(C.c_void_p))
    return out[0].item()


# ---------------------------------------------------------------------------
# Broadcast expressions (Interfaces.jl:1688-1765) and mapped reductions
# (1682-1686, 1767-1863): a lazy tree over PVectors and numbers, encoded into
# the postfix program of include/pa_hip.h and evaluated in one pass per part.

_BINARY = {"add": _lib.OP_ADD, "sub": _lib.OP_SUB, "mul": _lib.OP_MUL, "div": _lib.OP_DIV, "lt": _lib.OP_LT,
           "le": _lib.OP_LE, "gt": _lib.OP_GT, "ge": _lib.OP_GE, "eq": _lib.OP_EQ, "ne": _lib.OP_NE}
_UNARY = {"neg": _lib.OP_NEG, "abs": _lib.OP_ABS, "abs2": _lib.OP_ABS2, "conj": _lib.OP_CONJ}
_COMPARE = ("lt", "le", "gt", "ge", "eq", "ne")
_NUMBER = (int, float, complex, np.number)


def _expr_scalar(a, dtype):
    """(value, kind) of a scalar operand: kind 0 the element type, 1 Float64,
    2 ComplexF64 (_scalar_kind's rule); over complex vectors a real scalar of
    the element type's width (an int, a Float32 next to ComplexF32) is kind 3,
    a value of real(T), so that Julia's Real ∘ Complex methods apply"""
    cplx = np.dtype(dtype).kind == "c"
    if not cplx and np.iscomplexobj(a) and complex(a).imag != 0:
        raise TypeError("broadcast: a complex scalar into a real vector (InexactError)")
    v, k = _scalar_kind(a, dtype)
    if k == 0 and cplx and not np.iscomplexobj(a):
        return np.zeros(1, dtype).real.dtype.type(a), 3
    if k == 0:
        v = np.dtype(dtype).type(complex(a).real if (np.iscomplexobj(a) and not cplx) else a)
    return v, k >> 3


class Broadcasted(_ExprOps):
    """A lazy broadcast node (DistributedBroadcasted, Interfaces.jl:1688-1692):
    `op` over PVector / Broadcasted / number operands.  `rows` is the first
    vector operand's PRange; `ghosts` says whether ghost values are computed
    too — only when every PVector operand shares one rows object (1730).
    `wide` / `real`: the node is of the wide type (an operand is a Float64 /
    ComplexF64 scalar or a wide node) / real valued over complex vectors."""

    def __init__(self, op, *args, check=True):
        if op not in _BINARY and op not in _UNARY and op != "identity":
            raise TypeError(f"broadcast: unsupported function {op}")
        if len(args) != (2 if op in _BINARY else 1):
            raise TypeError(f"broadcast: {op} takes {2 if op in _BINARY else 1} operand(s)")
        vecs = [a for a in args if isinstance(a, (PVector, Broadcasted))]
        if not vecs:
            raise TypeError("broadcast: no PVector operand")
        for a in args:
            if not isinstance(a, (PVector, Broadcasted) + _NUMBER):
                raise TypeError(f"broadcast: unsupported operand {type(a).__name__}")
        self.op, self.args = op, args
        self.rows = vecs[0].rows
        self.dtype = np.dtype(vecs[0].dtype)
        for a in vecs[1:]:
            if np.dtype(a.dtype) != self.dtype:
                raise TypeError(f"broadcast: mixed element types {self.dtype} and {np.dtype(a.dtype)}")
            if check and not oids_are_equal(a.rows, self.rows):
                raise AssertionError("broadcast: owned ids differ")
        self.ghosts = all(a.rows is self.rows and (a.ghosts if isinstance(a, Broadcasted) else True) for a in vecs)
        cplx = self.dtype.kind == "c"
        t = [_operand_type(a, self.dtype) for a in args]  # (wide, real) per operand
        real = [r or not cplx for _, r in t]
        # a comparison's 1 / 0 is of the element type (Julia's Bool takes the other operand's type)
        self.wide = any(w for w, _ in t) and op not in _COMPARE
        if op in ("div", "abs") and not all(real):
            raise TypeError(f"broadcast: {op} of complex values is not supported")
        if op in ("lt", "le", "gt", "ge") and not all(real):
            raise TypeError("broadcast: ordered comparison of complex values")
        self.real = cplx and (op in _COMPARE or op in ("abs", "abs2") or all(real))


def _operand_type(a, dtype):
    if isinstance(a, Broadcasted):
        return a.wide, a.real
    if isinstance(a, PVector):
        return False, False
    k = _expr_scalar(a, dtype)[1]
    return k in (1, 2), k in (1, 3) and np.dtype(dtype).kind == "c"


def _node(op, *args):
    if not all(isinstance(a, (PVector, Broadcasted) + _NUMBER) for a in args):
        return NotImplemented
    return Broadcasted(op, *args)


def abs2(a):
    """abs2.(a)"""
    return Broadcasted("abs2", a)


def conj(a):
    """conj.(a)"""
    return Broadcasted("conj", a)


def eq(a, b):
    """a .== b (1 / 0 of the node's type)"""
    return Broadcasted("eq", a, b)


def ne(a, b):
    """a .!= b"""
    return Broadcasted("ne", a, b)


class ExprProgram:
    """The encoded form of an expression: `vecs` (the distinct PVector
    operands), `scalars` ((value, kind) pairs; kinds as pa_hip.h's scalar_kinds), `ops` ((code, arg, flags)
    triples in postfix order), the stack `depth` it needs and the root's
    `wide` / `real`."""

    def __init__(self, dtype):
        self.dtype = np.dtype(dtype)
        self.vecs, self.scalars, self.ops = [], [], []
        self.depth = 0
        self.wide = self.real = False

    def c_args(self):
        """(pa_expr, nscal, scalar slots, scalar kinds) for the C-ABI"""
        e = _lib.Expr()
        e.nops = len(self.ops)
        for i, (code, arg, flags) in enumerate(self.ops):
            e.ops[i] = _lib.ExprOp(code, arg, flags, 0)
        ns = len(self.scalars)
        buf = bytearray(16 * max(ns, 1))
        for k, (v, kind) in enumerate(self.scalars):
            b = np.array([v], dtype=(self.dtype, np.float64, np.complex128, np.asarray(v).dtype)[kind]).tobytes()
            buf[16 * k:16 * k + len(b)] = b
        return e, ns, (C.c_char * len(buf)).from_buffer(buf), (C.c_int * max(ns, 1))(*[k for _, k in self.scalars])


def encode_expr(root) -> ExprProgram:
    """Postfix program of a Broadcasted (or a PVector: the identity).  Sibling
    subtrees are pure, so the one that needs more stack slots is emitted first
    (the reversed operand mode keeps left ∘ right), which keeps the depth at
    the tree's minimum; scalars ride as immediates of their binary op."""
    P = ExprProgram(root.dtype)
    cplx = P.dtype.kind == "c"
    need_memo = {}

    def need(a):  # stack slots the subtree needs
        if isinstance(a, PVector):
            return 1
        if not isinstance(a, Broadcasted):
            return 0
        if id(a) not in need_memo:
            n = [need(x) for x in a.args]
            if len(n) == 1 or 0 in n:
                need_memo[id(a)] = max(max(n), 1)
            else:
                need_memo[id(a)] = max(n[0], n[1] + 1) if n[0] >= n[1] else max(n[1], n[0] + 1)
        return need_memo[id(a)]

    def scalar(a):
        v, kind = _expr_scalar(a, P.dtype)
        key = (kind, np.asarray(v).tobytes())
        for k, (w, kd) in enumerate(P.scalars):
            if (kd, np.asarray(w).tobytes()) == key:
                return k
        P.scalars.append((v, kind))
        return len(P.scalars) - 1

    def tags(a):  # PA_EXPR_WIDE | PA_EXPR_LREAL of an operand
        w, r = _operand_type(a, P.dtype)
        return (_lib.EXPR_WIDE if w else 0) | (_lib.EXPR_LREAL if (r and cplx) else 0)

    sp = [0]

    def push(code, arg, flags):
        P.ops.append((code, arg, flags))
        sp[0] += 1
        P.depth = max(P.depth, sp[0])

    def emit(a):
        if isinstance(a, PVector):
            for k, v in enumerate(P.vecs):
                if v is a:
                    break
            else:
                P.vecs.append(a)
                k = len(P.vecs) - 1
            return push(_lib.OP_VEC, k, 0)
        if not isinstance(a, Broadcasted):  # a lone scalar
            return push(_lib.OP_SCAL, scalar(a), tags(a))
        if a.op == "identity":
            return emit(a.args[0])
        if a.op in _UNARY:
            emit(a.args[0])
            return P.ops.append((_UNARY[a.op], 0, tags(a.args[0])))
        l, r = a.args
        tl, tr = tags(l), tags(r)
        fl = ((tl | tr) & _lib.EXPR_WIDE) | (tl & _lib.EXPR_LREAL) | (_lib.EXPR_RREAL if tr & _lib.EXPR_LREAL else 0)
        code = _BINARY[a.op]
        if not isinstance(r, (PVector, Broadcasted)):
            emit(l)
            return P.ops.append((code, scalar(r), fl | _lib.EXPR_SC))
        if not isinstance(l, (PVector, Broadcasted)):
            emit(r)
            return P.ops.append((code, scalar(l), fl | _lib.EXPR_CS))
        if need(l) >= need(r):
            emit(l)
            emit(r)
            mode = _lib.EXPR_SS
        else:
            emit(r)
            emit(l)
            mode = _lib.EXPR_RS
        sp[0] -= 1
        P.ops.append((code, 0, fl | mode))

    emit(root)
    if isinstance(root, Broadcasted):
        P.wide, P.real = root.wide, root.real
    if len(P.ops) > _lib.EXPR_MAX_OPS:
        raise TypeError(f"broadcast: the expression needs {len(P.ops)} ops, more than {_lib.EXPR_MAX_OPS}")
    if P.depth > _lib.EXPR_MAX_DEPTH:
        raise TypeError(f"broadcast: the expression needs {P.depth} stack slots, more than {_lib.EXPR_MAX_DEPTH}")
    if len(P.vecs) > _lib.EXPR_MAX_VECS:
        raise TypeError(f"broadcast: more than {_lib.EXPR_MAX_VECS} vector operands")
    if len(P.scalars) > _lib.EXPR_MAX_SCALARS:
        raise TypeError(f"broadcast: more than {_lib.EXPR_MAX_SCALARS} scalars")
    return P


def _as_expr(x):
    if isinstance(x, Broadcasted):
        return x
    if isinstance(x, PVector):
        return Broadcasted("identity", x)
    raise TypeError(f"expected a PVector or a broadcast expression, got {type(x).__name__}")


def assign_(w: PVector, expr) -> PVector:
    """w .= expr (materialize!, Interfaces.jl:1710-1720): all lids when every
    PVector operand and w share one rows object, else the owned values (w's
    ghosts untouched).  w may be an operand."""
    expr = _as_expr(expr)
    if np.dtype(w.dtype) != expr.dtype:
        raise TypeError(f"broadcast: mixed element types {np.dtype(w.dtype)} and {expr.dtype}")
    all_lids = 1 if (expr.ghosts and w.rows is expr.rows) else 0
    if not all_lids and not oids_are_equal(w.rows, expr.rows):
        raise AssertionError("broadcast: owned ids differ")
    P = encode_expr(expr)
    e, ns, sbuf, kinds = P.c_args()
    iy = _idx(w)
    iv = [_idx(v) for v in P.vecs]
    for p, dy in enumerate(w.values.parts):
        _lib.call("pa_vec_eval", dy.h, iy[p], C.byref(e), len(P.vecs),
                  _lib.ptr_array([v.values.parts[p].h for v in P.vecs]), _lib.ptr_array([i[p] for i in iv]),
                  ns, sbuf, kinds, all_lids)
    return w


def materialize(expr) -> PVector:
    """materialize(bc) (Interfaces.jl:1694-1708): a new PVector on the first
    operand's rows (ghosts computed when every operand shares them)"""
    expr = _as_expr(expr)
    return assign_(PVector.undef(expr.rows, expr.dtype), expr)


def _reduce_expr(x, kind):
    expr = _as_expr(x)
    P = encode_expr(expr)
    e, ns, sbuf, kinds = P.c_args()
    n = len(P.vecs[0].values.parts)
    iv = [_idx(v) for v in P.vecs]
    vh = _lib.ptr_array([v.values.parts[p].h for p in range(n) for v in P.vecs])
    ih = _lib.ptr_array([i[p] for p in range(n) for i in iv])
    out = np.zeros(1, dtype=P.dtype if kind == _lib.REDUCE_SUM else np.float64)
    _lib.call("pa_reduce_expr_all", n, kind, C.byref(e), len(P.vecs), vh, ih, ns, sbuf, kinds,
              out.ctypes.data_as(C.c_void_p))
    r = out[0].item()
    return r.real if (isinstance(r, complex) and P.real) else r


def _real_valued(x, what):
    x = _as_expr(x)
    if x.dtype.kind == "c" and not x.real:
        raise TypeError(f"{what} of a complex-valued expression")
    return x


def maximum(x) -> float:
    """maximum(x) / maximum(f, v) as maximum(f(v)) (Interfaces.jl:1841-1851):
    over the owned values, init -Inf, NaN if any owned element is NaN"""
    return _reduce_expr(_real_valued(x, "maximum"), _lib.REDUCE_MAX)


def minimum(x) -> float:
    """minimum(x) / minimum(f, v) (Interfaces.jl:1853-1863), init +Inf"""
    return _reduce_expr(_real_valued(x, "minimum"), _lib.REDUCE_MIN)


def _predicate(x, what):
    if not (isinstance(x, Broadcasted) and x.op in _COMPARE):
        raise TypeError(f"{what}: expected a comparison (v < c, eq(a, b), ...)")
    return x


def any_(expr) -> bool:
    """any(f, v) with f a comparison (Interfaces.jl:1827-1832)"""
    return maximum(_predicate(expr, "any")) > 0


def all_(expr) -> bool:
    """all(f, v) with f a comparison (Interfaces.jl:1834-1839)"""
    return minimum(_predicate(expr, "all")) > 0


def isequal(a: PVector, b: PVector) -> bool:
    """a == b (Interfaces.jl:1682-1686): equal lengths, parts and owned values"""
    if len(a) != len(b) or a.values.num_parts != b.values.num_parts:
        return False
    if np.dtype(a.dtype) != np.dtype(b.dtype):
        raise TypeError(f"broadcast: mixed element types {np.dtype(a.dtype)} and {np.dtype(b.dtype)}")
    if any(s.num_oids != t.num_oids for s, t in zip(a.rows.partition.parts, b.rows.partition.parts)):
        return False
    return all_(Broadcasted("eq", a, b, check=False))


def sqeuclidean(a: PVector, b: PVector):
    """Distances.SqEuclidean()(a, b) (Interfaces.jl:1774-1817): Σ |a - b|²"""
    return psum(abs2(a - b))


def euclidean(a: PVector, b: PVector) -> float:
    """Distances.Euclidean()(a, b): sqrt of sqeuclidean"""
    return math.sqrt(sqeuclidean(a, b))


# ---------------------------------------------------------------------------
# PSparseMatrix

class PSparseMatrix:
    """PSparseMatrix(values, rows, cols) (Interfaces.jl:2108-2125): values =
    PData of DeviceMatrix (owned rows in the SELL layout)."""

    def __init__(self, values: PData, rows: PRange, cols: PRange, exchanger=None):
        self.values = values
        self.rows = rows
        self.cols = cols
        # matrix_exchanger(values, rows, cols) (Interfaces.jl:2117): nz ids
        self.exchanger = exchanger if exchanger is not None else empty_exchanger(rows.partition)
        self._dev_xchg = None

    @property
    def dtype(self):
        return self.values.parts[0].dtype

    @property
    def shape(self):
        return (len(self.rows), len(self.cols))

    @staticmethod
    def from_csc(csc: PData, rows: PRange, cols: PRange) -> "PSparseMatrix":
        """From each part's local SparseMatrixCSC (num_lids(rows) × num_lids(cols))."""
        ctxs = contexts(rows.partition)
        mats = []
        for c, A, r, s in zip(ctxs, csc.parts, rows.partition.parts, cols.partition.parts):
            mats.append(DeviceMatrix.from_csc(c, A, device_index(c, r), device_index(c, s),
                                              r.num_lids, s.num_lids))
        ex = matrix_exchanger(csc, rows, cols)
        return PSparseMatrix(PData(rows.partition.backend, rows.partition.part_ids, mats,
                                   rows.partition.shape), rows, cols, ex)

    @staticmethod
    def from_csr(csr: PData, rows: PRange, cols: PRange) -> "PSparseMatrix":
        """From each part's local SparseMatrixCSR{Bi} (num_lids(rows) ×
        num_lids(cols)); mul! then follows SparseUtils.jl:222-252."""
        ctxs = contexts(rows.partition)
        mats = []
        for c, A, r, s in zip(ctxs, csr.parts, rows.partition.parts, cols.partition.parts):
            mats.append(DeviceMatrix.from_csr(c, A, device_index(c, r), device_index(c, s),
                                              r.num_lids, s.num_lids))
        ex = matrix_exchanger(csr, rows, cols)
        return PSparseMatrix(PData(rows.partition.backend, rows.partition.part_ids, mats,
                                   rows.partition.shape), rows, cols, ex)

    @staticmethod
    def from_coo(I, J, V, rows: PRange, cols: PRange, ids="local", init=None, exchanger=None):
        """PSparseMatrix(init, I, J, V, rows, cols; ids) (Interfaces.jl:
        2194-2215; `exchanger`: the matrix exchanger the caller supplies, as
        gather(A) passes an empty one, 2699-2702 — device compress only).  init None = sparse (2237-2244), on the device; I, J, V:
        PData of host arrays, or I a device COO (then J and V are None).
        init = csr_init(Bi) (sparsecsr): the same compress on the device into
        SparseMatrixCSR{Bi} parents (pa_mat_from_coo_csr).  Another callable
        init compresses each part's host triplets and uploads the result
        (pa_mat_from_csc / pa_mat_from_csr)."""
        if isinstance(init, csr_init):  # sparsecsr on the device
            return PSparseMatrix._from_coo_device(I, J, V, rows, cols, ids, csr_bi=init.Bi, exchanger=exchanger)
        if init is not None:
            if exchanger is not None:
                raise NotImplementedError("from_coo: a custom init builds its own matrix exchanger")
            if isinstance(I, COO):
                raise NotImplementedError("from_coo: a custom init needs host triplets")
            if ids == "global":
                I = map_parts(lambda i, r: r.to_lids(np.asarray(i, dtype=np.int64)), I, rows.partition)
                J = map_parts(lambda j, c: c.to_lids(np.asarray(j, dtype=np.int64)), J, cols.partition)
            loc = map_parts(lambda i, j, v, r, c: init(i, j, v, r.num_lids, c.num_lids), I, J, V,
                            rows.partition, cols.partition)
            if all(isinstance(m, CSR) for m in loc.parts):
                return PSparseMatrix.from_csr(loc, rows, cols)
            if all(isinstance(m, CSC) for m in loc.parts):
                return PSparseMatrix.from_csc(loc, rows, cols)
            raise TypeError("from_coo: init must return CSC or CSR local matrices")
        return PSparseMatrix._from_coo_device(I, J, V, rows, cols, ids, exchanger=exchanger)

    @staticmethod
    def _from_coo_device(I, J, V, rows: PRange, cols: PRange, ids="local", csr_bi=None, exchanger=None):
        # to_lids! (ids=:global) and sparse(I, J, V) (or sparsecsr) on the
        # device (pa_mat_from_coo[_csr]); the host keeps the pattern only, for
        # matrix_exchanger
        glob = ids == "global"
        idx = device_index_gids if glob else device_index
        ctxs = contexts(rows.partition)
        dev = isinstance(I, COO)  # device triplets: from_coo(coo, None, None, rows, cols; ids)
        if dev:
            I, J, V = I.values, I.values, I.values
        mats, pats = [], []
        # the host needs the CSC pattern only for matrix_exchanger, i.e. when
        # rows have ghosts (stored ghost rows of FE assembly)
        want_pattern = bool(rows.ghost) and exchanger is None
        trace = trace_setup()
        t0 = trace()
        for c, i, j, v, r, s in zip(ctxs, I.parts, J.parts, V.parts, rows.partition.parts, cols.partition.parts):
            if dev:
                M, colptr, rowval = DeviceMatrix.from_dcoo(i, idx(c, r), idx(c, s), r.num_lids, s.num_lids,
                                                           ids_global=glob, pattern=want_pattern, csr_bi=csr_bi)
            else:
                M, colptr, rowval = DeviceMatrix.from_coo(c, i, j, v, idx(c, r), idx(c, s), r.num_lids,
                                                          s.num_lids, ids_global=glob, pattern=want_pattern,
                                                          csr_bi=csr_bi)
            mats.append(M)
            if not want_pattern:
                pats.append(None)
            elif csr_bi is None:
                pats.append(CSC(r.num_lids, s.num_lids, colptr, rowval, np.zeros(0)))
            else:
                pats.append(CSR(csr_bi, r.num_lids, s.num_lids, colptr, rowval, np.zeros(0)))
        t1 = trace("device sparse + SELL, all parts", t0)
        backend, pids, shape = rows.partition.backend, rows.partition.part_ids, rows.partition.shape
        ex = (matrix_exchanger(PData(backend, pids, pats, shape), rows, cols) if want_pattern
              else exchanger if exchanger is not None else empty_exchanger(rows.partition))
        trace("matrix_exchanger", t1)
        return PSparseMatrix(PData(backend, pids, mats, shape), rows, cols, ex)

    def info(self):
        return map_parts(lambda m: m.info(), self.values)


def fillstored_(a: "PSparseMatrix", v) -> "PSparseMatrix":
    """LinearAlgebra.fillstored!(a, v) (Interfaces.jl:2127-2132): every
    stored value of every part becomes v (on the device)."""
    for M in a.values.parts:
        M.fillstored(v)
    return a


def matrix_exchanger(values: PData, rows: PRange, cols: PRange) -> Exchanger:
    """matrix_exchanger(values, rows, cols) (Interfaces.jl:2300-2372),
    vectorised: the nonzeros of ghost rows (CSC order k) grouped by the row
    owner in rows.exchanger.parts_rcv order; their (gi, gj) are sent to the
    owner, which answers with nzindex of (gi, gj) in its local matrix."""
    if not rows.ghost:
        return empty_exchanger(rows.partition)
    parts_rcv = rows.exchanger.parts_rcv
    parts_snd = rows.exchanger.parts_snd

    def nz_lids(A):
        """0-based (row, col) lids of the nonzeros in storage order
        (nziterator, SparseUtils.jl:106-150 for CSC, 254-300 for CSR)"""
        if isinstance(A, CSR):
            return np.repeat(np.arange(A.m), np.diff(A.rowptr)), A.colval - A.Bi
        return A.rowval - 1, np.repeat(np.arange(A.n), np.diff(A.colptr))

    def setup_rcv(prcv, r, c, A):
        prcv = np.asarray(prcv, dtype=np.int64)
        li, lj = nz_lids(A)
        owner = r.lid_to_part[li].astype(np.int64)
        k = np.flatnonzero(owner != r.part)
        seg = np.searchsorted(prcv, owner[k])
        if len(k) and (seg.max() >= len(prcv) or not np.array_equal(prcv[seg], owner[k])):
            raise KeyError("matrix_exchanger: a ghost row's owner is not in parts_rcv")
        o = np.argsort(seg, kind="stable")
        k = k[o]
        ptrs = counts_to_ptrs(np.bincount(seg, minlength=len(prcv)))
        gi = r.lid_to_gid[li[k]]
        gj = c.lid_to_gid[lj[k]]
        return (Table((k + 1).astype(np.int64), ptrs), Table(gi, ptrs.copy()), Table(gj, ptrs.copy()))
    k_rcv, gi_rcv, gj_rcv = unzip(map_parts(setup_rcv, parts_rcv, rows.partition, cols.partition, values), 3)
    segs = lambda t: [t[i] for i in range(1, len(t) + 1)]
    gi_snd = exchange(map_parts(segs, gi_rcv), parts_snd, parts_rcv)
    gj_snd = exchange(map_parts(segs, gj_rcv), parts_snd, parts_rcv)

    def setup_snd(r, c, gi, gj, A):
        ptrs = counts_to_ptrs([len(x) for x in gi])
        gi = np.concatenate(gi).astype(np.int64) if gi else np.zeros(0, np.int64)
        gj = np.concatenate(gj).astype(np.int64) if gj else np.zeros(0, np.int64)
        li = r.to_lids(gi) - 1
        lj = c.to_lids(gj) - 1
        # nzindex(A, li, lj): CSC order is sorted by (col, row) (SparseUtils.jl:
        # 96-104), CSR order by (row, col) (210-220)
        ri, rj = nz_lids(A)
        if isinstance(A, CSR):
            key, q = ri.astype(np.int64) * A.n + rj, li * A.n + lj
        else:
            key, q = rj.astype(np.int64) * A.m + ri, lj * A.m + li
        pos = np.searchsorted(key, q)
        ok = (pos < len(key)) & (key[np.minimum(pos, max(len(key) - 1, 0))] == q) if len(key) else pos < 0
        if not np.all(ok):
            raise AssertionError("The sparsity pattern of the ghost layer is inconsistent")
        return Table((pos + 1).astype(np.int64), ptrs)
    k_snd = map_parts(setup_snd, rows.partition, cols.partition, gi_snd, gj_snd, values)
    return Exchanger(parts_rcv, parts_snd, k_rcv, k_snd)


def _mat_dev_xchg(A: "PSparseMatrix"):
    """the device exchangers over nonzeros(A), created on first use"""
    if A._dev_xchg is None:
        ex = A.exchanger
        A._dev_xchg = [DeviceMatrixExchanger(M, ex.parts_rcv.local(p), ex.lids_rcv.local(p),
                                             ex.parts_snd.local(p), ex.lids_snd.local(p))
                       for M, p in zip(A.values.parts, A.values.part_ids)]
    return A._dev_xchg


def _mat_exchange(A: "PSparseMatrix", op, reverse, zero_sent):
    xg = _mat_dev_xchg(A)
    _lib.call("pa_mat_exchange_all", len(xg), _hs(A.values.parts), _hs(xg), op, reverse, zero_sent)
    return A


def mul_(c: PVector, a: PSparseMatrix, b: PVector, alpha=1.0, beta=0.0) -> PVector:
    """mul!(c, a, b, α, β) (Interfaces.jl:2246-2275): halo exchange of b
    overlapped with the interior slices, then the slices reading ghosts."""
    _spmv(c, a, b, alpha, beta, None)
    return c


def mul_dot_(c: PVector, a: PSparseMatrix, b: PVector, alpha=1.0, beta=0.0):
    """mul!(c, a, b, α, β) then dot(b, c), the dot accumulated by the SpMV
    kernel (pa_spmv_dot_all).  Returns the dot."""
    out = _scalar_out(a.dtype)
    _spmv(c, a, b, alpha, beta, out)
    return out[0].item()


def _spmv(c, a, b, alpha, beta, dot_out):
    args = _spmv_args(c, a, b, alpha, beta)
    if dot_out is None:
        _lib.call("pa_spmv_all", *args)
    else:
        _lib.call("pa_spmv_dot_all", *args, dot_out.ctypes.data_as(C.c_void_p))


_ARGS_CACHE_MAX = 8


def _spmv_args(c, a, b, alpha, beta):
    """The C-ABI arguments of mul!(c, a, b, α, β), cached on `a` per (c, b,
    α, β): the layout checks and the handle arrays are built on the first
    call only (the Python side of a mul! costs about as much as a small
    SpMV's kernels otherwise).  An entry is reused only while c and b are the
    same live objects with the same values and ranges (the entry holds no
    strong reference to them: their device memory is freed as usual)."""
    cache = a.__dict__.get("_args_cache")
    if cache is None:
        cache = a.__dict__["_args_cache"] = OrderedDict()
    key = (id(c), id(b), type(alpha), alpha, type(beta), beta)
    try:
        e = cache.get(key)
    except TypeError:  # unhashable scalars (0-d arrays): no caching
        return _spmv_args_build(c, a, b, alpha, beta)
    now = (id(c.values), id(b.values), id(c.rows), id(b.rows))
    if e is not None and e[0]() is c and e[1]() is b and e[2] == now:
        cache.move_to_end(key)
        return e[3]
    args = _spmv_args_build(c, a, b, alpha, beta)
    cache[key] = (weakref.ref(c), weakref.ref(b), now, args)
    while len(cache) > _ARGS_CACHE_MAX:
        cache.popitem(last=False)
    return args


def _spmv_args_build(c, a, b, alpha, beta):
    if not (c.rows is a.rows or oids_are_equal(c.rows, a.rows)):
        raise AssertionError("mul!: c.rows and a.rows own different ids")
    if not (b.rows is a.cols or (oids_are_equal(a.cols, b.rows) and hids_are_equal(a.cols, b.rows))):
        raise AssertionError("mul!: b.rows differs from a.cols")
    if b.rows is not a.cols and not _cached_eq(
            "layout", a.cols, b.rows,
            lambda s, t: bool(np.array_equal(s.oid_to_lid, t.oid_to_lid) and np.array_equal(s.hid_to_lid, t.hid_to_lid))):
        raise NotImplementedError("mul!: b.rows must have a.cols' local layout")
    ctxs = contexts(a.values)
    n = len(ctxs)
    ex = b.rows.exchanger
    has_x = any(len(ex.parts_rcv.local(p)) or len(ex.parts_snd.local(p)) for p in b.values.part_ids)
    xg = [device_exchanger(cx, ex, p) for cx, p in zip(ctxs, b.values.part_ids)] if has_x else None
    al, alp = _lib.scalar_buf(alpha, a.dtype)
    be, bep = _lib.scalar_buf(beta, a.dtype)
    # the scalar buffers ride along (the C side reads them during the call)
    return (n, _hs(a.values.parts), _hs(c.values.parts), _lib.ptr_array(_idx(c)),
            _hs(b.values.parts), _lib.ptr_array(_idx(b)), _hs(xg) if xg else None, alp, bep)


def cg_update_(x: PVector, r: PVector, u: PVector, c: PVector, alpha) -> float:
    """x .+= α.*u; r .-= α.*c; norm(r) in one pass (pa_cg_update_all); α is
    a Float64 (ComplexF64 for complex vectors) as in IterativeSolvers."""
    if not (x.rows is r.rows is u.rows is c.rows):
        raise ValueError("cg_update_: the four vectors must share one PRange")
    al, alp = _lib.scalar_buf(alpha, np.complex128 if np.dtype(x.dtype).kind == "c" else np.float64)
    out = C.c_double(0.0)
    _lib.call("pa_cg_update_all", len(x.values.parts), _hs(x.values.parts), _hs(r.values.parts),
              _hs(u.values.parts), _hs(c.values.parts), _lib.ptr_array(_idx(x)), alp, C.byref(out))
    return out.value


def _julia_inv(w: complex) -> complex:
    """Julia's inv(::ComplexF64) (base/complex.jl, scaled Smith): Float64 /
    ComplexF64 is a * inv(z) componentwise (Julia Base arithmetic, restated;
    the device CG's julia_inv is the same)."""
    c, d = w.real, w.imag
    if math.isinf(c) or math.isinf(d):
        return complex(math.copysign(0.0, c), 0.0 if math.copysign(1.0, d) < 0 else -0.0)
    half, two = 0.5, 2.0
    cd = max(abs(c), abs(d))
    ov, un, eps = sys.float_info.max, sys.float_info.min, sys.float_info.epsilon
    bs = two / (eps * eps)
    s = 1.0
    if cd >= half * ov:
        c, d, s = half * c, half * d, s * half
    if cd <= un * two / eps:
        c, d, s = c * bs, d * bs, s * bs
    if abs(d) <= abs(c):
        r = d / c
        t = 1.0 / (c + d * r)
        p, q = t, -r * t
    else:
        c, d = d, c
        r = d / c
        t = 1.0 / (c + d * r)
        p, q = r * t, -t
    return complex(p * s, q * s)


def _rdiv(a: float, z):
    """a::Float64 / z::T (Julia: Float64 for real T, a*inv(ComplexF64(z)) for complex)"""
    if isinstance(z, complex):
        w = _julia_inv(z)
        return complex(a * w.real, a * w.imag)
    return a / float(z)


def matvec(a: PSparseMatrix, b: PVector) -> PVector:
    """Base.:*(a, b) (Interfaces.jl:2605-2610)"""
    c = PVector.undef(a.rows, a.dtype)
    return mul_(c, a, b)


def _own_contig(v: PVector) -> bool:
    return all(s.num_oids == 0 or (s.oid_to_lid[0] == 1 and s.oid_to_lid[-1] == s.num_oids)
               for s in v.rows.partition.parts)


def cg_(x: PVector, A: PSparseMatrix, b: PVector, reltol=None, abstol=0.0, maxiter=None,
        history=None, fused=True, device=False, batch=8, Pl=None):
    """IterativeSolvers.cg! (v0.9; caller of the hot path at test_fdm.jl:115,
    test_fem_sa.jl:135), restated over the device operations:
    u = zero(x); r, c = similar(x); copyto!(r, b); mul!(c, A, x); r .-= c;
    residual = norm(r); tol = max(reltol*norm(b), abstol); prev = 1; then per
    iteration β = res²/prev²; u .= r .+ β.*u; mul!(c, A, u);
    α = res²/dot(u, c); x .+= α.*u; r .-= α.*c; prev = res; res = norm(r).

    device=True runs the same recurrence with its scalars on the device
    (pa_cg_solve_all): the host enqueues `batch` iterations between reads of
    the done flag; results equal the host-driven fused loop bit for bit.

    Pl: a left preconditioner (Jacobi); the preconditioned iterate then runs
    (_pcg), host-driven, Float32 / Float64 (cg_device_ runs it with its
    scalars on the device).  Pl=None is the loop above."""
    real = np.float32 if x.dtype in (np.float32, np.complex64) else np.float64
    if reltol is None:  # sqrt(eps(real(eltype(b)))), in that type
        reltol = float(np.sqrt(np.finfo(real).eps))
    if maxiter is None:
        maxiter = len(A.cols)
    if Pl is not None:
        if device:
            raise NotImplementedError("cg_(Pl=..., device=True): cg_ drives the preconditioned recurrence from the "
                                      "host; cg_device_(x, A, b, Pl=...) runs it with its scalars on the device")
        return _pcg(x, A, b, Pl, reltol, abstol, maxiter, history, fused)
    if device:
        return _cg_device(x, A, b, reltol, abstol, maxiter, history, batch)
    u = x.similar().fill_(0)
    r = x.similar()
    c = x.similar()
    copyto_(r, b)
    mul_(c, A, x)
    sub_(r, c)
    residual = norm(r)
    tol = max(reltol * norm(b), abstol)
    prev = 1.0
    it = 0
    # fusions (same arithmetic per element; reduction orders are this
    # library's deterministic ones): dot(u,c) inside the SpMV, and
    # x/r updates + norm(r) in one pass
    fuse = fused and _own_contig(u) and (x.rows is r.rows is u.rows is c.rows)
    while not (it >= maxiter or residual <= tol):
        beta = (residual * residual) / (prev * prev)  # residual^2 (literal_pow: x*x)
        xpby_(u, r, beta)
        if fuse:
            alpha = _rdiv(residual * residual, mul_dot_(c, A, u))
            new = cg_update_(x, r, u, c, alpha)
        else:
            mul_(c, A, u)
            alpha = _rdiv(residual * residual, dot(u, c))
            axpy_(x, alpha, u)
            axmy_(r, alpha, c)
            new = norm(r)
        prev = residual
        residual = new
        it += 1
        if history is not None:
            history.append(residual)
    return x


def _cg_device(x: PVector, A: PSparseMatrix, b: PVector, reltol, abstol, maxiter, history, batch):
    if not _own_contig(x):
        raise ValueError("cg_(device=True): x needs contiguous owned lids")
    if b.rows is not x.rows:  # copyto!(r, b) across partitions copies the owned values
        bb = x.similar()
        copyto_(bb, b)
        b = bb
    u, r, c = x.similar(), x.similar(), x.similar()
    ctxs = contexts(A.values)
    n = len(ctxs)
    ex = x.rows.exchanger
    has_x = any(len(ex.parts_rcv.local(p)) or len(ex.parts_snd.local(p)) for p in x.values.part_ids)
    xg = [device_exchanger(cx, ex, p) for cx, p in zip(ctxs, x.values.part_ids)] if has_x else None
    its = C.c_int64(0)
    res = C.c_double(0.0)
    hist = np.zeros(max(1, int(maxiter)), dtype=np.float64) if history is not None else None
    _lib.call("pa_cg_solve_all", n, _hs(A.values.parts), _hs(x.values.parts), _hs(b.values.parts),
              _hs(u.values.parts), _hs(r.values.parts), _hs(c.values.parts), _lib.ptr_array(_idx(x)),
              _hs(xg) if xg else None, float(reltol), float(abstol), int(maxiter), int(batch),
              C.byref(its), C.byref(res),
              hist.ctypes.data_as(C.POINTER(C.c_double)) if hist is not None else None)
    if history is not None:
        history.extend(float(v) for v in hist[:its.value])
    return x


# ---------------------------------------------------------------------------
# Jacobi-preconditioned CG: diag(A) read off the device
# layout, Pl \ r fused with ρ = dot(c, r), and the x / r updates fused with
# the next iteration's Pl \ r, norm(r) and ρ.

def _real_only(dtype, what):
    if np.dtype(dtype).kind == "c":
        raise NotImplementedError(f"{what}: complex element types are not supported (Float32 and Float64 only)")


def diag(A: PSparseMatrix) -> PVector:
    """diag(A) as a PVector on A.cols (pa_mat_diag): the stored diagonal entry
    of every owned row (+0.0 where the pattern has none), then exchange! once,
    so every ghost value equals its owner's and a division over all lids never
    divides by a ghost slot's zero.  It reads the entry the owner stores: for
    a matrix assembled from cell contributions it belongs after assemble_(A).
    The entry table is not built and nzval is not downloaded."""
    _real_only(A.dtype, "diag")
    if not oids_are_equal(A.rows, A.cols):
        raise AssertionError("diag: A.rows and A.cols own different ids")
    d = PVector.undef(A.cols, A.dtype)
    for M, (r, c), dv in zip(A.values.parts, _mat_index(A, False), d.values.parts):
        _lib.call("pa_mat_diag", M.h, r.h, c.h, dv.h)
    return exchange_(d)


class Jacobi:
    """The diagonal preconditioner Diagonal(diag(A)): Jacobi(A), or Jacobi(d)
    from a PVector holding the diagonal on every lid.  A zero diagonal is no
    error: it yields Inf / NaN, as ldiv!(c, Diagonal(d), r) does in Julia."""

    def __init__(self, A_or_d):
        self.d = diag(A_or_d) if isinstance(A_or_d, PSparseMatrix) else A_or_d
        if not isinstance(self.d, PVector):
            raise TypeError("Jacobi: a PSparseMatrix or a PVector")
        _real_only(self.d.dtype, "Jacobi")


def _on_rows(d: PVector, like: PVector) -> PVector:
    """d as a vector of like's PRange object (owned values copied, ghosts exchanged)"""
    if d.rows is like.rows:
        return d
    dd = like.similar(dtype=d.dtype)
    copyto_(dd, d)
    return exchange_(dd)


def pcg_apply_(c: PVector, r: PVector, d: PVector):
    """c .= r ./ d over all lids and dot(c, r) in one pass (pa_pcg_apply_all);
    the three vectors share one PRange.  Returns the dot, of the element type."""
    if not (c.rows is r.rows is d.rows):
        raise ValueError("pcg_apply_: the three vectors must share one PRange")
    out = _scalar_out(c.dtype)
    _lib.call("pa_pcg_apply_all", len(c.values.parts), _hs(c.values.parts), _hs(r.values.parts), _hs(d.values.parts),
              _lib.ptr_array(_idx(c)), out.ctypes.data_as(C.c_void_p))
    return out[0]


def pcg_update_(x: PVector, r: PVector, u: PVector, c: PVector, d: PVector, alpha):
    """x .+= α.*u; r .-= α.*c; c .= r ./ d in one pass over all lids
    (pa_pcg_update_all), α converted to the element type.  Returns norm(r)
    (a float) and dot(c, r) (of the element type) of the new values.  The
    owned lids must be contiguous (the entry refuses anything else)."""
    if not (x.rows is r.rows is u.rows is c.rows is d.rows):
        raise ValueError("pcg_update_: the five vectors must share one PRange")
    al, alp = _lib.scalar_buf(alpha, x.dtype)
    nr = C.c_double(0.0)
    out = _scalar_out(x.dtype)
    _lib.call("pa_pcg_update_all", len(x.values.parts), _hs(x.values.parts), _hs(r.values.parts),
              _hs(u.values.parts), _hs(c.values.parts), _hs(d.values.parts), _lib.ptr_array(_idx(x)), alp,
              C.byref(nr), out.ctypes.data_as(C.c_void_p))
    return nr.value, out[0]


def _pcg(x: PVector, A: PSparseMatrix, b: PVector, Pl, reltol, abstol, maxiter, history, fused):
    """IterativeSolvers 0.9's preconditioned CG iterate with Pl = Jacobi:
    u = 0; r = b - A*x; residual = norm(r); ρ = one(T); per iteration
    c = Pl \\ r; ρ_prev = ρ; ρ = dot(c, r); β = ρ/ρ_prev; u .= c .+ β.*u;
    c = A*u; α = ρ/dot(u, c); x .+= α.*u; r .-= α.*c; residual = norm(r).
    ρ, β and α are of the element type T (dot of two PVectors is a T), the
    residual a Float64.  fused: Pl \\ r with ρ once (pa_pcg_apply_all), then
    per iteration the u update, mul! with dot(u, c), and the x / r updates
    with the next Pl \\ r, norm(r) and ρ in one pass (pa_pcg_update_all);
    otherwise the same arithmetic from the separate operations.  The fused
    pass and mul!'s fused dot need contiguous owned lids: this is the caller's
    check the entries ask for, and other layouts take the separate operations."""
    if not isinstance(Pl, Jacobi):
        raise TypeError("cg_(Pl=...): Pl must be a Jacobi")
    _real_only(x.dtype, "cg_(Pl=...)")
    T = np.dtype(x.dtype).type
    if Pl.d.dtype != x.dtype:
        raise TypeError("cg_(Pl=...): the preconditioner's element type differs from x's")
    u = x.similar().fill_(0)
    r = x.similar()
    c = x.similar()
    d = _on_rows(Pl.d, x)
    copyto_(r, b)
    mul_(c, A, x)
    sub_(r, c)
    residual = norm(r)
    tol = max(reltol * norm(b), abstol)
    rho = T(1)
    it = 0
    fuse = fused and _own_contig(u)
    done = lambda: it >= maxiter or residual <= tol
    if fuse and not done():
        rho_next = pcg_apply_(c, r, d)
    with np.errstate(all="ignore"):  # a zero ρ or dot gives Inf / NaN as in Julia
        while not done():
            if fuse:
                rho_prev, rho = rho, T(rho_next)
            else:
                assign_(c, r / d)
                rho_prev, rho = rho, T(dot(c, r))
            beta = T(rho / rho_prev)
            xpby_(u, c, beta)
            if fuse:
                alpha = T(rho / T(mul_dot_(c, A, u)))
                residual, rho_next = pcg_update_(x, r, u, c, d, alpha)
            else:
                mul_(c, A, u)
                alpha = T(rho / T(dot(u, c)))
                axpy_(x, alpha, u)
                axmy_(r, alpha, c)
                residual = norm(r)
            it += 1
            if history is not None:
                history.append(residual)
    return x


def _pcg_device(x: PVector, A: PSparseMatrix, b: PVector, Pl, reltol, abstol, maxiter, history, batch):
    """_pcg's fused loop with its scalars on the device (pa_pcg_solve_all):
    the same x, residual history and iteration count, bit for bit."""
    if not isinstance(Pl, Jacobi):
        raise TypeError("cg_device_(Pl=...): Pl must be a Jacobi")
    _real_only(x.dtype, "cg_device_(Pl=...)")
    if Pl.d.dtype != x.dtype:
        raise TypeError("cg_device_(Pl=...): the preconditioner's element type differs from x's")
    if not _own_contig(x):
        raise ValueError("cg_device_(Pl=...): x needs contiguous owned lids")
    d = _on_rows(Pl.d, x)
    if b.rows is not x.rows:  # copyto!(r, b) across partitions copies the owned values
        bb = x.similar()
        copyto_(bb, b)
        b = bb
    u, r, c = x.similar(), x.similar(), x.similar()
    ctxs = contexts(A.values)
    n = len(ctxs)
    ex = x.rows.exchanger
    has_x = any(len(ex.parts_rcv.local(p)) or len(ex.parts_snd.local(p)) for p in x.values.part_ids)
    xg = [device_exchanger(cx, ex, p) for cx, p in zip(ctxs, x.values.part_ids)] if has_x else None
    its = C.c_int64(0)
    res = C.c_double(0.0)
    hist = np.zeros(max(1, int(maxiter)), dtype=np.float64) if history is not None else None
    _lib.call("pa_pcg_solve_all", n, _hs(A.values.parts), _hs(x.values.parts), _hs(b.values.parts),
              _hs(d.values.parts), _hs(u.values.parts), _hs(r.values.parts), _hs(c.values.parts),
              _lib.ptr_array(_idx(x)), _hs(xg) if xg else None, float(reltol), float(abstol), int(maxiter),
              int(batch), C.byref(its), C.byref(res),
              hist.ctypes.data_as(C.POINTER(C.c_double)) if hist is not None else None)
    if history is not None:
        history.extend(float(v) for v in hist[:its.value])
    return x


def cg_device_(x: PVector, A: PSparseMatrix, b: PVector, Pl=None, reltol=None, abstol=0.0, maxiter=None,
               history=None, batch=8):
    """cg_ with the recurrence's scalars on the device: the host enqueues
    `batch` iterations between reads of the done flag.  Pl=None is
    cg_(…, device=True) (pa_cg_solve_all); Pl=Jacobi(A) is the preconditioned
    iterate (pa_pcg_solve_all), Float32 / Float64, whose results equal
    cg_(…, Pl=Pl, fused=True) bit for bit.  Both need contiguous owned lids
    (ValueError otherwise)."""
    real = np.float32 if x.dtype in (np.float32, np.complex64) else np.float64
    if reltol is None:  # sqrt(eps(real(eltype(b)))), in that type
        reltol = float(np.sqrt(np.finfo(real).eps))
    if maxiter is None:
        maxiter = len(A.cols)
    if Pl is None:
        return _cg_device(x, A, b, reltol, abstol, maxiter, history, batch)
    return _pcg_device(x, A, b, Pl, reltol, abstol, maxiter, history, batch)


# ---------------------------------------------------------------------------
# Gather to MAIN and direct solves (Interfaces.jl:2626-2757).  Not efficient,
# just for convenience and debugging purposes, as the reference says of its
# own: the whole system moves to MAIN and is factored there on the host.  The
# device does the rest: reading the stored entries back (pa_mat_findnz),
# moving them and the vectors to MAIN (the COO and vector assemble) and
# scattering the solution (the vector exchange).

def findnz(A: PSparseMatrix, rows="owned", ids="global") -> COO:
    """findnz / nziterator of every part of A on the device (pa_mat_findnz):
    a COO whose parts hold the stored entries in the parent's storage order —
    rows="owned": of the rows the part owns (the filter of gather(A),
    Interfaces.jl:2671-2687), rows="all": of the stored ghost rows too;
    ids="global" (gids) or "local" (lids of A.rows / A.cols).  The COO
    composes with assemble_, exchange_, PSparseMatrix.from_coo and to_host."""
    if rows not in ("owned", "all"):
        raise ValueError("findnz: rows must be 'owned' or 'all'")
    if ids not in ("global", "local"):
        raise ValueError("findnz: ids must be 'global' or 'local'")
    glob = ids == "global"
    parts = [M.findnz(r, c, all_rows=rows == "all", ids_global=glob)
             for M, (r, c) in zip(A.values.parts, _mat_index(A, glob))]
    p = A.values
    return COO(PData(p.backend, p.part_ids, parts, p.shape))


class _OwnedMap:
    """An index set whose "owned" lids are the places `target` (1-based lids
    of an n-vector) in order: pa_vec_copy between it and a range's own index
    set moves the range's owned values to or from those places."""

    def __init__(self, n, target):
        self.oid_to_lid = np.asarray(target, dtype=np.int32)
        rest = np.ones(n, dtype=bool)
        rest[self.oid_to_lid - 1] = False
        self.hid_to_lid = (np.flatnonzero(rest) + 1).astype(np.int32)
        self.num_lids, self.num_oids, self.num_hids = int(n), len(self.oid_to_lid), len(self.hid_to_lid)


def _main_maps(rows: PRange, rows_in_main: PRange):
    """per part, the device index over rows_in_main's lids that places the
    owned values of rows: by gid on MAIN, in oid order elsewhere
    (Interfaces.jl:2709-2716); rows_in_main must be a to_main range of rows"""
    if rows.partition.part_ids != rows_in_main.partition.part_ids or len(rows) != len(rows_in_main):
        raise ValueError("gather / scatter!: the range in MAIN is not one of this range (parts or length differ)")
    cache = rows_in_main.__dict__.setdefault("_main_maps", {})
    hit = cache.get(id(rows.partition))
    if hit is not None and hit[0] is rows.partition:
        return hit[1]
    maps = []
    for c, s, m in zip(contexts(rows.partition), rows.partition.parts, rows_in_main.partition.parts):
        own = s.lid_to_gid[s.oid_to_lid - 1]
        if s.part == MAIN:
            ok = m.num_lids == len(rows) and np.array_equal(m.lid_to_gid, np.arange(1, len(rows) + 1))
            target = own
        else:
            ok = np.array_equal(m.lid_to_gid, own)
            target = np.arange(1, len(own) + 1)
        if not ok:
            raise ValueError(f"gather / scatter!: the range in MAIN does not hold this range's ids on part {s.part}")
        maps.append(DeviceIndex(c, _OwnedMap(m.num_lids, target)))
    cache[id(rows.partition)] = (rows.partition, maps)
    return maps


def gather(x, rows_in_main: PRange = None, cols_in_main: PRange = None):
    """gather(a) of a PData: the parts' values collected on MAIN
    (backends.gather).  Not efficient, for convenience and debugging:

    gather(b::PVector, rows_in_main = to_main(b.rows)) (Interfaces.jl:
    2706-2719): b_in_main = PVector(zero(T), rows_in_main) takes b's owned
    values — by gid on MAIN, in oid order on the other parts — and
    assemble!(b_in_main) adds them onto MAIN's, all on the device.

    gather(A::PSparseMatrix, rows_in_main, cols_in_main) (2664-2704):
    findnz(A, "owned", "global"), assemble!(I, J, V, rows_in_main), the
    triplets of the parts other than MAIN dropped, and PSparseMatrix(I, J, V,
    rows_in_main, cols_in_main; ids=:global) with A's parent kind and an
    empty exchanger: MAIN holds the whole matrix, the others an empty one."""
    if isinstance(x, PData):
        if rows_in_main is not None or cols_in_main is not None:
            raise TypeError("gather(a::PData) takes no ranges")
        return _gather_pdata(x)
    if isinstance(x, PVector):
        if cols_in_main is not None:
            raise TypeError("gather(b, rows_in_main): a PVector has no cols")
        rows_in_main = rows_in_main if rows_in_main is not None else to_main(x.rows)
        maps = _main_maps(x.rows, rows_in_main)
        b_in_main = PVector.full(0, rows_in_main, dtype=x.dtype)
        for d, m, v, i in zip(b_in_main.values.parts, maps, x.values.parts, _idx(x)):
            _lib.call("pa_vec_copy", d.h, m.h, v.h, i, 0)
        return assemble_(b_in_main)
    if not isinstance(x, PSparseMatrix):
        raise TypeError("gather: a PData, a PVector or a PSparseMatrix")
    rows_in_main = rows_in_main if rows_in_main is not None else to_main(x.rows)
    cols_in_main = cols_in_main if cols_in_main is not None else to_main(x.cols)
    _main_maps(x.rows, rows_in_main), _main_maps(x.cols, cols_in_main)  # the ranges are the matrix's
    coo = assemble_(findnz(x, "owned", "global"), rows_in_main)
    p = coo.values
    none = np.zeros(0, np.int64)
    kept = [c if part == MAIN else DeviceCOO(c.ctx, none, none, np.zeros(0, c.dtype))
            for c, part in zip(p.parts, p.part_ids)]
    bi = x.values.parts[0].csr_bi
    return PSparseMatrix.from_coo(COO(PData(p.backend, p.part_ids, kept, p.shape)), None, None, rows_in_main,
                                  cols_in_main, ids="global", init=None if bi is None else csr_init(bi),
                                  exchanger=empty_exchanger(rows_in_main.partition))


def scatter_(c: PVector, c_in_main: PVector) -> PVector:
    """scatter!(c, c_in_main) (Interfaces.jl:2721-2732): exchange!(c_in_main)
    sends MAIN's values to the parts, then c's owned values are taken from
    it (by gid on MAIN, in oid order elsewhere); c's ghost values stay."""
    if np.dtype(c.dtype) != np.dtype(c_in_main.dtype):
        raise TypeError("scatter!: element types differ")
    maps = _main_maps(c.rows, c_in_main.rows)
    exchange_(c_in_main)
    for d, i, v, m in zip(c.values.parts, _idx(c), c_in_main.values.parts, maps):
        _lib.call("pa_vec_copy", d.h, i, v.h, m.h, 0)
    return c


class _DenseLU:
    """the numpy.linalg stand-in for a sparse LU of a small matrix"""

    def __init__(self, a):
        self.a = a

    def solve(self, b):
        return np.linalg.solve(self.a, b)


def _main_lu(csc: CSC):
    """The factorisation of MAIN's gathered matrix, on the host: an object
    with solve(b).  csc is the canonical local CSC (rows ascending in every
    column, no duplicates).  scipy.sparse.linalg.splu when scipy is there;
    without it a dense numpy.linalg solve up to 8192 unknowns."""
    if csc.m != csc.n:
        raise _lib.PAError(f"lu: the matrix is not square ({csc.m} x {csc.n})")
    try:
        from scipy.sparse import csc_matrix
        from scipy.sparse.linalg import splu
    except ImportError:
        if csc.n > 8192:
            raise _lib.PAError(f"lu: {csc.n} unknowns need scipy.sparse.linalg.splu, and scipy cannot be imported "
                               "(the dense numpy.linalg fallback stops at 8192)")
        a = np.zeros((csc.m, csc.n), dtype=csc.nzval.dtype)
        a[csc.rowval - 1, np.repeat(np.arange(csc.n), np.diff(csc.colptr))] = csc.nzval
        return _DenseLU(a)
    return splu(csc_matrix((csc.nzval, csc.rowval - 1, csc.colptr - 1), shape=(csc.m, csc.n)))


def _main_csc(a_in_main: PSparseMatrix, dtype=None):
    """MAIN's gathered local matrix on the host as the canonical CSC (None
    where this process does not hold MAIN): the findnz download, compressed"""
    for part, M, (r, c), s, t in zip(a_in_main.values.part_ids, a_in_main.values.parts, _mat_index(a_in_main, False),
                                     a_in_main.rows.partition.parts, a_in_main.cols.partition.parts):
        if part == MAIN:
            I, J, V = M.findnz(r, c, all_rows=True, ids_global=False).download()
            return compresscoo(I, J, V.astype(dtype or V.dtype), s.num_lids, t.num_lids)
    return None


class PLU:
    """PLU (Interfaces.jl:2641-2645): MAIN's factors and the ranges in MAIN.
    Not efficient, for convenience and debugging."""

    def __init__(self, lu_in_main, rows: PRange, cols: PRange, dtype, src_rows: PRange, src_cols: PRange):
        self.lu_in_main, self.rows, self.cols, self.dtype = lu_in_main, rows, cols, np.dtype(dtype)
        self._src = (src_rows, src_cols)


def _factor(a_in_main, dtype):
    csc = _main_csc(a_in_main, dtype)
    return _main_lu(csc) if csc is not None else None


def lu(A: PSparseMatrix, dtype=None) -> PLU:
    """lu(A) (Interfaces.jl:2646-2650): gather(A), then the LU on MAIN's host
    (_main_lu).  Not efficient, for convenience and debugging."""
    a_in_main = gather(A)
    dtype = np.dtype(dtype or A.dtype)
    return PLU(_factor(a_in_main, dtype), a_in_main.rows, a_in_main.cols, dtype, A.rows, A.cols)


def lu_(F: PLU, A: PSparseMatrix) -> PLU:
    """lu!(F, A) (Interfaces.jl:2651-2655): A gathered again through F.rows
    and F.cols — the ranges in MAIN and their exchangers are reused — and
    factored anew."""
    F.lu_in_main = _factor(gather(A, F.rows, F.cols), F.dtype)
    F._src = (A.rows, A.cols)
    return F


def ldiv_(c: PVector, F: PLU, b: PVector) -> PVector:
    """ldiv!(c, F, b) (Interfaces.jl:2656-2662): b gathered through F.rows,
    solved on MAIN's host, and scattered into c's owned values.

    ldiv!(c, P::Jacobi, b): c .= b ./ P.d over all lids on the device
    (pa_pcg_apply_all; its dot is discarded)."""
    if isinstance(F, Jacobi):
        _real_only(c.dtype, "ldiv_(c, Jacobi, b)")
        if c.rows is not b.rows:
            raise ValueError("ldiv_(c, Jacobi, b): c and b must share one PRange")
        pcg_apply_(c, b, _on_rows(F.d, c))
        return c
    b_in_main = gather(b, F.rows)
    c_in_main = PVector.full(0, F.cols, dtype=c.dtype)
    _main_maps(c.rows, F.cols)
    for part, vb, vc in zip(b_in_main.values.part_ids, b_in_main.values.parts, c_in_main.values.parts):
        if part == MAIN:
            x = F.lu_in_main.solve(vb.download().astype(F.dtype))
            vc.upload(np.ascontiguousarray(x, dtype=c.dtype))
    return scatter_(c, c_in_main)


def zerox(A: PSparseMatrix, b: PVector) -> PVector:
    """IterativeSolvers.zerox(A, b) (Interfaces.jl:2752-2757): zeros of the
    solve's element type over A.cols."""
    return PVector.full(0, A.cols, dtype=np.result_type(A.dtype, b.dtype))


def solve(A: PSparseMatrix, b: PVector) -> PVector:
    """A \\ b (Interfaces.jl:2626-2638).  Not efficient, just for convenience
    and debugging purposes: A and b are gathered on MAIN (on the device),
    MAIN's host factors and solves, and the solution is scattered over
    A.cols.  The element type is numpy.result_type of the two."""
    c = zerox(A, b)
    return ldiv_(c, lu(A, dtype=c.dtype), b)
