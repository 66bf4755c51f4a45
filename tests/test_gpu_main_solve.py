"""Gather to MAIN and direct solves on the device (Interfaces.jl:2626-2757):
pamd.findnz (pa_mat_findnz) against the oracle's nz_entries, and to_main /
gather / scatter_ / solve / lu / lu_ / ldiv_ / zerox against the sequential
restatement of tests/main_solve_ref.py.  Every comparison is bit for bit, sign
of zero included, except the residuals of the solves, which are held to the
reference's own bound (tests/golden/interfaces_kats.json, residual_tol)."""
import contextlib
import json
import os

import numpy as np
import pytest

import main_solve_ref as R
import matrix_cases as MC
from mat_view_ref import bits

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
PARENTS = ["csc", 0, 1]  # a SparseMatrixCSC parent, or SparseMatrixCSR{Bi}
NL = 200
# entries one grid pass of k_findnz_write covers: kFindnzBlocks = 2048 blocks of 256 threads (pa_coo.hip)
PASS = 2048 * 256
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "interfaces_kats.json")))["irregular_coo"]


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


@pytest.fixture(scope="module")
def be_rccl(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    prev = pamd._lib.tune("halo_transport", 0)
    yield pamd.HIPBackend(devices=[0], rccl=True)
    pamd._lib.tune("halo_transport", prev)


def pdata(parts, values):
    return type(parts)(parts.backend, parts.part_ids, list(values), parts.shape)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@contextlib.contextmanager
def knob(pamd, key, value):
    prev = pamd._lib.tune(key, value)
    try:
        yield
    finally:
        pamd._lib.tune(key, prev)


def entries(dtype, n, rng):
    """uniform(-1, 1) * 10^k, k in -3..3"""
    f = lambda: rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-3, 4, n)
    V = f()
    if np.dtype(dtype).kind == "c":
        V = V + 1j * f()
    return V.astype(dtype)


def minus_zero(dtype):
    return np.dtype(dtype).type(complex(-0.0, -0.0) if np.dtype(dtype).kind == "c" else -0.0)


def is_minus_zero(v):
    v = np.asarray(v)
    return (v == 0) & np.signbit(v.real) & (np.signbit(v.imag) if np.iscomplexobj(v) else True)


def is_plus_zero(v):
    v = np.asarray(v)
    return (v == 0) & ~np.signbit(v.real) & (~np.signbit(v.imag) if np.iscomplexobj(v) else True)


def nz_order(M):
    """1-based (row, col) lids of a host CSC / CSR in nziterator order
    (SparseUtils.jl:106-150, 254-300); the values are M.nzval in that order"""
    if hasattr(M, "rowptr"):
        return (np.repeat(np.arange(1, M.m + 1, dtype=np.int64), np.diff(M.rowptr)),
                (M.colval - M.Bi + 1).astype(np.int64))
    return M.rowval.astype(np.int64), np.repeat(np.arange(1, M.n + 1, dtype=np.int64), np.diff(M.colptr))


def oracle_matrix(O, M):
    if hasattr(M, "rowptr"):
        return O.CSR(M.Bi, M.m, M.n, M.rowptr, M.colval, M.nzval)
    return O.CSC(M.m, M.n, M.colptr, M.rowval, M.nzval)


def oracle_range(O, r):
    parts = [O.IndexSet(s.part, s.lid_to_gid.tolist(), s.lid_to_part.tolist(), s.oid_to_lid.tolist(),
                        s.hid_to_lid.tolist()) for s in r.partition.parts]
    return O.prange(r.ngids, O.PData(parts, r.partition.shape), ghost=bool(r.ghost))


def expected(M, r, c, which, ids, order=None):
    """what findnz must give for one part whose parent is the host matrix M"""
    i, j = nz_order(M)
    v = M.nzval
    if order is not None:
        i, j, v = i[order], j[order], v[order]
    if which == "owned":
        keep = r.lid_to_part[i - 1] == r.part
        i, j, v = i[keep], j[keep], v[keep]
    if ids == "global":
        i, j = r.lid_to_gid[i - 1], c.lid_to_gid[j - 1]
    return i, j, v


KINDS = [(w, k) for w in ("owned", "all") for k in ("global", "local")]


def check_findnz(pamd, A, Ms, order=None, kinds=KINDS, what=""):
    for which, ids in kinds:
        coo = pamd.findnz(A, which, ids)
        I, J, V = coo.to_host()
        for p, (M, r, c) in enumerate(zip(Ms, A.rows.partition.parts, A.cols.partition.parts)):
            wi, wj, wv = expected(M, r, c, which, ids, None if order is None else order[p])
            assert I.parts[p].dtype == np.int64 and J.parts[p].dtype == np.int64
            assert np.array_equal(I.parts[p], wi), (what, which, ids, p)
            assert np.array_equal(J.parts[p], wj), (what, which, ids, p)
            assert same_bits(V.parts[p], wv), (what, which, ids, p)


def one_part_rows(pamd, be, nl, seed=3):
    """one part whose lids are a permutation of the gids 1..nl (gid != lid)"""
    parts = be.get_part_ids(1)
    gids = np.random.default_rng(seed).permutation(nl).astype(np.int64) + 1
    assert (gids != np.arange(1, nl + 1)).any()
    part = pdata(parts, [pamd.IndexSet(1, gids, np.ones(nl, np.int32))])
    return parts, pamd.prange_from_partition(nl, part, ghost=False)


def host_parent(pamd, parent, I, J, V, m, n):
    return pamd.compresscoo(I, J, V, m, n) if parent == "csc" else pamd.sparsecsr(parent, I, J, V, m, n)


def init_of(pamd, parent):
    return None if parent == "csc" else pamd.csr_init(parent)


# ---------------------------------------------------------------------------
# 1. findnz against nz_entries

def irregular_triplets(nl, rng):
    """(I, J) lids of about 7.5 * nl distinct entries, 1..14 per row"""
    lens = rng.integers(1, 15, nl)
    I = np.repeat(np.arange(1, nl + 1), lens)
    J = np.concatenate([rng.choice(nl, size=k, replace=False) + 1 for k in lens])
    o = rng.permutation(len(I))
    return I[o].astype(np.int64), J[o].astype(np.int64)


@pytest.mark.parametrize("builder", ["parent", "coo_host", "coo_device"])
@pytest.mark.parametrize("parent", PARENTS, ids=lambda p: f"parent_{p}")
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_findnz_against_nz_entries(be, pamd, O, dtype, parent, builder):
    rng = np.random.default_rng(5)
    I0, J0 = irregular_triplets(NL, rng)
    V0 = entries(dtype, len(I0), rng)
    V0[11] = minus_zero(dtype)
    assert 1400 <= len(I0) <= 1600
    M = host_parent(pamd, parent, I0, J0, V0, NL, NL)
    assert is_minus_zero(M.nzval).sum() == 1
    parts, rows = one_part_rows(pamd, be, NL)
    s = rows.partition.parts[0]
    if builder == "parent":
        build = pamd.PSparseMatrix.from_csc if parent == "csc" else pamd.PSparseMatrix.from_csr
        A = build(pdata(parts, [M]), rows, rows)
    elif builder == "coo_host":
        A = pamd.PSparseMatrix.from_coo(pdata(parts, [I0.copy()]), pdata(parts, [J0.copy()]), pdata(parts, [V0]),
                                        rows, rows, ids="local", init=init_of(pamd, parent))
    else:
        coo = pamd.COO.from_host(pdata(parts, [s.lid_to_gid[I0 - 1]]), pdata(parts, [s.lid_to_gid[J0 - 1]]),
                                 pdata(parts, [V0]), rows)
        A = pamd.PSparseMatrix.from_coo(coo, None, None, rows, rows, ids="global", init=init_of(pamd, parent))
    # the order the test expects is the oracle's nziterator
    e = O.nz_entries(oracle_matrix(O, M))
    wi, wj = nz_order(M)
    assert [k for k, _, _ in e] == list(range(1, len(wi) + 1))
    assert np.array_equal([i for _, i, _ in e], wi) and np.array_equal([j for _, _, j in e], wj)
    check_findnz(pamd, A, [M])
    I, J, V = pamd.findnz(A, "all", "local").to_host()
    assert is_minus_zero(V.parts[0]).sum() == 1  # the -0.0 survives
    assert A.values.parts[0].entry_table() == (0, 0)  # no entry table was built behind the caller's back
    assert same_bits(A.values.parts[0].get_values(), M.nzval)  # and A is unchanged


# ---------------------------------------------------------------------------
# 2. more entries than one grid pass

def test_second_grid_pass(be, pamd):
    nl, count = 3000, PASS + 66_001
    assert count > PASS and count % 64 != 0  # the pass size this case means to exceed
    rng = np.random.default_rng(7)
    flat = rng.choice(nl * nl, size=count, replace=False)
    I0, J0 = flat // nl + 1, flat % nl + 1
    V0 = rng.uniform(-1, 1, count)
    for parent in ("csc", 1):
        M = host_parent(pamd, parent, I0, J0, V0, nl, nl)
        assert len(M.nzval) == count
        parts, rows = one_part_rows(pamd, be, nl)
        build = pamd.PSparseMatrix.from_csc if parent == "csc" else pamd.PSparseMatrix.from_csr
        A = build(pdata(parts, [M]), rows, rows)
        assert len(pamd.findnz(A, "all", "local").values.parts[0]) == count > PASS
        check_findnz(pamd, A, [M], kinds=[("owned", "global"), ("all", "local")], what=parent)


# ---------------------------------------------------------------------------
# 3. every layout at once, 4. round trip

GRID = (30, 12, 6)  # x-lines of 30 rows (no divisor of a slice's 128 or 256 rows), 12 per z-plane, 3 planes per part
LONG = (400, 600)   # draws of the two long rows of each part (distinct columns: more than max(256, 8 x 27))


def neighbours27(grid, g):
    """(I, J) gids of the 27-point neighbourhoods of the nodes g inside the grid"""
    nx, ny, nz = grid
    g0 = g - 1
    x, y, z = g0 % nx, g0 // nx % ny, g0 // (nx * ny)
    Is, Js = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                X, Y, Z = x + dx, y + dy, z + dz
                ok = (X >= 0) & (X < nx) & (Y >= 0) & (Y < ny) & (Z >= 0) & (Z < nz)
                Is.append(g[ok])
                Js.append(1 + X[ok] + nx * (Y[ok] + ny * Z[ok]))
    return np.concatenate(Is), np.concatenate(Js)


class FECase:
    """A 27-point operator over two parts as an FE assembly leaves it: each
    part stores its owned rows and the rows of its ghost nodes (the plane of
    the other part next to the interface), plus the long rows of
    matrix_cases.long_row_coo over two of its owned rows.  The triplets are
    generated here, as tests/test_gpu_mat_view.py generates its twin: no
    problem of the oracle assembles a 27-point matrix with stored ghost rows
    (its stencil_problem stores owned rows only, its fem_sa_problem is the
    2-D 9-point one); the oracle supplies the expected order (nz_entries) and
    the restatement of gather(A) over this matrix."""

    def __init__(self, pamd, be, dtype, f32_rows=0, seed=29):
        rng = np.random.default_rng(seed)
        self.dtype, self.f32_rows = dtype, f32_rows
        self.parts = parts = be.get_part_ids(2)
        n = int(np.prod(GRID))
        rows, cols = pamd.prange_linear(parts, n), pamd.prange_linear(parts, n)
        Ig, Jg = [], []
        for s in rows.partition.parts:
            own = s.lid_to_gid[s.oid_to_lid - 1]
            nodes = np.unique(neighbours27(GRID, own)[1])  # owned nodes and the ghost plane
            i, j = neighbours27(GRID, nodes)
            keep = np.isin(j, nodes)
            Ig.append(i[keep])
            Jg.append(j[keep])
        pamd.add_gids_(rows, pdata(parts, Ig))
        pamd.add_gids_(cols, pdata(parts, Jg))
        for k, p in enumerate(parts.part_ids):  # the long rows: lids of cols (its owned lids are the rows' too)
            c = cols.partition.local(p)
            li, lj, _, longs = MC.long_row_coo(rng, cols, p, dtype, list(LONG))
            sel = np.isin(li, longs)
            Ig[k] = np.concatenate([Ig[k], c.lid_to_gid[li[sel] - 1]])
            Jg[k] = np.concatenate([Jg[k], c.lid_to_gid[lj[sel] - 1]])
            o = rng.permutation(len(Ig[k]))
            Ig[k], Jg[k] = Ig[k][o], Jg[k][o]
        self.rows, self.cols = rows, cols
        self.Ig, self.Jg = Ig, Jg
        self.V0 = [entries(dtype, len(i), rng) for i in Ig]
        with knob(pamd, "f32_rows", f32_rows):
            self.A = pamd.PSparseMatrix.from_coo(pdata(parts, [i.copy() for i in Ig]),
                                                 pdata(parts, [j.copy() for j in Jg]), pdata(parts, self.V0),
                                                 rows, cols, ids="global")
        # the host restatement of sparse(I, J, V): the parents
        self.csc = [pamd.compresscoo(r.to_lids(i), c.to_lids(j), v, r.num_lids, c.num_lids)
                    for r, c, i, j, v in zip(rows.partition.parts, cols.partition.parts, Ig, Jg, self.V0)]

    def counters(self):
        out = {}
        for M in self.A.values.parts:
            info = M.info()
            info["ghost_nnz"] = M.csc_nnz - info["nnz"]
            for k, v in info.items():
                out[k] = out.get(k, 0) + v
        return out


_FE = {}


def fe_case(pamd, be, dtype, f32_rows=0):
    if (dtype, f32_rows) not in _FE:
        _FE[dtype, f32_rows] = FECase(pamd, be, dtype, f32_rows)
    return _FE[dtype, f32_rows]


# The structures each matrix must show, so that a layout change cannot empty
# the test.  Float64 has 2 rows per lane; Float32 with f32_rows 4 keeps 4 rows
# per lane, and the rows of its delta16 slices are interleaved.
MUST_SHOW = {
    ("float64", 0): ("pattern_slices", "side_rows", "triple_sell_slices", "tri_slices", "pair_slices", "long_rows",
                     "ghost_nnz"),
    ("float32", 4): ("pattern_slices", "side_rows", "delta16_slices", "long_rows", "ghost_nnz"),
}


@pytest.mark.parametrize("name,f32_rows", sorted(MUST_SHOW))
def test_every_layout_at_once(be, pamd, O, name, f32_rows):
    dtype = np.dtype(name).type
    c = fe_case(pamd, be, dtype, f32_rows)
    A, parts = c.A, c.parts
    cnt = c.counters()
    print({k: cnt[k] for k in ("nrows", "nslices", "nnz", "pattern_slices", "regular_rows", "side_rows",
                               "delta16_slices", "triple_sell_slices", "tri_slices", "pair_slices", "long_rows",
                               "ghost_nnz")})
    for key in MUST_SHOW[name, f32_rows]:
        assert cnt[key] > 0, key
    assert cnt["long_rows"] == 2 * len(LONG)
    for M in c.csc:  # the expected order is the oracle's nziterator here too
        e = O.nz_entries(oracle_matrix(O, M))
        wi, wj = nz_order(M)
        assert np.array_equal([i for _, i, _ in e], wi) and np.array_equal([j for _, _, j in e], wj)
    for fmt in (1, 0):
        with knob(pamd, "spmv_format", fmt):
            check_findnz(pamd, A, c.csc, what=f"format {fmt}")
    # rows="owned" holds no entry of a ghost row, rows="all" all of them
    own, every = pamd.findnz(A, "owned", "local").to_host(), pamd.findnz(A, "all", "local").to_host()
    for p, (r, M) in enumerate(zip(c.rows.partition.parts, A.values.parts)):
        ghost = r.lid_to_part[every[0].parts[p] - 1] != r.part
        assert ghost.sum() == M.csc_nnz - M.info()["nnz"] > 0
        assert (r.lid_to_part[own[0].parts[p] - 1] == r.part).all()
        assert len(own[0].parts[p]) == M.info()["nnz"]
    # new values: fillstored!, the entry views, assemble!(A) — findnz reads what nonzeros(A) holds
    rng = np.random.default_rng(41)
    try:
        pamd.fillstored_(A, 0)
        assert all(not v.any() for v in pamd.findnz(A, "all", "global").to_host()[2].parts)
        W = [entries(dtype, len(M.nzval), rng) for M in c.csc]
        ij = [nz_order(M) for M in c.csc]
        pamd.add_coo_(A, pdata(parts, [i for i, _ in ij]), pdata(parts, [j for _, j in ij]), pdata(parts, W),
                      ids="local")
        changed = [pamd.CSC(M.m, M.n, M.colptr, M.rowval, w) for M, w in zip(c.csc, W)]
        check_findnz(pamd, A, changed, what="after add_coo_")
        pamd.assemble_(A)
        after = [M.get_values() for M in A.values.parts]
        assert any(not same_bits(a, w) for a, w in zip(after, W))  # (the ghost rows were sent and zeroed)
        moved = [pamd.CSC(M.m, M.n, M.colptr, M.rowval, a) for M, a in zip(c.csc, after)]
        for fmt in (1, 0):
            with knob(pamd, "spmv_format", fmt):
                check_findnz(pamd, A, moved, what=f"after assemble_, format {fmt}")
    finally:
        for M, H in zip(A.values.parts, c.csc):
            M.set_values(H.nzval)


def test_findnz_with_the_uniform_layout(be, pamd):
    """The uniform layout of short Float64 pattern rows (FD7) is one more copy
    of the values: findnz reads the main array, with it and without it."""
    grid = (12, 11, 9)
    parts = be.get_part_ids((1, 1, 1))
    rows, cols = pamd.drivers.stencil_partition(parts, grid, 7)
    s = rows.partition.parts[0]
    own = s.lid_to_gid[s.oid_to_lid - 1]
    i, J, V = pamd.drivers.stencil_entries(7, grid, own)
    I = own[i]
    V = V * np.random.default_rng(43).uniform(0.5, 1.5, len(V))  # distinct values
    M = pamd.compresscoo(s.to_lids(I), cols.partition.parts[0].to_lids(J), V, s.num_lids, s.num_lids)
    traffic = {}
    for uniform in (1, 0):
        with knob(pamd, "spmv_uniform", uniform):
            A = pamd.PSparseMatrix.from_coo(pdata(parts, [I.copy()]), pdata(parts, [J.copy()]), pdata(parts, [V]),
                                            rows, cols, ids="global")
            check_findnz(pamd, A, [M], what=f"uniform {uniform}")
            pamd.fillstored_(A, 2.5)
            check_findnz(pamd, A, [pamd.CSC(M.m, M.n, M.colptr, M.rowval, np.full(len(M.nzval), 2.5))],
                         kinds=[("all", "local")])
            traffic[uniform] = A.values.parts[0].traffic()["value_bytes"]
    assert traffic[1] != traffic[0]  # the first matrix had the uniform layout


@pytest.mark.parametrize("name,f32_rows", sorted(MUST_SHOW))
def test_round_trip(be, pamd, name, f32_rows):
    dtype = np.dtype(name).type
    c = fe_case(pamd, be, dtype, f32_rows)
    A, parts = c.A, c.parts
    with knob(pamd, "f32_rows", f32_rows):
        B = pamd.PSparseMatrix.from_coo(pamd.findnz(A, "all", "local"), None, None, c.rows, c.cols, ids="local")
    for Ma, Mb in zip(A.values.parts, B.values.parts):
        assert Ma.csc_nnz == Mb.csc_nnz
        assert same_bits(Ma.get_values(), Mb.get_values())
    rng = np.random.default_rng(31)
    x = pamd.PVector.from_host(pdata(parts, [entries(dtype, s.num_lids, rng) for s in c.cols.partition.parts]), c.cols)
    for fmt in (1, 0):
        with knob(pamd, "spmv_format", fmt):
            ya, yb = pamd.PVector.undef(c.rows, dtype), pamd.PVector.undef(c.rows, dtype)
            pamd.mul_(ya, A, x)
            pamd.mul_(yb, B, x)
            for a, b in zip(ya.owned_values().parts, yb.owned_values().parts):
                assert bits(a).any() and same_bits(a, b), fmt


# ---------------------------------------------------------------------------
# 5. a CSR parent whose rows are not column-sorted

@pytest.mark.parametrize("order", ["diag_first", "descending"])
@pytest.mark.parametrize("Bi", [0, 1])
def test_unsorted_csr(be, pamd, O, Bi, order):
    n = 300
    rowptr, colval, V, _, _, _ = MC.unsorted_csr(n, (-40, -3, 0, 1, 2, 17), Bi, order, np.float64)
    M = pamd.CSR(Bi, n, n, rowptr, colval, V)
    i, j = nz_order(M)
    assert (np.diff(j)[np.diff(i) == 0] < 0).any()  # the rows are not column-sorted
    parts = be.get_part_ids(1)
    rows = pamd.prange_linear(parts, n)
    A = pamd.PSparseMatrix.from_csr(pdata(parts, [M]), rows, rows)
    # the deviation: every stored entry exactly once, in ascending (row, col)
    check_findnz(pamd, A, [M], order=[np.lexsort((j, i))])
    I, J, _ = pamd.findnz(A, "all", "local").to_host()
    key = I.parts[0] * (n + 1) + J.parts[0]
    assert len(key) == len(V) and (np.diff(key) > 0).all()
    # gather(A) does not see the difference: sparsecsr sorts the rows
    orows = oracle_range(O, rows)
    want = R.gather_matrix(O.PSparseMatrix(O.PData([oracle_matrix(O, M)]), orows, orows)).values.parts[0]
    got = pamd.gather(A)
    assert got.values.parts[0].csr_bi == Bi == want.Bi
    gi, gj, gv = (x.parts[0] for x in pamd.findnz(got, "all", "local").to_host())
    wi, wj, wv = R.entries(want)
    assert np.array_equal(gi, wi) and np.array_equal(gj, wj) and same_bits(gv, wv)


# ---------------------------------------------------------------------------
# 6. gather(b) and scatter_

def vector_ranges(pamd, O, be, case):
    """(parts, the range, its oracle twin) of a 4-part case"""
    if case == "periodic":  # with_ghost: owned and ghost lids interleave
        parts, shape = be.get_part_ids((2, 2)), (6, 5)
        rows = pamd.prange_cartesian(parts, shape, with_ghost=True, isperiodic=(True, False))
        orows = O.prange_cartesian(O.get_part_ids((2, 2)), shape, with_ghost=True, isperiodic=(True, False))
        s = rows.partition.parts[0]
        assert s.num_hids > 0 and s.hid_to_lid.min() < s.oid_to_lid.max()  # interleaved
    else:
        parts = be.get_part_ids(4)
        rows, orows = pamd.prange_linear(parts, case), O.prange_linear(O.get_part_ids(4), case)
    for s, t in zip(rows.partition.parts, orows.partition.parts):
        assert s.lid_to_gid.tolist() == t.lid_to_gid and s.oid_to_lid.tolist() == t.oid_to_lid
    return parts, rows, orows


def run_vector_case(pamd, O, be, case, dtype):
    parts, rows, orows = vector_ranges(pamd, O, be, case)
    rng = np.random.default_rng(17)
    vals = [entries(dtype, s.num_lids, rng) for s in rows.partition.parts]
    for v, s in zip(vals, rows.partition.parts):
        if s.num_oids:
            v[s.oid_to_lid[0] - 1] = minus_zero(dtype)  # one -0.0 among the owned values of every part
    b = pamd.PVector.from_host(pdata(parts, vals), rows)
    ob = O.PVector(O.PData([MC._to_oracle(O, v) for v in vals], orows.partition.shape), orows)
    rows_in_main = pamd.to_main(rows)
    lids = [s.num_lids for s in rows_in_main.partition.parts]
    assert lids[0] == len(rows) and lids[1:] == [s.num_oids for s in rows.partition.parts[1:]]
    if case == 2:
        assert 0 in lids  # a part without a lid in the range in MAIN
    if case in (2, 3):
        assert 0 in [s.num_oids for s in rows.partition.parts]  # a part that owns nothing
    want = R.gather_vector(ob)
    for bm in (pamd.gather(b), pamd.gather(b, rows_in_main), pamd.gather(b, rows_in_main)):  # the range is reused
        assert bm.dtype == np.dtype(dtype)
        for g, w in zip(bm.to_host().parts, want.values.parts):  # ghosts zeroed after assemble! included
            assert same_bits(g, R.as_array(w))
    # the reference adds what arrives onto zero(T): a -0.0 owned by MAIN stays, one owned elsewhere arrives as +0.0
    main = bm.to_host().parts[0]
    for s in rows.partition.parts:
        if s.num_oids:
            z = main[s.lid_to_gid[s.oid_to_lid[0] - 1] - 1]
            assert is_minus_zero(z) if s.part == pamd.MAIN else is_plus_zero(z)
    # scatter_(c, gather(b)) restores the owned values; c's ghosts stay
    start = [entries(dtype, s.num_lids, rng) for s in rows.partition.parts]
    c = pamd.PVector.from_host(pdata(parts, start), rows)
    oc = O.PVector(O.PData([MC._to_oracle(O, v) for v in start], orows.partition.shape), orows)
    R.scatter(oc, R.gather_vector(ob))
    assert pamd.scatter_(c, pamd.gather(b, rows_in_main)) is c
    for g, w, v0, c0, s in zip(c.to_host().parts, oc.values.parts, vals, start, rows.partition.parts):
        assert same_bits(g, R.as_array(w))
        own, gh = s.oid_to_lid - 1, s.hid_to_lid - 1
        if s.part == pamd.MAIN:
            assert same_bits(g[own], v0[own])
        else:  # (a -0.0 came back from MAIN as +0.0)
            assert np.array_equal(g[own], v0[own]) and same_bits(g[own][1:], v0[own][1:])
        assert same_bits(g[gh], c0[gh])


@pytest.mark.parametrize("case", [2, 3, 10, "periodic"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_gather_and_scatter_of_a_vector(be, pamd, O, dtype, case):
    run_vector_case(pamd, O, be, case, dtype)


# ---------------------------------------------------------------------------
# 7. gather(A)

def kat(pamd, O, be, parent="csc"):
    """the reference's 4-part 10 x 10 matrix (test_interfaces.jl:686-697) on
    the device and in the oracle, with y = PVector(1.0, A.rows)"""
    k = GOLD
    parts = be.get_part_ids(4)
    mk = lambda key, t: pdata(parts, [np.array(v, t) for v in k[key]])
    I, J, V = mk("I", np.int64), mk("J", np.int64), mk("V", np.float64)
    rows, cols = pamd.prange_linear(parts, k["n"]), pamd.prange_linear(parts, k["n"])
    pamd.add_gids_(rows, I)
    pamd.add_gids_(cols, J)
    A = pamd.PSparseMatrix.from_coo(mk("I", np.int64), mk("J", np.int64), V, rows, cols, ids="global",
                                    init=init_of(pamd, parent))
    oparts = O.get_part_ids(4)
    oI, oJ = O.PData([list(v) for v in k["I"]]), O.PData([list(v) for v in k["J"]])
    oV = O.PData([np.array(v) for v in k["V"]])
    orows, ocols = O.prange_linear(oparts, k["n"]), O.prange_linear(oparts, k["n"])
    O.add_gids_(orows, oI)
    O.add_gids_(ocols, oJ)
    oinit = None if parent == "csc" else (lambda i, j, v, m, n: O.sparse_csr(parent, i, j, v, m, n))
    OA = O.psparse_from_coo(oI, oJ, oV, orows, ocols, ids="global", init=oinit)
    return parts, A, OA, (I, J, V)


def check_gathered(pamd, got, want, parent):
    """MAIN's pattern and values equal the restatement's; the other parts are empty"""
    gi, gj, gv = pamd.findnz(got, "all", "local").to_host()
    wi, wj, wv = R.entries(want.values.parts[0])
    assert np.array_equal(gi.parts[0], wi) and np.array_equal(gj.parts[0], wj) and same_bits(gv.parts[0], wv)
    for M in got.values.parts:
        assert M.csr_bi == (None if parent == "csc" else parent)
    for p, (M, w, r, c) in enumerate(zip(got.values.parts, want.values.parts, got.rows.partition.parts,
                                         got.cols.partition.parts)):
        if p > 0:
            assert M.info()["nnz"] == 0 and M.csc_nnz == 0 and len(gi.parts[p]) == 0
            assert M.info()["nrows"] == 0 and (r.num_lids, c.num_lids) == (w.m, w.n)
    assert all(len(t) == 0 for t in got.exchanger.parts_rcv.parts)  # the empty exchanger


def run_gather_kat(pamd, O, be, parent):
    parts, A, OA, _ = kat(pamd, O, be, parent)
    want = R.gather_matrix(OA)
    got = pamd.gather(A)
    check_gathered(pamd, got, want, parent)
    assert got.values.parts[0].csc_nnz == 15
    # through ranges the caller supplies, twice
    rm, cm = pamd.to_main(A.rows), pamd.to_main(A.cols)
    for _ in range(2):
        check_gathered(pamd, pamd.gather(A, rm, cm), want, parent)


@pytest.mark.parametrize("parent", PARENTS, ids=lambda p: f"parent_{p}")
def test_gather_matrix_kat(be, pamd, O, parent):
    run_gather_kat(pamd, O, be, parent)


def test_gather_matrix_fe(be, pamd, O):
    c = fe_case(pamd, be, np.float64)
    OA = O.PSparseMatrix(O.PData([oracle_matrix(O, M) for M in c.csc]), oracle_range(O, c.rows),
                         oracle_range(O, c.cols))
    want = R.gather_matrix(OA)
    got = pamd.gather(c.A)
    check_gathered(pamd, got, want, "csc")
    assert got.values.parts[0].csc_nnz == sum(M.info()["nnz"] for M in c.A.values.parts)


# ---------------------------------------------------------------------------
# 8. solves

def residual(pamd, A, x, y):
    r = pamd.matvec(A, x)
    pamd.sub_(r, y)
    return pamd.norm(r)


def run_solves_kat(pamd, O, be):
    parts, A, OA, (I, J, V) = kat(pamd, O, be)
    tol = GOLD["residual_tol"]
    y = pamd.PVector.full(1.0, A.rows)
    x = pamd.solve(A, y)
    assert isinstance(x, pamd.PVector) and x.rows is A.cols and x.dtype == np.float64
    res = {"solve": residual(pamd, A, x, y)}
    F = pamd.lu(A)
    assert isinstance(F, pamd.PLU)
    x.fill_(0)
    assert pamd.ldiv_(x, F, y) is x
    res["lu + ldiv_"] = residual(pamd, A, x, y)
    assert pamd.lu_(F, A) is F
    x.fill_(0)
    pamd.ldiv_(x, F, y)
    res["lu_ + ldiv_"] = residual(pamd, A, x, y)
    print(res)
    for k, v in res.items():
        assert v < tol, k
    # other values in the same pattern: the old factors no longer solve the system, lu_ follows
    rows_in_main = F.rows
    pamd.fillstored_(A, 0)
    pamd.add_coo_(A, I, J, pamd.map_parts(lambda v: 3.0 * v + 0.25, V), ids="global")
    x.fill_(0)
    pamd.ldiv_(x, F, y)
    stale = residual(pamd, A, x, y)
    print("old factors on the new matrix:", stale)
    assert stale >= tol
    pamd.lu_(F, A)
    assert F.rows is rows_in_main  # the ranges in MAIN are reused
    x.fill_(0)
    pamd.ldiv_(x, F, y)
    assert residual(pamd, A, x, y) < tol
    z = pamd.zerox(A, y)
    assert z.rows is A.cols and z.dtype == np.float64 and all(not v.any() for v in z.to_host().parts)
    z32 = pamd.zerox(A, pamd.PVector.full(1.0, A.rows, dtype=np.float32))
    assert z32.dtype == np.float64  # result_type of the two element types


def test_solves_kat(be, pamd, O):
    run_solves_kat(pamd, O, be)


@pytest.mark.parametrize("shape", [4, (2, 2, 1)])
def test_solve_fdm_equals_the_host_routine(be, pamd, O, shape):
    """fdm_problem(parts, nx=6), 216 unknowns: x equals the same _main_lu
    applied on the host to the restatement's gathered matrix and vector, bit
    for bit (the same input bits into the same deterministic host routine)"""
    parts = be.get_part_ids(shape)
    A, b, _, _ = pamd.drivers.fdm_problem(parts, 6)
    OA, ob, _, _ = O.fdm_problem(O.get_part_ids(shape), nx=6)
    assert len(A.rows) == 216
    lu = lambda m, n, colptr, rowval, nzval: pamd.pvector._main_lu(pamd.CSC(m, n, colptr, rowval, nzval))
    want = R.solve(OA, ob, lu)
    x = pamd.solve(A, b)
    for g, w, s in zip(x.to_host().parts, want.values.parts, A.cols.partition.parts):
        own = s.oid_to_lid - 1
        assert same_bits(g[own], R.as_array(w)[own])
        assert not g[s.hid_to_lid - 1].any()  # the ghosts of x are not touched
    assert residual(pamd, A, x, b) < 1e-9 * max(1.0, pamd.norm(b))


def test_solve_keeps_float32(be, pamd):
    parts = be.get_part_ids(4)
    A, b, _, _ = pamd.drivers.fdm_problem(parts, 4, dtype=np.float32)
    x = pamd.solve(A, b)
    assert x.dtype == np.float32
    # 64 unknowns, entries up to 6/h^2 = 13.5: a backward-stable solve leaves about n * eps * |A| |x|
    assert residual(pamd, A, x, b) < 64 * np.finfo(np.float32).eps * 13.5 * 7 * 4.0


# ---------------------------------------------------------------------------
# 9. the same over the RCCL transport

def test_rccl_transport(be_rccl, pamd, O):
    for dtype in (np.float64, np.complex64):
        run_vector_case(pamd, O, be_rccl, 10, dtype)
        run_vector_case(pamd, O, be_rccl, 2, dtype)
    run_gather_kat(pamd, O, be_rccl, "csc")
    run_gather_kat(pamd, O, be_rccl, 1)
    run_solves_kat(pamd, O, be_rccl)


# ---------------------------------------------------------------------------
# 10. to_gids_

def test_to_gids_round_trip(be, pamd):
    parts = be.get_part_ids(4)
    cols = pamd.prange_linear(parts, 40)
    pamd.add_gids_(cols, pamd.map_parts(lambda p: np.array([1, 40, 17, 23, 5 * p], np.int64), parts))
    assert all(s.num_hids > 0 for s in cols.partition.parts)
    lids = pamd.map_parts(lambda s: np.random.default_rng(s.part).permutation(s.num_lids).astype(np.int64) + 1,
                          cols.partition)
    keep = [a.copy() for a in lids.parts]
    g = pamd.to_gids_(lids, cols)  # in place, through the device's lid_to_gid
    assert all(a is b for a, b in zip(g.parts, lids.parts))
    assert all(np.array_equal(a, s.lid_to_gid[k - 1]) for a, k, s in zip(g.parts, keep, cols.partition.parts))
    # back through the device gid table (the device path of to_lids!)
    from pamd.device import device_to_lids
    for a, k, s in zip(g.parts, keep, cols.partition.parts):
        assert np.array_equal(device_to_lids(be.context(s.part), s, a), k)
    for wrong in (0, -3, None):
        bad = pamd.map_parts(lambda s: np.array([1, (s.num_lids + 1) if wrong is None else wrong, 2], np.int64),
                             cols.partition)
        before = [a.copy() for a in bad.parts]
        with pytest.raises(pamd.PAError, match="out of range"):
            pamd.to_gids_(bad, cols)
        assert all(np.array_equal(a, b) for a, b in zip(bad.parts, before))


# ---------------------------------------------------------------------------
# 11. errors

def test_errors(be, pamd, O):
    parts = be.get_part_ids((2, 2, 1))
    S = pamd.drivers.stencil_operator(parts, (12, 10, 9), 27)
    with pytest.raises(pamd.PAError, match="not built from a CSC pattern"):
        pamd.findnz(S)
    with pytest.raises(pamd.PAError):
        pamd.gather(S)
    _, A, _, _ = kat(pamd, O, be)
    with pytest.raises(ValueError):
        pamd.findnz(A, rows="ghost")
    with pytest.raises(ValueError):
        pamd.findnz(A, ids="gids")
    other = pamd.to_main(pamd.prange_linear(be.get_part_ids(4), 12))  # 12 gids: not the matrix's
    shifted = pamd.to_main(pamd.prange_noids(be.get_part_ids(4), pamd.map_parts(lambda p: [1, 2, 3, 4][p - 1],
                                                                               be.get_part_ids(4))))
    assert len(shifted) == len(A.rows)  # the same gids over other owners
    for wrong in (other, shifted):
        with pytest.raises(ValueError, match="range in MAIN"):
            pamd.gather(A, wrong, None)
        with pytest.raises(ValueError, match="range in MAIN"):
            pamd.gather(A, None, wrong)
        with pytest.raises(ValueError, match="range in MAIN"):
            pamd.gather(pamd.PVector.full(1.0, A.rows), wrong)
    F = pamd.lu(A)
    y12 = pamd.PVector.full(1.0, pamd.prange_linear(be.get_part_ids(4), 12))
    x = pamd.zerox(A, pamd.PVector.full(1.0, A.rows))
    with pytest.raises(ValueError, match="range in MAIN"):
        pamd.ldiv_(x, F, y12)
    with pytest.raises(ValueError, match="range in MAIN"):
        pamd.ldiv_(y12, F, pamd.PVector.full(1.0, A.rows))
    assert all(not v.any() for v in x.to_host().parts)  # nothing was written
