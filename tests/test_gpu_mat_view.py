"""local_view / global_view of a PSparseMatrix on the device (Interfaces.jl:
2277-2298): pa_mat_scatter / pa_mat_gather against the sequential
restatement of tests/mat_view_ref.py.  Every comparison is bit for bit (sign
of zero included) on DeviceMatrix.get_values(), nonzeros(A) in the parent's
order; the only exception is the payload of a NaN the hardware generates
(Inf - Inf), where the positions of the NaNs are compared."""
import contextlib

import numpy as np
import pytest

import mat_view_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
NL, N = 200, 70001  # lids of the part; triplets: more than one grid pass (65,536 threads), no multiple of 64


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


def pdata(parts, values):
    return type(parts)(parts.backend, parts.part_ids, list(values), parts.shape)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


@contextlib.contextmanager
def knob(pamd, key, value):
    prev = pamd._lib.tune(key, value)
    try:
        yield
    finally:
        pamd._lib.tune(key, prev)


def one_part_rows(pamd, be, nl, seed=3):
    """one part whose lids are a permutation of the gids 1..nl (gid != lid)"""
    parts = be.get_part_ids(1)
    gids = np.random.default_rng(seed).permutation(nl).astype(np.int64) + 1
    part = pdata(parts, [pamd.IndexSet(1, gids, np.ones(nl, np.int32))])
    return parts, pamd.prange_from_partition(nl, part, ghost=False)


def entries(dtype, n, rng):
    """uniform(-1, 1) * 10^k, k in -3..3"""
    f = lambda: rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-3, 4, n)
    V = f()
    if np.dtype(dtype).kind == "c":
        V = V + 1j * f()
    return V.astype(dtype)


def pattern_of(M):
    """the reference's Pattern of a host CSC / CSR"""
    if hasattr(M, "rowptr"):
        return R.Pattern(M.m, M.n, M.rowptr, M.colval, "row", M.Bi)
    return R.Pattern(M.m, M.n, M.colptr, M.rowval, "col", 1)


# ---------------------------------------------------------------------------
# 1. order-sensitive accumulation

def irregular_triplets(nl, rng):
    """(I, J) lids of about 7.5 * nl distinct entries, 1..14 per row"""
    lens = rng.integers(1, 15, nl)
    I = np.repeat(np.arange(1, nl + 1), lens)
    J = np.concatenate([rng.choice(nl, size=k, replace=False) + 1 for k in lens])
    return I.astype(np.int64), J.astype(np.int64)


_ORDER = {}


def order_case(pamd, dtype, parent):
    """(host parent, triplet lids I, J, values V, expected nzval, share of the
    stored entries whose bits change when the triplets are summed in reverse
    input order); computed once per element type and parent kind"""
    key = (dtype, parent)
    if key not in _ORDER:
        rng = np.random.default_rng(5)
        I0, J0 = irregular_triplets(NL, rng)
        V0 = entries(dtype, len(I0), rng)
        M = pamd.compresscoo(I0, J0, V0, NL, NL) if parent == "csc" else pamd.sparsecsr(parent, I0, J0, V0, NL, NL)
        pat = pattern_of(M)
        assert 1400 <= pat.nnz <= 1600
        ri, ci = pat.rows_cols()
        k = rng.integers(0, pat.nnz, size=N)
        I, J, V = ri[k] + 1, ci[k] + 1, entries(dtype, N, rng)
        want = R.scatter_add(np.zeros(pat.nnz, dtype), pat, I, J, V)
        rev = R.scatter_add(np.zeros(pat.nnz, dtype), pat, I[::-1], J[::-1], V[::-1])
        changed = (R.bits(want).reshape(pat.nnz, -1) != R.bits(rev).reshape(pat.nnz, -1)).any(axis=1).mean()
        for a in (I, J, V, want):
            a.setflags(write=False)
        _ORDER[key] = M, I, J, V, want, changed
    return _ORDER[key]


def run_order_case(be, pamd, dtype, parent, idkind, wide):
    M, I, J, V, want, changed = order_case(pamd, dtype, parent)
    print(f"{np.dtype(dtype).name} {parent}: reverse order changes {100 * changed:.1f} % of the stored entries")
    assert changed >= 0.5  # an unordered sum would not reproduce `want`
    parts, rows = one_part_rows(pamd, be, NL)
    s = rows.partition.parts[0]
    build = pamd.PSparseMatrix.from_csc if parent == "csc" else pamd.PSparseMatrix.from_csr
    A = build(pdata(parts, [M]), rows, rows)
    if idkind == "global":
        Ii, Ji, ids = s.lid_to_gid[I - 1].copy(), s.lid_to_gid[J - 1].copy(), "global"
    else:
        t = np.int32 if idkind == "local32" else np.int64
        Ii, Ji, ids = I.astype(t), J.astype(t), "local"
    I0, J0 = Ii.copy(), Ji.copy()
    pamd.fillstored_(A, 0)
    with knob(pamd, "scatter_wide", wide):
        assert pamd.add_coo_(A, pdata(parts, [Ii]), pdata(parts, [Ji]), pdata(parts, [V]), ids=ids) is A
    assert same_bits(A.values.parts[0].get_values(), want)
    assert np.array_equal(Ii, I0) and np.array_equal(Ji, J0)  # the matrix views do not call to_lids!


@pytest.mark.parametrize("wide", [0, 1], ids=["keys32", "keys64"])
@pytest.mark.parametrize("idkind", ["local32", "local64", "global"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_order_sensitive_accumulation(be, pamd, dtype, idkind, wide):
    run_order_case(be, pamd, dtype, "csc", idkind, wide)


@pytest.mark.parametrize("wide", [0, 1], ids=["keys32", "keys64"])
@pytest.mark.parametrize("idkind", ["local32", "local64", "global"])
@pytest.mark.parametrize("Bi", [0, 1])
def test_order_sensitive_accumulation_csr_parent(be, pamd, Bi, idkind, wide):
    run_order_case(be, pamd, np.float64, Bi, idkind, wide)


# ---------------------------------------------------------------------------
# 2. every place a value can live

GRID = (30, 12, 6)  # x-lines of 30 rows (no divisor of a slice's 128 or 256 rows), 12 per z-plane, 3 planes per part
LONG = (300, 411)   # entries of the two long rows of each part (more than max(256, 8 x 27))


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


class Case2:
    """A 27-point operator over two parts as an FE assembly leaves it: each
    part stores its owned rows and the rows of its ghost nodes (the plane of
    the other part next to the interface), plus two long owned rows.
    parent: "csc", or the Bi of SparseMatrixCSR{Bi} parents; shuffle_row_lids:
    the lids of rows in a random order, owned and ghost lids mixed (those of
    cols stay owned-then-ghost, which the pattern and delta16 slices need)."""

    def __init__(self, pamd, be, dtype, f32_rows=0, seed=29, parent="csc", shuffle_row_lids=False):
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
            i, j = i[keep], j[keep]
            for g, k in zip(rng.choice(own, size=len(LONG), replace=False), LONG):
                i = np.concatenate([i, np.full(k, g)])
                j = np.concatenate([j, rng.choice(nodes, size=k, replace=False)])
            o = rng.permutation(len(i))
            Ig.append(i[o])
            Jg.append(j[o])
        pamd.add_gids_(rows, pdata(parts, Ig))
        pamd.add_gids_(cols, pdata(parts, Jg))
        if shuffle_row_lids:
            order = [rng.permutation(s.num_lids) for s in rows.partition.parts]
            rows = pamd.prange_from_partition(n, pdata(parts, [
                pamd.IndexSet(s.part, s.lid_to_gid[o], s.lid_to_part[o]) for s, o in zip(rows.partition.parts, order)]))
        self.rows, self.cols = rows, cols
        V0 = [entries(dtype, len(i), rng) for i in Ig]
        with knob(pamd, "f32_rows", f32_rows):
            self.A = pamd.PSparseMatrix.from_coo(pdata(parts, [i.copy() for i in Ig]),
                                                 pdata(parts, [j.copy() for j in Jg]), pdata(parts, V0), rows, cols,
                                                 ids="global", init=None if parent == "csc" else pamd.csr_init(parent))
        # the host restatement of sparse(I, J, V) / sparsecsr: the parents' patterns
        compress = pamd.compresscoo if parent == "csc" else pamd.csr_init(parent)
        self.csc = [compress(r.to_lids(i), c.to_lids(j), v, r.num_lids, c.num_lids)
                    for r, c, i, j, v in zip(rows.partition.parts, cols.partition.parts, Ig, Jg, V0)]
        self.pat = [pattern_of(M) for M in self.csc]
        # shuffled triplets: every stored entry once, and as many again drawn with repetition
        self.I, self.J, self.V, self.want = [], [], [], []
        for pat in self.pat:
            k = np.concatenate([np.arange(pat.nnz), rng.integers(0, pat.nnz, size=pat.nnz)])
            k = k[rng.permutation(len(k))]
            ri, ci = pat.rows_cols()
            self.I.append(ri[k] + 1)
            self.J.append(ci[k] + 1)
            self.V.append(entries(dtype, len(k), rng))
            self.want.append(R.scatter_add(np.zeros(pat.nnz, dtype), pat, self.I[-1], self.J[-1], self.V[-1]))

    def gids(self):
        return ([r.lid_to_gid[i - 1] for r, i in zip(self.rows.partition.parts, self.I)],
                [c.lid_to_gid[j - 1] for c, j in zip(self.cols.partition.parts, self.J)])

    def counters(self):
        out = {}
        for M in self.A.values.parts:
            info = M.info()
            info["ghost_nnz"] = M.csc_nnz - info["nnz"]
            for k, v in info.items():
                out[k] = out.get(k, 0) + v
        return out


_CASE2 = {}


def case2(pamd, be, dtype, f32_rows=0):
    if (dtype, f32_rows) not in _CASE2:
        _CASE2[dtype, f32_rows] = Case2(pamd, be, dtype, f32_rows)
    return _CASE2[dtype, f32_rows]


# The structures each matrix must show, so that a layout change cannot empty
# the test.  Float64 has 2 rows per lane; Float32 4, which the build of this
# matrix turns into 2 (few pattern slices) unless f32_rows 4 keeps them: then
# the rows of its delta16 slices are interleaved.
MUST_SHOW = {
    ("float64", 0): ("pattern_slices", "side_rows", "triple_sell_slices", "tri_slices", "pair_slices", "long_rows",
                     "ghost_nnz"),
    ("float32", 0): ("pattern_slices", "side_rows", "triple_sell_slices", "tri_slices", "long_rows", "ghost_nnz"),
    ("float32", 4): ("pattern_slices", "side_rows", "delta16_slices", "long_rows", "ghost_nnz"),
}


@pytest.mark.parametrize("name,f32_rows", sorted(MUST_SHOW))
def test_every_place_a_value_can_live(be, pamd, name, f32_rows):
    dtype = np.dtype(name).type
    c = case2(pamd, be, dtype, f32_rows)
    parts, A = c.parts, c.A
    cnt = c.counters()
    print({k: cnt[k] for k in ("nrows", "nslices", "nnz", "pattern_slices", "regular_rows", "side_rows",
                               "delta16_slices", "triple_sell_slices", "tri_slices", "pair_slices", "long_rows",
                               "ghost_nnz")})
    for key in MUST_SHOW[name, f32_rows]:
        assert cnt[key] > 0, key
    # rows per slice: 256 with 4 rows per lane, else 128
    assert cnt["nslices"] == 2 * -(-(cnt["nrows"] // 2) // (256 if f32_rows == 4 else 128))
    assert all(s.num_hids > 0 for s in c.rows.partition.parts)
    Ig, Jg = c.gids()
    pamd.fillstored_(A, 0)
    pamd.add_coo_(A, pdata(parts, Ig), pdata(parts, Jg), pdata(parts, c.V), ids="global")
    got = [M.get_values() for M in A.values.parts]
    for g, w in zip(got, c.want):  # (a)
        assert same_bits(g, w)
    # (b) the SpMV layouts' copies follow: a matrix built from the same
    # pattern with these values multiplies to the same bits
    with knob(pamd, "f32_rows", f32_rows):
        B = pamd.PSparseMatrix.from_csc(pdata(parts, [pamd.CSC(M.m, M.n, M.colptr, M.rowval, g)
                                                      for M, g in zip(c.csc, got)]), c.rows, c.cols)
    rng = np.random.default_rng(31)
    x = pamd.PVector.from_host(pdata(parts, [entries(dtype, s.num_lids, rng) for s in c.cols.partition.parts]), c.cols)
    for fmt in (1, 0):
        with knob(pamd, "spmv_format", fmt):
            ya, yb = pamd.PVector.undef(c.rows, dtype), pamd.PVector.undef(c.rows, dtype)
            pamd.mul_(ya, A, x)
            pamd.mul_(yb, B, x)
            for a, b in zip(ya.owned_values().parts, yb.owned_values().parts):
                assert R.bits(a).any() and same_bits(a, b), fmt
    # (c) assemble!(A) moves the ghost rows' values as it does after an upload
    pamd.assemble_(A)
    pamd.assemble_(B)
    for Ma, Mb, g in zip(A.values.parts, B.values.parts, got):
        assert same_bits(Ma.get_values(), Mb.get_values())
        assert not same_bits(Ma.get_values(), g)  # (the ghost rows were sent and zeroed)


def test_uniform_layout_follows(be, pamd):
    """The uniform layout of short Float64 pattern rows (FD7) is a copy of
    the values too: with it and without it, mul! after a scatter equals mul!
    of a matrix built with the new values."""
    grid = (12, 11, 9)
    parts = be.get_part_ids((1, 1, 1))
    rows, cols = pamd.drivers.stencil_partition(parts, grid, 7)
    s = rows.partition.parts[0]
    own = s.lid_to_gid[s.oid_to_lid - 1]
    i, J, V = pamd.drivers.stencil_entries(7, grid, own)
    I = own[i]
    rng = np.random.default_rng(37)
    traffic = {}
    for uniform in (1, 0):
        with knob(pamd, "spmv_uniform", uniform):
            A = pamd.PSparseMatrix.from_coo(pdata(parts, [I.copy()]), pdata(parts, [J.copy()]), pdata(parts, [V]),
                                            rows, cols, ids="global")
            M = pamd.compresscoo(s.to_lids(I), cols.partition.parts[0].to_lids(J), V, s.num_lids, s.num_lids)
            pat = pattern_of(M)
            ri, ci = pat.rows_cols()
            k = rng.permutation(np.concatenate([np.arange(pat.nnz), rng.integers(0, pat.nnz, size=pat.nnz)]))
            W = entries(np.float64, len(k), rng)
            want = R.scatter_add(np.zeros(pat.nnz), pat, ri[k] + 1, ci[k] + 1, W)
            pamd.fillstored_(A, 0)
            pamd.local_view(A, rows, cols).parts[0].add_(ri[k] + 1, ci[k] + 1, W)
            assert same_bits(A.values.parts[0].get_values(), want)
            B = pamd.PSparseMatrix.from_csc(pdata(parts, [pamd.CSC(M.m, M.n, M.colptr, M.rowval, want)]), rows, cols)
            x = pamd.PVector.from_host(pdata(parts, [entries(np.float64, s.num_lids, rng)]), cols)
            ya, yb = pamd.PVector.undef(rows), pamd.PVector.undef(rows)
            pamd.mul_(ya, A, x)
            pamd.mul_(yb, B, x)
            assert same_bits(ya.to_host().parts[0], yb.to_host().parts[0])
            traffic[uniform] = A.values.parts[0].traffic()["value_bytes"]
    assert traffic[1] != traffic[0]  # the first matrix had the uniform layout


# ---------------------------------------------------------------------------
# 3. views

def small_case(pamd, be, dtype, rng):
    """two parts whose owned and ghost lids interleave (no pattern layout,
    rows through oid_to_lid), every part storing rows of its ghosts"""
    parts = be.get_part_ids((2, 1))
    rows = pamd.prange_cartesian(parts, (9, 7), with_ghost=True)
    # about 70 % of the 9-point pattern, chosen once for all parts: a ghost
    # row's entries then exist in its owner's matrix too (matrix_exchanger)
    g = np.arange(63)
    near = (np.abs(g[:, None] % 9 - g[None, :] % 9) <= 1) & (np.abs(g[:, None] // 9 - g[None, :] // 9) <= 1)
    GI, GJ = np.nonzero(near & (rng.random((63, 63)) < 0.7))
    GI, GJ = GI + 1, GJ + 1
    csc = []
    for s in rows.partition.parts:
        mine = np.isin(GI, s.lid_to_gid) & np.isin(GJ, s.lid_to_gid)
        I, J = s.to_lids(GI[mine]), s.to_lids(GJ[mine])
        csc.append(pamd.compresscoo(I, J, entries(dtype, len(I), rng), s.num_lids, s.num_lids))
    return parts, rows, csc


def absent(pat, rng, n):
    """n (i, j) lids the pattern does not store"""
    out = []
    while len(out) < n:
        i, j = int(rng.integers(1, pat.m + 1)), int(rng.integers(1, pat.n + 1))
        if pat.nzindex([i], [j])[0] < 0:
            out.append((i, j))
    return np.array(out, dtype=np.int64).T


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_views_get_set_add(be, pamd, dtype):
    rng = np.random.default_rng(41)
    parts, rows, csc = small_case(pamd, be, dtype, rng)
    A = pamd.PSparseMatrix.from_csc(pdata(parts, csc), rows, rows)
    assert all(not np.array_equal(s.oid_to_lid, np.arange(1, s.num_oids + 1)) for s in rows.partition.parts)
    other = pamd.prange_cartesian(parts, (9, 7))  # other lids: no ghosts
    lv, gv = pamd.local_view(A, rows, rows), pamd.global_view(A, rows, rows)
    assert isinstance(lv.parts[0], pamd.MatrixView)
    mv = pamd.local_view(A, other, other)
    for p, (s, M, o) in enumerate(zip(rows.partition.parts, csc, other.partition.parts)):
        pat = pattern_of(M)
        ri, ci = pat.rows_cols()
        ghost_row = s.lid_to_part[ri] != s.part
        assert ghost_row.any() and not ghost_row.all()
        nz = M.nzval.copy()
        dm = A.values.parts[p]
        k = rng.integers(0, pat.nnz, size=2001)
        I, J, V = ri[k] + 1, ci[k] + 1, entries(dtype, 2001, rng)
        assert len(np.unique(I * 1000 + J)) < len(I)
        # set_: the last value of a repeated (i, j) stays; the ids stay as they are
        I0, J0 = I.copy(), J.copy()
        assert lv.parts[p].set_(I, J, V) is lv.parts[p]
        assert np.array_equal(I, I0) and np.array_equal(J, J0)
        nz = R.scatter_set(nz, pat, I, J, V)
        assert same_bits(dm.get_values(), nz)
        # the same through global ids, then add_ on top in input order
        gi, gj = s.lid_to_gid[I - 1], s.lid_to_gid[J - 1]
        V2, V3 = entries(dtype, 2001, rng), entries(dtype, 2001, rng)
        gv.parts[p].set_(gi, gj, V2)
        nz = R.scatter_set(nz, pat, I, J, V2)
        assert same_bits(dm.get_values(), nz)
        gv.parts[p].add_(gi, gj, V3)
        nz = R.scatter_add(nz, pat, I, J, V3)
        assert same_bits(dm.get_values(), nz)
        # reads: stored entries (Int32 and Int64 lids, gids), among them unstored ones: exact zeros
        ai, aj = absent(pat, rng, 50)
        qi, qj = np.concatenate([I[:300], ai]), np.concatenate([J[:300], aj])
        o2 = rng.permutation(len(qi))
        qi, qj = qi[o2], qj[o2]
        want = R.gather(nz, pat, qi, qj)
        assert not R.bits(want[np.isin(o2, np.arange(300, 350))]).any()
        for t in (np.int32, np.int64):
            assert same_bits(lv.parts[p].get(qi.astype(t), qj.astype(t)), want)
        assert same_bits(gv.parts[p].get(s.lid_to_gid[qi - 1], s.lid_to_gid[qj - 1]), want)
        # the mapped kind: lids of `other`; those the matrix's ranges do not hold read zero
        oi = rng.integers(1, o.num_lids + 1, size=400)
        oj = rng.integers(1, o.num_lids + 1, size=400)
        want = R.gather(nz, pat, s.to_lids(o.lid_to_gid[oi - 1]), s.to_lids(o.lid_to_gid[oj - 1]))
        assert R.bits(want).any()
        assert same_bits(mv.parts[p].get(oi, oj), want)
        # ... entries it stores can be written through it
        hit = np.flatnonzero(R.bits(want).reshape(400, -1).any(axis=1))[:20]
        W = entries(dtype, len(hit), rng)
        mv.parts[p].add_(oi[hit], oj[hit], W)
        nz = R.scatter_add(nz, pat, s.to_lids(o.lid_to_gid[oi[hit] - 1]), s.to_lids(o.lid_to_gid[oj[hit] - 1]), W)
        assert same_bits(dm.get_values(), nz)
        # n = 0
        e = np.zeros(0, np.int64)
        assert lv.parts[p].get(e, e).shape == (0,) and gv.parts[p].get(e, e).shape == (0,)
        lv.parts[p].add_(e, e, np.zeros(0, dtype))
        gv.parts[p].set_(e, e, np.zeros(0, dtype))
        assert same_bits(dm.get_values(), nz)
    # lids of a range that A's ranges do not hold on the part (the linear
    # partition cuts the grid the other way): they read zero and cannot be written
    lin = pamd.prange_linear(parts, 63)
    wv = pamd.local_view(A, lin, lin).parts
    for p, (s, w) in enumerate(zip(rows.partition.parts, lin.partition.parts)):
        held = np.isin(w.lid_to_gid, s.lid_to_gid)
        assert held.any() and not held.all()
        miss, hold = np.flatnonzero(~held) + 1, np.flatnonzero(held) + 1
        before = A.values.parts[p].get_values()
        m = min(len(miss), len(hold))
        got = wv[p].get(np.concatenate([miss[:m], hold[:m]]), np.concatenate([hold[:m], miss[:m]]))
        assert got.dtype == np.dtype(dtype) and not R.bits(got).any()
        with pytest.raises(pamd.PAError, match="KeyError"):
            wv[p].set_(miss[:1], hold[:1], [1.0])
        with pytest.raises(pamd.PAError, match="BoundsError"):
            wv[p].get([w.num_lids + 1], [1])
        assert same_bits(A.values.parts[p].get_values(), before)
    with pytest.raises(NotImplementedError):
        pamd.global_view(A, other, A.cols)
    with pytest.raises(NotImplementedError):
        pamd.global_view(A, A.rows, other)


def test_edges(be, pamd):
    parts, rows = one_part_rows(pamd, be, 37)
    rng = np.random.default_rng(43)
    I0, J0 = irregular_triplets(37, rng)
    for dtype in (np.float32, np.float64):
        M = pamd.compresscoo(I0, J0, np.full(len(I0), -0.0, dtype), 37, 37)
        pat = pattern_of(M)
        ri, ci = pat.rows_cols()
        A = pamd.PSparseMatrix.from_csc(pdata(parts, [M]), rows, rows)
        dm, lv = A.values.parts[0], pamd.local_view(A, rows, rows).parts[0]
        # -0.0 added onto -0.0 stays -0.0; onto zero(T) it gives +0.0
        i, j = ri[[3, 5, 3]] + 1, ci[[3, 5, 3]] + 1
        W = np.array([-0.0, 1.5, -0.0], dtype)
        lv.add_(i, j, W)
        want = R.scatter_add(M.nzval.copy(), pat, i, j, W)
        got = dm.get_values()
        assert same_bits(got, want) and np.signbit(got[3]) and np.signbit(got[0]) and got[5] == 1.5
        pamd.fillstored_(A, 0)
        lv.add_(ri[[7]] + 1, ci[[7]] + 1, np.array([-0.0], dtype))
        assert not R.bits(dm.get_values()).any()
        lv.set_(ri[[7]] + 1, ci[[7]] + 1, np.array([-0.0], dtype))
        assert np.signbit(dm.get_values()[7]) and np.signbit(lv.get(ri[[7]] + 1, ci[[7]] + 1)[0])
    # NaN and Inf propagate
    M = pamd.compresscoo(I0, J0, np.zeros(len(I0)), 37, 37)
    pat = pattern_of(M)
    ri, ci = pat.rows_cols()
    A = pamd.PSparseMatrix.from_csc(pdata(parts, [M]), rows, rows)
    k = np.array([0, 1, 1, 2, 2, 3, 3, 1])
    V = np.array([np.nan, np.inf, 1.0, np.inf, -np.inf, -np.inf, 3.0, 2.0])
    s = rows.partition.parts[0]
    pamd.global_view(A, rows, rows).parts[0].add_(s.lid_to_gid[ri[k]], s.lid_to_gid[ci[k]], V)
    got = A.values.parts[0].get_values()
    with np.errstate(invalid="ignore"):
        want = R.scatter_add(np.zeros(pat.nnz), pat, ri[k] + 1, ci[k] + 1, V)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and list(np.flatnonzero(np.isnan(want))) == [0, 2]
    ok = ~np.isnan(want)
    assert same_bits(got[ok], want[ok]) and got[1] == np.inf and got[3] == -np.inf


def test_ghost_row_and_long_row_entries(be, pamd):
    c = case2(pamd, be, np.float64)
    lv = pamd.local_view(c.A, c.rows, c.cols).parts
    gv = pamd.global_view(c.A, c.rows, c.cols).parts
    for p, (r, cl, pat, M) in enumerate(zip(c.rows.partition.parts, c.cols.partition.parts, c.pat, c.A.values.parts)):
        ri, ci = pat.rows_cols()
        per_row = np.bincount(ri, minlength=pat.m)
        long_row = int(np.argmax(per_row))
        assert per_row[long_row] >= min(LONG) and r.lid_to_part[long_row] == r.part
        kl = np.flatnonzero(ri == long_row)[[0, 150, -1]]
        kg = np.flatnonzero(r.lid_to_part[ri] != r.part)[[0, 77, -1]]
        for k in (kl, kg):
            nz = M.get_values()
            i, j = ri[k] + 1, ci[k] + 1
            assert same_bits(lv[p].get(i, j), nz[k])
            gi, gj = r.lid_to_gid[i - 1], cl.lid_to_gid[j - 1]
            gv[p].set_(gi, gj, [1.5, -2.5, 3.25])
            gv[p].add_(gi[[0, 0]], gj[[0, 0]], [0.1, 0.2])
            nz[k] = [(1.5 + 0.1) + 0.2, -2.5, 3.25]
            assert same_bits(M.get_values(), nz) and same_bits(gv[p].get(gi, gj), nz[k])


def test_device_inputs_give_the_same_bits(be, pamd):
    """on_device = 1: I, J, V / out are device arrays of the caller"""
    parts, rows = one_part_rows(pamd, be, NL)
    s = rows.partition.parts[0]
    ctx = pamd.device.contexts(rows.partition)[0]
    DV = pamd.device.DeviceVector
    rng = np.random.default_rng(59)

    def on_device(a):
        words = np.ascontiguousarray(a).view(np.float32)
        holder = DV(ctx, np.float32, words.size)
        holder.upload(words)
        return holder, holder.as_array(a.dtype)

    for dtype in DTYPES:
        M, I, J, V, want, _ = order_case(pamd, dtype, "csc")
        pat = pattern_of(M)
        I, J, V = I[:4099], J[:4099], V[:4099]
        want = R.scatter_add(M.nzval.copy(), pat, I, J, V)
        hv, dV = on_device(V)
        for t, glob in ((np.int64, True), (np.int32, False), (np.int64, False)):
            A = pamd.PSparseMatrix.from_csc(pdata(parts, [M]), rows, rows)
            dm = A.values.parts[0]
            idx = (pamd.device.device_index_gids if glob else pamd.device.device_index)(ctx, s)
            ids = (s.lid_to_gid[I - 1], s.lid_to_gid[J - 1]) if glob else (I.astype(t), J.astype(t))
            (hi, dI), (hj, dJ) = on_device(ids[0]), on_device(ids[1])
            dm.scatter(idx, idx, dI, dJ, dV, ids_global=glob)
            assert same_bits(dm.get_values(), want)
            assert np.array_equal(hi.download().view(t), ids[0]) and np.array_equal(hj.download().view(t), ids[1])
            out = DV(ctx, dtype, 4099)
            dm.gather(idx, idx, dI, dJ, ids_global=glob, out=out.as_array())
            assert same_bits(out.download(), R.gather(want, pat, I, J))


# ---------------------------------------------------------------------------
# 4. errors leave A unchanged

def test_errors_leave_the_matrix_unchanged(be, pamd):
    rng = np.random.default_rng(47)
    for dtype in (np.float32, np.complex128):
        parts, rows, csc = small_case(pamd, be, dtype, rng)
        A = pamd.PSparseMatrix.from_csc(pdata(parts, csc), rows, rows)
        lv, gv = pamd.local_view(A, rows, rows).parts, pamd.global_view(A, rows, rows).parts
        for p, (s, M) in enumerate(zip(rows.partition.parts, csc)):
            pat = pattern_of(M)
            ri, ci = pat.rows_cols()
            dm = A.values.parts[p]
            start = dm.get_values()
            assert same_bits(start, M.nzval)
            k = rng.integers(0, pat.nnz, size=300)
            good_i, good_j, V = ri[k] + 1, ci[k] + 1, entries(dtype, 300, rng)
            for bad_lid in (0, s.num_lids + 1):
                for which in (0, 1):
                    ids = [good_i.copy(), good_j.copy()]
                    ids[which][250] = bad_lid
                    for t in (np.int32, np.int64):
                        i, j = ids[0].astype(t), ids[1].astype(t)
                        with pytest.raises(pamd.PAError, match="BoundsError"):
                            lv[p].add_(i, j, V)
                        with pytest.raises(pamd.PAError, match="BoundsError"):
                            lv[p].set_(i, j, V)
                        with pytest.raises(pamd.PAError, match="BoundsError"):
                            lv[p].get(i, j)
                        assert same_bits(dm.get_values(), start)
            # a gid outside the part
            G, H = s.lid_to_gid[good_i - 1].copy(), s.lid_to_gid[good_j - 1].copy()
            G[7] = 1000
            G0 = G.copy()
            with pytest.raises(pamd.PAError, match="KeyError"):
                gv[p].add_(G, H, V)
            with pytest.raises(pamd.PAError, match="KeyError"):
                gv[p].set_(H, G, V)
            with pytest.raises(pamd.PAError, match="KeyError"):
                gv[p].get(G, H)
            assert np.array_equal(G, G0) and same_bits(dm.get_values(), start)
            # a write to an entry the pattern does not store, in the middle of a valid batch
            ai, aj = absent(pat, rng, 1)
            i, j = good_i.copy(), good_j.copy()
            i[150], j[150] = ai[0], aj[0]
            with pytest.raises(pamd.PAError, match="not stored"):
                lv[p].add_(i, j, V)
            with pytest.raises(pamd.PAError, match="not stored"):
                gv[p].set_(s.lid_to_gid[i - 1], s.lid_to_gid[j - 1], V)
            assert same_bits(dm.get_values(), start)
            assert same_bits(lv[p].get(i, j), R.gather(start, pat, i, j))  # the read is fine
        a = [absent(pattern_of(M), rng, 1) for M in csc]
        with pytest.raises(pamd.PAError, match="not stored"):  # add_coo_ over all parts
            pamd.add_coo_(A, pdata(parts, [x[0] for x in a]), pdata(parts, [x[1] for x in a]),
                          pdata(parts, [np.ones(1, dtype) for _ in a]), ids="local")
        other = pamd.prange_cartesian(parts, (9, 7))
        with pytest.raises(NotImplementedError):
            pamd.global_view(A, other, A.cols)
    # a matrix without a nonzero map has no entry views
    S = pamd.drivers.stencil_operator(be.get_part_ids((1, 1, 1)), (6, 5, 4), 7)
    with pytest.raises(pamd.PAError, match="CSC pattern"):
        pamd.local_view(S, S.rows, S.cols).parts[0].get([1], [1])


# ---------------------------------------------------------------------------
# 5. laziness

def test_the_entry_table_is_built_by_the_first_view_call(be, pamd):
    c = Case2(pamd, be, np.float64, seed=53)
    for M in c.A.values.parts:
        assert M.entry_table() == (0, 0)
    x = pamd.PVector.full(1.0, c.cols)
    y = pamd.PVector.undef(c.rows)
    pamd.mul_(y, c.A, x)
    pamd.fillstored_(c.A, 0)
    e = np.zeros(0, np.int64)
    views = pamd.local_view(c.A, c.rows, c.cols).parts  # opening a view builds nothing yet
    views[0].add_(e, e, np.zeros(0))                    # ... nor does an empty call
    for M in c.A.values.parts:
        assert M.entry_table() == (0, 0)
    assert not R.bits(views[0].get([1], [1])).any()
    M0, M1 = c.A.values.parts
    info = M0.info()
    ghost_nnz = M0.csc_nnz - info["nnz"]
    assert ghost_nnz > 0 and info["long_rows"] > 0
    assert M0.entry_table() == (info["nnz"] + ghost_nnz, 16 * (info["nnz"] + ghost_nnz))
    assert M1.entry_table() == (0, 0)  # a table per matrix part


# ---------------------------------------------------------------------------
# 6. the entry table and findnz: one pair-building routine, no shared state

def _findnz(pamd, c, p, all_rows, ids_global):
    """findnz of part p of the case's matrix: (I, J, V) on the host"""
    ctx = pamd.device.contexts(c.rows.partition)[p]
    index = pamd.device.device_index_gids if ids_global else pamd.device.device_index
    r, cl = index(ctx, c.rows.partition.parts[p]), index(ctx, c.cols.partition.parts[p])
    return c.A.values.parts[p].findnz(r, cl, all_rows=all_rows, ids_global=ids_global).download()


def _same_coo(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2])


@pytest.mark.parametrize("parent", ["csc", 1], ids=["csc", "csr"])
@pytest.mark.parametrize("dtype,f32_rows", [(np.float32, 4), (np.float64, 0)], ids=["float32", "float64"])
def test_entry_table_and_findnz_share_no_state(be, pamd, dtype, f32_rows, parent):
    """findnz before, between and after the view calls that build the entry
    table: neither changes what the other gives, in either order."""
    c = Case2(pamd, be, dtype, f32_rows, seed=61, parent=parent, shuffle_row_lids=True)
    F = []
    for p, (M, s) in enumerate(zip(c.A.values.parts, c.rows.partition.parts)):
        info = M.info()
        print(p, {k: info[k] for k in ("nrows", "nnz", "nslices", "long_rows", "delta16_slices")}, M.csc_nnz)
        # what the matrix must hold for the passes to meet every kind of value index
        assert np.any(np.diff(s.oid_to_lid) != 1) and s.num_hids > 0  # owned lids not contiguous
        assert M.csc_nnz - info["nnz"] > 0                            # stored ghost rows
        assert info["long_rows"] > 0
        assert dtype != np.float32 or info["delta16_slices"] > 0
        # 1. findnz builds no table
        F0 = _findnz(pamd, c, p, True, False)
        assert len(F0[0]) == M.csc_nnz and M.entry_table() == (0, 0)
        # 2. the first view call does, and reads the same values
        view = pamd.local_view(c.A, c.rows, c.cols).parts[p]
        assert same_bits(view.get(F0[0], F0[1]), F0[2])
        table = M.entry_table()
        assert table == (len(F0[0]), 16 * len(F0[0]))
        # 3. findnz again: the same, and the table as it was
        assert _same_coo(_findnz(pamd, c, p, True, False), F0) and M.entry_table() == table
        # 4. a write through the table, read back by findnz over the owned rows
        view.add_(F0[0], F0[1], np.ones(len(F0[0]), dtype))
        own = s.lid_to_part[F0[0] - 1] == s.part
        assert 0 < own.sum() < len(own)
        F4 = _findnz(pamd, c, p, False, False)
        assert _same_coo(F4, (F0[0][own], F0[1][own], F0[2][own] + dtype(1)))
        # 5. and with global ids
        gids = (s.lid_to_gid[F4[0] - 1], c.cols.partition.parts[p].lid_to_gid[F4[1] - 1], F4[2])
        assert _same_coo(_findnz(pamd, c, p, False, True), gids) and M.entry_table() == table
        F.append(F0)
    # a fresh matrix, the table first: findnz gives the same
    c = Case2(pamd, be, dtype, f32_rows, seed=61, parent=parent, shuffle_row_lids=True)
    for p, (M, F0) in enumerate(zip(c.A.values.parts, F)):
        assert M.entry_table() == (0, 0)
        assert same_bits(pamd.local_view(c.A, c.rows, c.cols).parts[p].get(F0[0], F0[1]), F0[2])
        assert M.entry_table() == (len(F0[0]), 16 * len(F0[0]))
        assert _same_coo(_findnz(pamd, c, p, True, False), F0)
