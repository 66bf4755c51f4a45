"""Band matrices without identity rows against the oracle: pattern rows whose
first column is x[0] or whose last column is x[nx-1], rows that share a lane
with a side row or with a row past nrows, and CSR parents whose rows are not
stored in ascending column order.

A band matrix of order n with offset set D stores (i, i+d) for every d in D
with 1 <= i+d <= n (1-based gids): no identity rows, no wrap-around, every
stored value distinct (seeded uniform(-1, 1)).  The Dirichlet stencils of the
other parity tests keep diagonal-only rows next to the ends of x, so there
the 16 B x runs of the pattern kernels never start before x[0] or end after
x[nx-1] on behalf of a valid row.

The offset sets are chosen by the kernel they reach (Float64, 128-row slices):
D3, D5, D5w, D7 the short-row kernels and the uniform layout (spmv_wave_u),
D8 the short-row batch of 8, D9, D9w, D12 rows_pattern_tri, D11 rows_pattern.
The sizes are the smallest that keep the first and the last slice pattern
slices for Float64 (at least 70 % of the slice's valid rows regular), in both
parities of n: with reach b the low end has a lane whose first row is a side
row when b is odd, the high end when n-1-b is even.

Every test but the last needs the GPU and carries the gpu mark itself (the
module has no pytestmark: the long-double reference is checked against the
oracle on the CPU)."""
import numpy as np
import pytest

from matrix_cases import (SEED, _as_array, _eq, _knobs, _nan, _real, _sel, _to_oracle, check_bound, rand as _rand,
                          unsorted_csr as _unsorted_csr)

gpu = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128, np.complex64]
AB = [(1.0, 0.0), (-1.3, 0.5)]

_D9W = (-20, -19, -18, -1, 0, 1, 18, 19, 20)
BANDS = {
    "D3": (-1, 0, 1),
    "D5": (-2, -1, 0, 1, 2),
    "D5w": (-19, -1, 0, 1, 19),
    "D7": (-37, -19, -1, 0, 1, 19, 37),
    "D8": tuple(range(-3, 5)),
    "D9": tuple(range(-4, 5)),
    "D9w": _D9W,
    "D11": tuple(range(-5, 6)),
    "D12": _D9W + (37, 38, 39),
}
SIZES = {"D3": (389, 390), "D5": (389, 390), "D8": (389, 390), "D9": (389, 390), "D11": (389, 390),
         "D5w": (484, 485), "D7": (511, 512), "D9w": (511, 512), "D12": (511, 512)}
UNIFORM = ("D3", "D5w", "D7")  # at most 7 offsets: Float64 gets the uniform layout


def _ids(names):
    return [(k, n) for k in names for n in SIZES[k]]


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


def band_coo(n, D, dtype, seed, spd=False):
    """The band matrix's global COO in row order (1-based gids) and a global
    x.  spd: diagonal 4 + 0.01*i, off-diagonals -1 (D3 only)."""
    D = np.asarray(D, np.int64)
    g = np.arange(1, n + 1, dtype=np.int64)
    J = g[:, None] + D[None, :]
    keep = (J >= 1) & (J <= n)
    I = np.broadcast_to(g[:, None], J.shape)[keep]
    J = J[keep]
    rng = np.random.default_rng([SEED, seed, n, len(D)])
    V = _rand(rng, len(I), dtype)
    if spd:
        V = np.where(I == J, 4.0 + 0.01 * I, -1.0).astype(dtype)
    x = _rand(rng, n, dtype)
    return I, J, V, x


def oracle_band(O, nparts, n, I, J, V):
    oparts = O.get_part_ids(nparts)
    orows = O.prange_linear(oparts, n)
    sel = [np.isin(I, np.asarray(s.lid_to_gid)[np.asarray(s.oid_to_lid) - 1]) for s in orows.partition.parts]
    oI = O.PData([list(I[k]) for k in sel])
    oJ = O.PData([list(J[k]) for k in sel])
    oV = O.PData([_to_oracle(O, V[k]) for k in sel])
    ocols = O.add_gids(orows, oJ)
    return O.psparse_from_coo(oI, oJ, oV, orows, ocols, ids="global")


def oracle_x(O, OA, x):
    """the oracle's x: owned values from the global x, ghosts 0."""
    def f(s):
        own = np.asarray(s.lid_to_part) == s.part
        v = np.where(own, x[np.asarray(s.lid_to_gid) - 1], 0).astype(x.dtype)
        return _to_oracle(O, v)
    return O.PVector(O.map_parts(f, OA.cols.partition), OA.cols)


class Case:
    """One band matrix on the device and in the oracle."""

    def __init__(self, pamd, O, be, name, n, dtype, nparts, spd=False):
        self.name, self.n, self.dtype, self.nparts, self.D = name, n, np.dtype(dtype), nparts, BANDS[name]
        self.I, self.J, self.V, self.x = band_coo(n, self.D, dtype, 1, spd)
        self.parts = parts = be.get_part_ids(nparts)
        rows = pamd.prange_linear(parts, n)
        sel = {p: np.isin(self.I, s.lid_to_gid[s.oid_to_lid - 1]) for p, s in zip(parts.part_ids, rows.partition.parts)}
        mk = lambda a: pamd.PData(parts.backend, parts.part_ids, [a[sel[p]].copy() for p in parts.part_ids],
                                  parts.shape)
        cols = pamd.add_gids(rows, mk(self.J))
        self.A = pamd.PSparseMatrix.from_coo(mk(self.I), mk(self.J), mk(self.V), rows, cols, ids="global")
        self.OA = oracle_band(O, nparts, n, self.I, self.J, self.V)
        self.info = {p: self.A.values.local(p).info() for p in parts.part_ids}

    def device_x(self, pamd, nan_ghosts=True):
        """x on the device: owned values from the global x, the ghosts NaN
        (the halo has to fill them)."""
        def f(s):
            v = _nan(s.num_lids, self.dtype) if nan_ghosts else np.zeros(s.num_lids, self.dtype)
            own = s.oid_to_lid - 1
            v[own] = self.x[s.lid_to_gid[own] - 1]
            return v
        return pamd.PVector.from_host(pamd.map_parts(f, self.A.cols.partition), self.A.cols)

    def regular_rows(self, p):
        """rows of part p with every offset in range whose columns' lids are
        row + offset (a ghost column counts only at that lid)."""
        s, c = self.A.rows.partition.local(p), self.A.cols.partition.local(p)
        D = np.asarray(self.D, np.int64)
        g = s.lid_to_gid[s.oid_to_lid - 1]
        G = g[:, None] + D[None, :]
        full = np.flatnonzero(((G >= 1) & (G <= self.n)).all(axis=1))
        lids = c.to_lids(G[full].ravel()).reshape(len(full), len(D)) - 1
        return int(np.count_nonzero((lids == full[:, None] + D[None, :]).all(axis=1)))


_cache = {}


def get_case(pamd, O, be, name, n, dtype, nparts, **knobs):
    """The case built under the knobs now set (passed again as the key): the
    (α, β) cases of one matrix share it."""
    key = (name, n, np.dtype(dtype).str, nparts, tuple(sorted(knobs.items())))
    if key not in _cache:
        _cache.clear()
        _cache[key] = Case(pamd, O, be, name, n, dtype, nparts)
    return _cache[key]


def check_paths(c, fmt=1):
    """the pattern path was really taken (item 1 of the issue)."""
    # ComplexF64 slices hold 64 rows: with a reach of 20 or more fewer than
    # 70 % of the rows of the first and of the last slice have every offset in
    # range at any n, so those two are int32 / delta16 slices, which hold the
    # boundary rows, and the pattern slices between them have no side row
    ends_irregular = c.dtype == np.dtype(np.complex128) and max(np.abs(c.D)) >= 20 and c.nparts == 1
    for p, i in c.info.items():
        assert i["pattern_slices"] >= 1, (p, i)
        if ends_irregular:
            assert i["side_rows"] == 0 and i["pattern_slices"] == i["nslices"] - 2, (p, i)
        else:
            assert i["side_rows"] >= 1, (p, i)
        if fmt == 0:  # int32 column ids for every stored entry
            assert c.A.values.local(p).traffic()["index_bytes"] >= 4 * i["nnz"], (p, i)
    if c.dtype == np.dtype(np.float64) and c.name in UNIFORM:
        for p, i in c.info.items():
            assert i["pattern_slices"] == i["nslices"], (p, i)
            assert i["regular_rows"] == c.regular_rows(p), (p, i["regular_rows"], c.regular_rows(p))


def check_mul(pamd, O, c, alpha, beta, what=""):
    """mul!(y, A, x, α, β): owned rows of y and every lid of x bit-equal to
    the oracle's; for (1, 0) also the long-double bound."""
    A, OA = c.A, c.OA
    rng = np.random.default_rng([SEED, 7, c.n])
    y0 = _rand(rng, c.n, c.dtype)
    x = c.device_x(pamd)
    ox = oracle_x(O, OA, c.x)
    if beta == 0:  # a row never written stays NaN
        y = pamd.PVector.from_host(pamd.map_parts(lambda s: _nan(s.num_lids, c.dtype), A.rows.partition), A.rows)
    else:
        y = pamd.PVector.from_host(pamd.map_parts(lambda s: y0[s.lid_to_gid - 1], A.rows.partition), A.rows)
    oy = O.PVector(O.map_parts(lambda s: _to_oracle(O, y0[np.asarray(s.lid_to_gid) - 1]), OA.rows.partition), OA.rows)
    sc = _real(c.dtype)
    pamd.mul_(y, A, x, alpha, beta)
    O.mul_(oy, OA, ox, sc(alpha), sc(beta))
    got, gx = y.to_host(), x.to_host()
    yg = np.empty(c.n, c.dtype)
    for p in c.parts.part_ids:
        s = A.rows.partition.local(p)
        own = s.oid_to_lid - 1
        yg[s.lid_to_gid[own] - 1] = got.local(p)[own]
    bound_failure = None
    if (alpha, beta) == (1.0, 0.0):  # its figure is printed before anything is asserted
        try:
            check_bound(yg, c.n, c.I, c.J, c.V, c.x, f"{c.name} n={c.n} {c.dtype} {what}")
        except AssertionError as e:
            bound_failure = e
    for p in c.parts.part_ids:
        own = A.rows.partition.local(p).oid_to_lid - 1
        ref = _as_array(O, _sel(O, oy.values[p], own))
        bad = np.flatnonzero(~((got.local(p)[own] == ref) | (np.isnan(ref) & np.isnan(got.local(p)[own]))))
        assert _eq(O, got.local(p)[own], _sel(O, oy.values[p], own)), \
            f"{what} part {p} (α, β) = {(alpha, beta)}: {bad.size} owned rows differ from the oracle, oids {bad[:8]}"
        assert _eq(O, gx.local(p), ox.values[p]), f"{what} part {p}: x after the halo differs from the oracle's"
    if bound_failure is not None:
        raise bound_failure
    return yg


# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,n", _ids(BANDS))
def test_band_one_part_default_knobs(be, pamd, O, name, n, dtype, alpha, beta):
    c = get_case(pamd, O, be, name, n, dtype, 1)
    check_paths(c)
    check_mul(pamd, O, c, alpha, beta)


@gpu
@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("fmt", [1, 0], ids=["pattern", "int32"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,n", _ids(("D3", "D9", "D11")))
def test_band_one_part_both_column_encodings(be, pamd, O, name, n, dtype, fmt, alpha, beta):
    """spmv_format 0: the int32 / delta16 kernels see the same rows."""
    with _knobs(pamd, spmv_format=fmt):
        c = get_case(pamd, O, be, name, n, dtype, 1, spmv_format=fmt)
        check_paths(c, fmt)
        check_mul(pamd, O, c, alpha, beta, f"spmv_format {fmt}")


def _sizes3(name):
    return {"D3": (3 * 389, 3 * 390), "D5w": (3 * 484, 3 * 485)}[name]


@gpu
@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,n", [(k, n) for k in ("D3", "D5w") for n in _sizes3(k)])
def test_band_three_parts_default_knobs(be, pamd, O, name, n, dtype, alpha, beta):
    """Three parts: the last owned row of part 1 is a regular row whose +1
    column is the first ghost lid (== nx-1 for D3) and whose lane partner
    lies past nrows."""
    c = get_case(pamd, O, be, name, n, dtype, 3)
    check_paths(c)
    check_mul(pamd, O, c, alpha, beta)


@gpu
@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("uniform", [1, 0], ids=["uniform", "no_uniform"])
@pytest.mark.parametrize("merge", [1, 0], ids=["merged", "per_kind"])
@pytest.mark.parametrize("nparts", [1, 3], ids=["1part", "3parts"])
@pytest.mark.parametrize("name,n1", _ids(UNIFORM))
def test_band_float64_uniform_layout_and_launch_modes(be, pamd, O, name, n1, nparts, merge, uniform, alpha, beta):
    """Float64 with the uniform layout on and off, the merged launch and the
    per-kind launches (one part: the short-row tail launch over the uniform
    layout, spmv_wave_u; three parts reach it with spmv_merge 0: direct pull,
    per-kind launches, the side rows as the tail)."""
    n = nparts * n1  # n1 rows per part
    with _knobs(pamd, spmv_uniform=uniform, spmv_merge=merge):
        c = get_case(pamd, O, be, name, n, np.float64, nparts, spmv_uniform=uniform, spmv_merge=merge)
        check_paths(c)
        check_mul(pamd, O, c, alpha, beta, f"spmv_uniform {uniform} spmv_merge {merge}")


@gpu
@pytest.mark.parametrize("name,n", _ids(("D3", "D7")))
def test_band_fused_dot(be, pamd, O, name, n):
    """mul_dot_ (spmv_wave_u has its own copy of the fused-dot code): y is
    bit-equal to mul_'s and the dot is within 1e-12 relative (the project's
    tolerance for dots) of dot(x, y) in long double from the device's own y."""
    c = get_case(pamd, O, be, name, n, np.float64, 1)
    check_paths(c)
    yref = check_mul(pamd, O, c, 1.0, 0.0)
    x = c.device_x(pamd)
    y = pamd.PVector.from_host(pamd.map_parts(lambda s: _nan(s.num_lids, c.dtype), c.A.cols.partition), c.A.cols)
    d = pamd.mul_dot_(y, c.A, x)
    got = y.to_host().local(1)
    assert np.array_equal(got, yref)
    ref = np.sum(c.x.astype(np.longdouble) * got.astype(np.longdouble))
    print(f"{name} n={n}: fused dot {d!r}, long double {float(ref)!r}")
    assert abs(np.longdouble(d) - ref) <= 1e-12 * abs(ref), (d, float(ref))


@gpu
@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("n", SIZES["D5w"])
def test_band_set_values_refreshes_uniform_copy(be, pamd, O, n, alpha, beta):
    """set_values with fresh random values, then mul! again: the uniform
    layout's copy of the values follows."""
    c = Case(pamd, O, be, "D5w", n, np.float64, 1)
    check_paths(c)
    check_mul(pamd, O, c, alpha, beta, "before set_values")
    M = c.OA.values.parts[0]
    v2 = np.random.default_rng([SEED, 11, n]).uniform(-1, 1, len(M.nzval))
    c.A.values.local(1).set_values(v2)  # nonzeros(A) in CSC order, as the oracle's
    # the triplets again for the long-double reference: CSC order is (column, row)
    order = np.lexsort((c.I, c.J))
    c.V = np.empty_like(c.V)
    c.V[order] = v2
    c.OA = O.PSparseMatrix(O.map_parts(lambda M: O.CSC(M.m, M.n, M.colptr, M.rowval, v2.copy()), c.OA.values),
                           c.OA.rows, c.OA.cols)
    check_mul(pamd, O, c, alpha, beta, "after set_values")


@gpu
@pytest.mark.parametrize("n,nparts,dtype,fuse", [
    (389, 1, np.float64, 0), (389, 1, np.float64, 1), (390, 1, np.float64, 0), (390, 1, np.float64, 1),
    (3 * 389, 3, np.float64, 0), (3 * 389, 3, np.float64, 1), (390, 1, np.float32, 1)])
def test_band_device_cg(be, pamd, O, n, nparts, dtype, fuse):
    """Device CG on the symmetric positive definite D3 (diagonal 4 + 0.01*i,
    off-diagonals -1), 25 iterations in batches of 4: x and the residual
    history are bit-identical between the host-driven and the device
    recurrence (cg_fuse 0: u .= r .+ β.*u as a sweep; 1: the XV kernels, whose runs read r[-1] and u[-1]),
    and the history follows the oracle's cg! (rtol 1e-8, atol 1e-14, as
    test_empty_parts_cg).  Float32 (cg_fuse 1 only): the oracle comparison
    covers the residuals above sqrt(eps(Float32))*norm(b), cg!'s own default
    tolerance, at the 5e-6 of test_fdm_cg_float32_julia_scalars (the local
    dot / norm order is not pinned); below it a Float32 recurrence is
    rounding noise."""
    with _knobs(pamd, cg_fuse=fuse):
        c = Case(pamd, O, be, "D3", n, dtype, nparts, spd=True)
        check_paths(c)
        b = c.device_x(pamd, nan_ghosts=False)
        xs, hs = [], []
        for device in (False, True):
            x = pamd.PVector.undef(c.A.cols, dtype).fill_(0)
            h = []
            pamd.cg_(x, c.A, b, reltol=0.0, maxiter=25, history=h, fused=True, device=device, batch=4)
            xs.append(x.to_host())
            hs.append(h)
        ob = oracle_x(O, c.OA, c.x)
        ox = O.pvector_undef(c.OA.cols, dtype)
        oh = []
        O.cg_(ox, c.OA, ob, reltol=0.0, maxiter=25, log=oh)
        print("device", hs[1], "\noracle", oh)
        assert len(hs[0]) == len(hs[1]) == len(oh) == 25
        assert hs[0] == hs[1]
        for p in c.parts.part_ids:
            assert np.array_equal(xs[0].local(p), xs[1].local(p))
        if np.dtype(dtype) == np.float32:
            nb = float(np.sqrt(np.sum(c.x.astype(np.float64) ** 2)))
            k = int(np.argmax(np.asarray(oh) <= np.sqrt(np.finfo(np.float32).eps) * nb))
            assert k >= 3
            np.testing.assert_allclose(hs[1][:k], oh[:k], rtol=5e-6)
        else:
            np.testing.assert_allclose(hs[1], oh, rtol=1e-8, atol=1e-14)


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
@pytest.mark.parametrize("Bi", [0, 1])
@pytest.mark.parametrize("order", ["diag_first", "descending"])
@pytest.mark.parametrize("name", ["D3", "D5w"])
def test_band_csr_parent_with_unsorted_rows(be, pamd, O, name, order, Bi, dtype):
    """A SparseMatrixCSR{Bi} parent whose rows are not stored in ascending
    column order (pa_mat_from_csr: storage order is the summation order):
    the build succeeds (no uniform layout for such a matrix) and mul! with
    α = 1 and 0.1 is bit-equal to the oracle's literal storage-order loop;
    Float64 also with spmv_uniform 0, bit-equal to the default's."""
    n = 390
    rowptr, colval, V, I, J, xg = _unsorted_csr(n, BANDS[name], Bi, order, dtype)
    parts = be.get_part_ids(1)
    rows = pamd.prange_linear(parts, n)
    orows = O.prange_linear(O.get_part_ids(1), n)
    OA = O.PSparseMatrix(O.PData([O.CSR(Bi, n, n, rowptr, colval, _to_oracle(O, V))]), orows, orows)
    ox = O.PVector(O.PData([_to_oracle(O, xg)]), orows)
    res = {}
    for uniform in ((1, 0) if np.dtype(dtype) == np.float64 else (1,)):
        with _knobs(pamd, spmv_uniform=uniform):
            csr = pamd.PData(parts.backend, parts.part_ids, [pamd.CSR(Bi, n, n, rowptr, colval, V)], parts.shape)
            A = pamd.PSparseMatrix.from_csr(csr, rows, rows)
            info = A.values.local(1).info()
            assert info["pattern_slices"] >= 1 and info["side_rows"] >= 1, info
            x = pamd.PVector.from_host(pamd.map_parts(lambda s: xg, rows.partition), rows)
            for alpha in (1.0, 0.1):
                y = pamd.PVector.from_host(pamd.map_parts(lambda s: _nan(n, dtype), rows.partition), rows)
                pamd.mul_(y, A, x, alpha, 0.0)
                got = res[uniform, alpha] = y.to_host().local(1)
                oy = O.pvector_undef(orows, dtype)
                O.mul_(oy, OA, ox, alpha, 0.0, literal=True)
                if alpha == 1.0:
                    try:
                        check_bound(got, n, I, J, V, xg, f"CSR {name} {order} Bi={Bi} {np.dtype(dtype)}")
                    except AssertionError as e:
                        print(e)
                assert _eq(O, got, oy.values[1]), (uniform, alpha)
    for (uniform, alpha), got in res.items():
        assert np.array_equal(got, res[1, alpha]), (uniform, alpha)


# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,n", _ids(("D3", "D9", "D5w")))
def test_longdouble_reference_against_oracle(O, name, n, dtype):
    """The long-double reference and its bound, checked where there is no
    GPU: the oracle's mul! (the reference's summation order in the element
    type) stays inside the bound on one part."""
    I, J, V, x = band_coo(n, BANDS[name], dtype, 1)
    OA = oracle_band(O, 1, n, I, J, V)
    ox = oracle_x(O, OA, x)
    oy = O.pvector_undef(OA.rows, dtype)
    O.mul_(oy, OA, ox)
    y = np.asarray(_as_array(O, oy.values[1])).astype(dtype)
    check_bound(y, n, I, J, V, x, f"oracle {name} n={n} {np.dtype(dtype)}")
    # the bound is not vacuous: x[1] in place of x[0] in row 2's first term misses it
    y2 = y.copy()
    k = np.flatnonzero((I == 2) & (J == 1))[0]
    y2[1] = y2[1] - V[k] * x[0] + V[k] * x[1]
    with pytest.raises(AssertionError, match="miss the long-double bound"):
        check_bound(y2, n, I, J, V, x, "perturbed")
