"""Run matrices against the oracle: the column encodings that are not
pattern slices (delta16 slices, the triple SELL with its tri and pair slices,
Float32 interleaved rows) on rows the stencil drivers never produce.

matrix_cases.run_coo: rows of 1 to 19 consecutive-column triples in groups
of shifted copies (pairs), every remainder of the batches of 4 and of 9
triples, rows of runs of 1, 2, 4, 5 columns and of broken triples, triples
at lid 0, at lid nx-1 and across the owned/ghost boundary, a distinct value
per entry.  matrix_cases.reach_coo: columns exactly at the limits of the
16-bit codes (owned deltas +16383, +16384, -16384, -16385; a slice's ghost
span 32766, 32767), in a part with more than 32767 ghosts.

The sizes: 1300 rows per part gave no tri slice of exactly 4 triples at 128
rows per slice, so the run matrices have 1801, 1802 and 3 x 1400 rows, the
smallest scanned (steps of 50 and 100) whose predicted layouts hold every
slice shape test_run_coverage asks for.

The CPU tests (no gpu mark) check from the oracle's matrices that the rows,
slices and limits above are really there, and that the oracle's mul! stays
inside the long-double bound.  The GPU tests carry the gpu mark themselves."""
import numpy as np
import pytest

from matrix_cases import (OTHER_RUNS, SEED, TRI_LENS, _as_array, _knobs, _nan, _to_oracle, check_bound,
                          classify_rows, predict_triple_sell, rand as _rand, reach_coo, reach_rows, rows_of_csc,
                          run_coo, slice_fit, triple_counters)
from test_gpu_band import check_mul, oracle_band, oracle_x

gpu = pytest.mark.gpu

DTYPES = [np.float64, np.float32, np.complex128, np.complex64]
AB = [(1.0, 0.0), (-1.3, 0.5)]
RUNS = [(1801, 1), (1802, 1), (3 * 1400, 3)]
RUNS3 = RUNS[2]
PER = 52000  # rows per part of the reach matrix
FLAGS = (1 | 4 | 16 | 64, 1 | 4 | 16 | 64 | 8)  # without / with the masked tail batch
LIMITS = ("dmax 16383", "dmax 16384", "dmin -16384", "dmin -16385", "span 32766", "span 32767")


def slice_rows(dtype, f32_rows=2):
    """rows per slice and per lane of the element type's SELL (Float32: 2
    rows per lane by the auto rule of a matrix without pattern slices)"""
    dtype = np.dtype(dtype)
    R = 1 if dtype == np.complex128 else f32_rows if dtype == np.float32 else 2
    return 64 * R, R


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


class Host:
    """The triplets, x and the oracle's matrix of one generated case (never
    modified), and per part the rows' column lids from the oracle's CSC."""

    def __init__(self, O, gen, n, nparts, dtype, probes=None):
        self.name, self.n, self.nparts, self.dtype = f"{gen} {probes or ''}".strip(), n, nparts, np.dtype(dtype)
        self.I, self.J, self.V, self.x = run_coo(n, nparts, dtype, 1) if gen == "run" else \
            reach_coo(n // 2, dtype, probes)
        self.OA = oracle_band(O, nparts, n, self.I, self.J, self.V)
        self.noids = [len(s.oid_to_lid) for s in self.OA.cols.partition.parts]
        self.nx = [M.n for M in self.OA.values.parts]
        self._rows = {}

    def rows(self, k):
        if k not in self._rows:
            self._rows[k] = rows_of_csc(self.OA.values.parts[k], self.noids[k])
        return self._rows[k]

    def classes(self, k):
        return classify_rows(self.rows(k), self.noids[k])

    def oracle_y(self, O):
        """the oracle's mul! as one global vector"""
        oy = O.pvector_undef(self.OA.rows, self.dtype)
        O.mul_(oy, self.OA, oracle_x(O, self.OA, self.x))
        y = np.empty(self.n, self.dtype)
        for s, v in zip(self.OA.rows.partition.parts, oy.values.parts):
            own = np.asarray(s.oid_to_lid) - 1
            y[np.asarray(s.lid_to_gid)[own] - 1] = np.asarray(_as_array(O, v))[own]
        return y


_host = {}


def host(O, gen, n, nparts, dtype, probes=None):
    key = (gen, n, nparts, np.dtype(dtype).str, probes)
    if key not in _host:
        if gen == "reach":  # (large: one at a time)
            for k in [k for k in _host if k[0] == "reach"]:
                del _host[k]
        _host[key] = Host(O, gen, n, nparts, dtype, probes)
    return _host[key]


class Case:
    """One host case on the device, built under the knobs now set (the
    attributes check_mul reads)."""

    def __init__(self, pamd, be, h):
        self.h, self.name, self.n, self.dtype, self.nparts = h, h.name, h.n, h.dtype, h.nparts
        self.I, self.J, self.V, self.x, self.OA = h.I, h.J, h.V, h.x, h.OA
        self.parts = parts = be.get_part_ids(h.nparts)
        rows = pamd.prange_linear(parts, h.n)
        sel = {p: np.isin(self.I, s.lid_to_gid[s.oid_to_lid - 1]) for p, s in zip(parts.part_ids, rows.partition.parts)}
        mk = lambda a: pamd.PData(parts.backend, parts.part_ids, [a[sel[p]].copy() for p in parts.part_ids],
                                  parts.shape)
        cols = pamd.add_gids(rows, mk(self.J))
        self.A = pamd.PSparseMatrix.from_coo(mk(self.I), mk(self.J), mk(self.V), rows, cols, ids="global")
        self.info = [self.A.values.local(p).info() for p in parts.part_ids]
        # the CPU audit of the oracle's matrix applies to this one
        for p, s in zip(parts.part_ids, h.OA.cols.partition.parts):
            assert np.array_equal(self.A.cols.partition.local(p).lid_to_gid, np.asarray(s.lid_to_gid)), p

    def device_x(self, pamd):
        """x on the device: owned values from the global x, the ghosts NaN
        (the halo has to fill them)."""
        def f(s):
            v = _nan(s.num_lids, self.dtype)
            own = s.oid_to_lid - 1
            v[own] = self.x[s.lid_to_gid[own] - 1]
            return v
        return pamd.PVector.from_host(pamd.map_parts(f, self.A.cols.partition), self.A.cols)


_cache = {}


def get_case(pamd, be, h, **knobs):
    """The case built under the knobs now set (passed again as the key): the
    (α, β) cases of one matrix share it."""
    key = (h.name, h.n, h.dtype.str, h.nparts, tuple(sorted(knobs.items())))
    if key not in _cache:
        _cache.clear()
        _cache[key] = Case(pamd, be, h)
    return _cache[key]


def check_triple_counters(c, H, R, tri_order=1, pairs_on=True, rows_of=None):
    """info()'s triple-SELL counters per part against predict_triple_sell."""
    out = []
    for k, i in enumerate(c.info):
        cl = c.h.classes(k)
        if rows_of is not None:
            cl = [cl[r] for r in rows_of[k]]
        want = triple_counters(predict_triple_sell(cl, H, R, tri_order, pairs_on))
        got = {key: i[key] for key in want}
        out.append((want, got))
        assert got == want, (k + 1, got, want)
    return out


# ---------------------------------------------------------------------------
# CPU: what the generated matrices contain

@pytest.mark.parametrize("n,nparts", RUNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_run_matrix_oracle_inside_bound(O, dtype, n, nparts):
    """The oracle's mul! of the run matrix stays inside the long-double
    bound, and the bound is not vacuous."""
    h = host(O, "run", n, nparts, dtype)
    # a distinct value per entry of a row (Float32 values repeat somewhere among 10^4 draws)
    assert len(np.unique(np.column_stack((h.I, h.V.real, h.V.imag)), axis=0)) == len(h.V)
    y = h.oracle_y(O)
    check_bound(y, n, h.I, h.J, h.V, h.x, f"oracle run n={n} {nparts} parts {h.dtype}")
    # the next column's x in row 2's first term misses it
    k = np.flatnonzero(h.I == 2)[0]
    y2 = y.copy()
    y2[1] = y2[1] - h.V[k] * h.x[h.J[k] - 1] + h.V[k] * h.x[h.J[k]]
    with pytest.raises(AssertionError, match="miss the long-double bound"):
        check_bound(y2, n, h.I, h.J, h.V, h.x, "perturbed")


def _shapes(layout, kind, B):
    """the batch classes of the slices of one kind: their triples per row
    below / equal to / above one batch of B with a remainder"""
    out = set()
    for k, L, _, _ in layout:
        if k == kind:
            t = L // 3
            out.add("below" if t < B else "equal" if t == B else "remainder" if t % B else "multiple")
    return out


@pytest.mark.parametrize("H,R,pairs_on", [(128, 2, True), (64, 1, False)], ids=["H128_pairs", "H64_no_pairs"])
@pytest.mark.parametrize("n,nparts", RUNS)
def test_run_coverage(O, n, nparts, H, R, pairs_on):
    """The run matrix holds the rows and, in the layout predicted for the
    default knobs, the slices that the GPU tests are meant to run (the
    structure does not depend on the element type)."""
    h = host(O, "run", n, nparts, np.float64)
    single_ntri, pair_ntri, other_lens = set(), set(), set()
    shapes_tri, shapes_pair, nother, short = set(), set(), 0, set()
    hand = {"lid 0": set(), "nx-1": set(), "straddle": set()}
    for k in range(nparts):
        cl, noids, nx = h.classes(k), h.noids[k], h.nx[k]
        assert len(cl) == noids
        layout = predict_triple_sell(cl, H, R, 1, pairs_on)
        assert layout, "fewer than a quarter of the rows are regular"
        paired = np.zeros(noids, bool)
        for i in range(noids - 1 if pairs_on else 0):
            a, b = cl[i], cl[i + 1]
            if not paired[i] and a[1] and b[1] and a[0] == b[0] and np.array_equal(a[2] + 1, b[2]):
                paired[i] = paired[i + 1] = True
        for i, (L, reg, c) in enumerate(cl):
            if not reg:
                other_lens.add(L)
                continue
            (pair_ntri if paired[i] else single_ntri).add(L // 3)
            how = "pair" if paired[i] else "single"
            if c[0] == 0:
                hand["lid 0"].add(how)
            if c[-1] == nx - 1:
                hand["nx-1"].add(how)
            if np.any((c[::3] < noids) & (c[::3] + 2 >= noids)):
                hand["straddle"].add(how)
        shapes_tri |= _shapes(layout, "tri", 4)
        shapes_pair |= _shapes(layout, "pair", 9)
        nother += sum(1 for s in layout if s[0] == "other")
        short |= {s[0] for s in layout if s[3] < s[1]}  # slices holding rows shorter than the slice
    print(f"n={n} {nparts} parts H={H}: single ntri {sorted(single_ntri)}, pair ntri {sorted(pair_ntri)}, "
          f"tri slices {sorted(shapes_tri)}, pair slices {sorted(shapes_pair)}, other slices {nother}, hand {hand}")
    assert single_ntri >= set(TRI_LENS)
    assert {sum(r) for r in OTHER_RUNS} <= other_lens
    assert shapes_tri >= {"below", "equal", "remainder"}
    assert nother >= 2 and "tri" in short
    if pairs_on:
        assert pair_ntri >= set(TRI_LENS)
        assert shapes_pair >= {"below", "equal", "remainder"} and "pair" in short
    want = {"pair", "single"} if pairs_on and nparts > 1 else {"single"} if not pairs_on else set()
    assert hand["lid 0"] >= want and hand["lid 0"], hand
    assert hand["nx-1"] >= want and hand["nx-1"], hand
    if nparts > 1:
        assert hand["straddle"] >= want, hand


@pytest.mark.parametrize("probes", ["owned", "ghost"])
def test_reach_limits_present(O, probes):
    """Part 1 of the reach matrix has, for 64, 128 and 256 rows per slice,
    exactly one slice at each limit of the 16-bit codes (those asked for by
    `probes`), the slices past a limit do not fit, part 2 fits entirely, and
    the oracle stays inside the bound."""
    h = host(O, "reach", 2 * PER, 2, np.float64, probes)
    assert h.nx[0] - h.noids[0] > 32767 and h.nx[1] == h.noids[1]
    own, back = reach_rows(PER, probes)
    for H in (64, 128, 256):
        fit, dmin, dmax, span = slice_fit(h.rows(0), H, h.noids[0])
        found = {"dmax 16383": np.flatnonzero(dmax == 16383), "dmax 16384": np.flatnonzero(dmax == 16384),
                 "dmin -16384": np.flatnonzero(dmin == -16384), "dmin -16385": np.flatnonzero(dmin == -16385),
                 "span 32766": np.flatnonzero(span == 32766), "span 32767": np.flatnonzero(span == 32767)}
        print(f"{probes} H={H}: {len(fit)} slices, unfit {np.flatnonzero(~fit)}, {found}")
        for name in LIMITS[:4 if probes == "owned" else 6]:
            assert len(found[name]) == 1, (H, name, found[name])
            assert fit[found[name][0]] == (name in ("dmax 16383", "dmin -16384", "span 32766")), (H, name)
        assert np.count_nonzero(~fit) == (2 if probes == "owned" else 3)
        assert dmax.max() <= 16384 and dmin.min() >= -16385 and span.max() <= 32767
        assert slice_fit(h.rows(1), H, h.noids[1])[0].all()
    # the probe rows' lengths: the ghost probes are the only rows of 5 entries
    lens = np.array([len(r) for r in h.rows(0)])
    assert sorted(np.flatnonzero(lens == 5) + 1) == sorted(back) and lens.max() == (5 if back else 4)
    assert all(lens[i - 1] == 4 for i in own)
    check_bound(h.oracle_y(O), h.n, h.I, h.J, h.V, h.x, f"oracle reach {probes}")


# ---------------------------------------------------------------------------
# GPU

@gpu
@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("n,nparts", RUNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_default_knobs(be, pamd, O, dtype, n, nparts, alpha, beta):
    """Default knobs: every row is in the triple SELL, whose tri and pair
    slices are the predicted ones (ComplexF64: one row per lane, no pairs;
    Float32: 2 rows per lane by the auto rule)."""
    c = get_case(pamd, be, host(O, "run", n, nparts, dtype))
    H, R = slice_rows(dtype)
    for i in c.info:
        assert i["pattern_slices"] == 0 and i["delta16_slices"] == 0, i
        assert i["nslices"] == -(-i["nrows"] // H), i
    for want, got in check_triple_counters(c, H, R):
        print(f"{c.dtype} n={n}: predicted {want}, reported {got}")
        assert (got["pair_rows"] == 0) == (R == 1)
    check_mul(pamd, O, c, alpha, beta)


def _packs(dtype):
    return (7, 4, 1, 0) if np.dtype(dtype) == np.float32 else (7, 0)


@gpu
@pytest.mark.parametrize("merge", [1, 0], ids=["merged", "per_kind"])
@pytest.mark.parametrize("order", [0, 1], ids=["triples_first", "others_first"])
@pytest.mark.parametrize("dtype,pack", [(d, p) for d in (np.float32, np.float64, np.complex64) for p in _packs(d)])
def test_runs_triple_knobs(be, pamd, O, dtype, pack, order, merge):
    """Three parts under spmv_tri_pack (pair slices, Float32 value packs),
    spmv_tri_order and spmv_merge: mul! (-1.3, 0.5), then set_values with
    fresh random values (the triple SELL's copies refreshed into the same
    packs) and mul! (1, 0)."""
    n, nparts = RUNS3
    h = host(O, "run", n, nparts, dtype)
    with _knobs(pamd, f32_rows=2, spmv_tri_pack=pack, spmv_tri_order=order, spmv_merge=merge):
        c = Case(pamd, be, h)
        check_triple_counters(c, 128, 2, order, bool(pack & 4))
        what = f"spmv_tri_pack {pack} spmv_tri_order {order} spmv_merge {merge}"
        check_mul(pamd, O, c, -1.3, 0.5, what)
        rng = np.random.default_rng([SEED, 11, n, pack])
        new = []
        c.V = np.empty_like(h.V)
        for k, (p, s) in enumerate(zip(c.parts.part_ids, h.OA.cols.partition.parts)):
            g = np.asarray(s.lid_to_gid)
            a, b = np.searchsorted(h.I, [g[0], g[h.noids[k] - 1] + 1])  # the part's triplets
            new.append(_rand(rng, b - a, dtype))
            c.A.values.local(p).set_values(new[k])  # nonzeros(A) in CSC order, as the oracle's
            # the triplets again for the long-double reference: CSC order is (column lid, row)
            lid = np.empty(h.n + 1, np.int64)
            lid[g] = np.arange(len(g))
            v = np.empty(b - a, c.V.dtype)
            v[np.lexsort((h.I[a:b], lid[h.J[a:b]]))] = new[k]
            c.V[a:b] = v
        it = iter(new)
        c.OA = O.PSparseMatrix(O.map_parts(lambda M: O.CSC(M.m, M.n, M.colptr, M.rowval, _to_oracle(O, next(it))),
                                           h.OA.values), h.OA.rows, h.OA.cols)
        check_mul(pamd, O, c, 1.0, 0.0, what + " after set_values")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_other_encodings(be, pamd, O, dtype):
    """Three parts with the rows kept in delta16 slices (spmv_tri16 0), in
    int32 slices (spmv_delta16 0), under spmv_format 0 and, Float32, in the
    interleaved 256-row slices (f32_rows 4), each with and without the
    masked tail batch: the oracle's bits every time."""
    n, nparts = RUNS3
    h = host(O, "run", n, nparts, dtype)
    configs = [{"spmv_tri16": 0}, {"spmv_delta16": 0}, {"spmv_format": 0}]
    if np.dtype(dtype) == np.float32:
        configs.append({"f32_rows": 4})
    ys = {}
    for cfg in configs:
        for flags in FLAGS:
            with _knobs(pamd, spmv_flags=flags, **cfg):
                c = Case(pamd, be, h)
                for i in c.info:
                    assert i["pattern_slices"] == 0, i
                    if "spmv_tri16" in cfg:
                        assert i["triple_sell_rows"] == 0 and i["delta16_slices"] == i["nslices"], i
                    if "spmv_delta16" in cfg:
                        assert i["triple_sell_rows"] == 0 and i["delta16_slices"] == 0, i
                    if "f32_rows" in cfg:
                        assert i["nslices"] == -(-i["nrows"] // 256) and i["delta16_slices"] == i["nslices"], i
                for ab in AB:
                    ys[tuple(cfg.items()), flags, ab] = check_mul(pamd, O, c, *ab, f"{cfg} spmv_flags {flags}")
    for (cfg, flags, ab), y in ys.items():
        assert np.array_equal(y, ys[tuple(configs[0].items()), FLAGS[0], ab]), (cfg, flags, ab)


@gpu
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_runs_fused_dot(be, pamd, O, dtype, tol):
    """mul_dot_ on three parts: y is bit-equal to mul_'s and the dot is
    within the project's tolerance for dots (1e-12 relative; Float32 1e-5,
    as test_gpu_drivers compares mul_dot_ with dot) of dot(x, y) in long
    double from the device's own y."""
    n, nparts = RUNS3
    c = get_case(pamd, be, host(O, "run", n, nparts, dtype))
    yref = check_mul(pamd, O, c, 1.0, 0.0)
    x = c.device_x(pamd)
    y = pamd.PVector.from_host(pamd.map_parts(lambda s: _nan(s.num_lids, c.dtype), c.A.rows.partition), c.A.rows)
    d = pamd.mul_dot_(y, c.A, x)
    got = y.to_host()
    for p in c.parts.part_ids:
        s = c.A.rows.partition.local(p)
        own = s.oid_to_lid - 1
        assert np.array_equal(got.local(p)[own], yref[s.lid_to_gid[own] - 1]), p
    ref = np.sum(c.x.astype(np.longdouble) * yref.astype(np.longdouble))
    print(f"run n={n} {c.dtype}: fused dot {d!r}, long double {float(ref)!r}, "
          f"relative difference {float(abs(np.longdouble(d) - ref) / abs(ref)):.3g}")
    assert abs(np.longdouble(d) - ref) <= tol * abs(ref), (d, float(ref))


LAYOUTS = {"Float64": (np.float64, 2), "ComplexF64": (np.complex128, 2), "ComplexF32": (np.complex64, 2),
           "Float32_r2": (np.float32, 2), "Float32_r4": (np.float32, 4)}


@gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("probes", ["owned", "ghost"])
def test_reach_code_limits(be, pamd, O, probes, layout):
    """Columns exactly at the limits of the 16-bit codes.  spmv_tri16 0: the
    delta16 slices of part 1 are those the documented rule accepts.
    spmv_tri16 1, "owned": the accepted slices' rows (those of the slices at
    +16383 and -16384 among them) are in the triple SELL, laid out as
    predicted.  "ghost": the two rows of 5 entries sort into one triple-SELL
    slice whose ghost columns span more than 15 bits, so the triple SELL is
    abandoned after its buffers were built and the delta16 slices stay."""
    dtype, f32_rows = LAYOUTS[layout]
    H, R = slice_rows(dtype, f32_rows)
    h = host(O, "reach", 2 * PER, 2, dtype, probes)
    fit = slice_fit(h.rows(0), H, h.noids[0])[0]
    nfit = [int(np.count_nonzero(fit)), -(-h.noids[1] // H)]
    for tri16 in ((0,) if R == 4 else (0, 1)):
        with _knobs(pamd, f32_rows=f32_rows, spmv_tri16=tri16):
            c = Case(pamd, be, h)
            print(f"{layout} {probes} spmv_tri16 {tri16}: slices accepted by the rule {nfit}, "
                  + ", ".join(str({k: i[k] for k in ("nslices", "delta16_slices", "triple_sell_rows", "tri_rows",
                                                     "pair_rows")}) for i in c.info))
            for k, i in enumerate(c.info):
                assert i["pattern_slices"] == 0 and i["nslices"] == -(-h.noids[k] // H), i
            if tri16 == 0 or probes == "ghost":
                assert c.info[0]["triple_sell_rows"] == 0, c.info[0]
                assert c.info[0]["delta16_slices"] == nfit[0], (c.info[0], nfit)
            else:
                cand = [np.flatnonzero(np.repeat(fit, H)[:h.noids[0]]), np.arange(h.noids[1])]
                for k, i in enumerate(c.info):
                    assert i["delta16_slices"] == 0 and i["triple_sell_rows"] >= len(cand[k]) > 0, (k, i)
                check_triple_counters(c, H, R, rows_of=cand)
            if tri16 == 0:
                assert c.info[1]["delta16_slices"] == nfit[1], c.info[1]
            for ab in AB:
                check_mul(pamd, O, c, *ab, f"{layout} {probes} spmv_tri16 {tri16}")
