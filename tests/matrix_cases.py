"""Matrix generators shared by the GPU test modules (plain helpers, no
fixtures): each returns host triplets or a host CSR; the tests build the
device matrices from them.  Below them the checks the parity tests share
(the long-double reference and its bound, the oracle conversions) and the
layout specifications of the run matrices."""
import contextlib

import numpy as np

SEED = 20250114


def rand(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def long_row_coo(rng, part, p, dtype, long_lens):
    """owned rows with ~9 entries, a few rows with long_lens entries (over all
    local columns, ghosts included), in random order with duplicates."""
    s = part.partition.local(p)
    own = s.oid_to_lid
    I, J = [], []
    longs = rng.choice(own, size=min(len(long_lens), len(own)), replace=False)
    for li in own:
        k = 9
        if li in longs:
            k = long_lens[list(longs).index(li)]
        I += [li] * k
        J += list(rng.integers(1, s.num_lids + 1, size=k))
    I, J = np.array(I), np.array(J)
    o = rng.permutation(len(I))
    V = rng.uniform(-1, 1, len(I))
    if np.dtype(dtype).kind == "c":
        V = V + 1j * rng.uniform(-1, 1, len(I))
    return I[o], J[o], V[o].astype(dtype), sorted(int(v) for v in longs)


def unsorted_csr(n, D, Bi, order, dtype):
    """rowptr, colval (Bi-based), nzval of the band matrix with every row
    stored diagonal first and the others ascending, or descending; the
    triplets in that order too."""
    rows, cols = [], []
    for i in range(n):
        js = [i + d for d in sorted(D) if 0 <= i + d < n]
        js = ([i] + [j for j in js if j != i]) if order == "diag_first" else js[::-1]
        rows += [i] * len(js)
        cols += js
    I, J = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=n))]).astype(np.int64) + Bi
    rng = np.random.default_rng([SEED, 13, n, len(D)])
    V = rand(rng, len(I), dtype)
    return rowptr, J + Bi, V, I + 1, J + 1, rand(rng, n, dtype)


def with_ghost_coo(rows, parts, ngids, periodic, rng):
    """global-id COO of a 7-point operator with random coefficients over each
    part's owned rows (neighbours wrap around periodic dimensions)."""
    D = len(ngids)
    per = periodic or (False,) * D
    I, J, V = {}, {}, {}
    for p in parts.part_ids:
        s = rows.partition.local(p)
        own = s.lid_to_gid[s.oid_to_lid - 1]
        ci = [(own - 1) // int(np.prod(ngids[:d])) % ngids[d] for d in range(D)]
        ii, jj = [own], [own]
        for d in range(D):
            for step in (-1, 1):
                c = ci[d] + step
                ok = np.ones(len(own), bool) if per[d] else (c >= 0) & (c < ngids[d])
                c = c % ngids[d]
                nb = own + (c - ci[d]) * int(np.prod(ngids[:d]))
                ii.append(own[ok])
                jj.append(nb[ok])
        I[p] = np.concatenate(ii)
        J[p] = np.concatenate(jj)
        V[p] = rng.uniform(-1, 1, len(I[p]))
    return I, J, V


def tridiag(n, part_rows):
    """global-id COO of the owned rows of a 1-D Laplacian-like matrix."""
    I, J, V = [], [], []
    for g in part_rows:
        for d, v in ((-1, -1.0), (0, 4.0), (1, -1.5)):
            if 1 <= g + d <= n:
                I.append(g)
                J.append(g + d)
                V.append(v + 0.01 * g)
    return np.array(I, np.int64), np.array(J, np.int64), np.array(V)


# ---------------------------------------------------------------------------
# shared checks of the parity tests (test_gpu_band, test_gpu_runs)

@contextlib.contextmanager
def _knobs(pamd, **kw):
    """pa_tune knobs for the body, every one restored afterwards."""
    prev = []
    try:
        for k, v in kw.items():
            prev.append((k, pamd._lib.tune(k, v)))
        yield
    finally:
        for k, v in reversed(prev):
            pamd._lib.tune(k, v)


def _real(dtype):
    return np.float32 if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64


def _nan(n, dtype):
    v = np.empty(n, dtype)
    v[:] = np.nan + (1j * np.nan if np.dtype(dtype).kind == "c" else 0)
    return v


def _to_oracle(O, a):
    return O.Cx(a.real.copy(), a.imag.copy()) if np.iscomplexobj(a) else a.copy()


def _eq(O, got, ref):
    if isinstance(ref, O.Cx):
        return np.array_equal(got.real, ref.re) and np.array_equal(got.imag, ref.im)
    return np.array_equal(got, ref)


def _sel(O, ref, idx):
    return O.Cx(ref.re[idx], ref.im[idx]) if isinstance(ref, O.Cx) else ref[idx]


def _as_array(O, ref):
    return ref.re + 1j * ref.im if isinstance(ref, O.Cx) else ref


def ref_longdouble(n, I, J, V, x):
    """y = A*x straight from the triplets in extended precision (no code of
    the oracle's): the sums, Σ|v||x| and the entry count of every row."""
    wide = np.clongdouble if np.iscomplexobj(V) else np.longdouble
    v, xj = V.astype(wide), x.astype(wide)[J - 1]
    y = np.zeros(n, wide)
    np.add.at(y, I - 1, v * xj)
    mag = np.zeros(n, np.longdouble)
    np.add.at(mag, I - 1, np.abs(v).astype(np.longdouble) * np.abs(xj).astype(np.longdouble))
    return y, mag, np.bincount(I - 1, minlength=n)


def check_bound(y, n, I, J, V, x, what):
    """|y[i] - y_ref[i]| <= k_i * eps * Σ|v||x|: recursive summation of a row
    of k terms has relative error γ_k ~ k*u of Σ|v||x| with unit roundoff
    u = eps/2 (one more for the product), so k_i = entries + 1 leaves a factor
    2; a complex product carries about 2.8 unit roundoffs: entries + 4."""
    yref, mag, cnt = ref_longdouble(n, I, J, V, x)
    eps = np.finfo(_real(V.dtype)).eps
    k = cnt + (4 if np.iscomplexobj(V) else 1)
    err = np.abs(y.astype(yref.dtype) - yref).astype(np.longdouble)
    bound = k * np.longdouble(eps) * mag
    worst = float(np.max(err / np.maximum(bound, np.finfo(np.longdouble).tiny)))
    print(f"{what}: largest error / bound = {worst:.3g}")
    bad = np.flatnonzero(~(err <= bound))  # a NaN fails
    assert bad.size == 0, f"{what}: {bad.size} rows miss the long-double bound, first gid {bad[0] + 1}: " \
                          f"error {float(err[bad[0]]):.3e}, bound {float(bound[bad[0]]):.3e}"


# ---------------------------------------------------------------------------
# run matrices: rows made of short column runs (test_gpu_runs)

TRI_LENS = (1, 2, 3, 4, 5, 8, 9, 10, 13, 18, 19)  # triples per row of a triple group
OTHER_RUNS = ((1,), (2,), (4,), (5,), (2, 1), (4, 2), (1, 1, 1), (3, 3, 1), (3, 2), (5, 4), (3, 4, 5, 3), (2,) * 7)
GROUP_SIZES = (2, 1, 2, 3, 1, 2, 1, 3)  # consecutive rows per group: a third of the rows stay unpaired
RUN_REACH = 200  # run starts lie within this many columns of the group's first row
FAR = 216  # first column past a part's end that no row placed by the window reaches (200 + 1 + 2 + 4 < 216)
HAND_NTRI = 5  # triples per row of the hand-placed groups (one batch of 4 plus 1; below a batch of 9)


def linear_bounds(n, nparts):
    """first and last gid (1-based, inclusive) of every part of prange_linear(parts, n)."""
    q, rem = divmod(n, nparts)
    out, a = [], 1
    for p in range(1, nparts + 1):
        m = q + (0 if rem < nparts - p + 1 else 1)
        out.append((a, a + m - 1))
        a += m
    return out


def run_coo(n, nparts, dtype, seed):
    """Global COO (1-based gids, rows ascending, columns ascending within a
    row) of a matrix whose rows are short runs of consecutive columns, with
    distinct seeded uniform(-1, 1) values, and a global x.

    Rows come in groups of GROUP_SIZES consecutive rows inside one part of
    prange_linear; row r of a group has the group's runs shifted by r, so
    rows r, r + 1 are a pair of the triple SELL.  Three groups in four are
    triple groups (TRI_LENS runs of length 3), the fourth an "other" group
    (OTHER_RUNS).  Run starts: a grid of spacing 8 in [row - 200, row + 200]
    without replacement, plus 0 or 1, so the runs of a row never touch.

    Hand-placed (HAND_NTRI triples, all other runs on the part's own columns
    so that the ghosts they touch get the lids described): the first group
    of part k (0-based; 2 rows for even k, 1 row for odd k) starts its first
    run at the part's first gid (lid 0) and, when another part follows, ends
    with the run (b-1, b, b+1) on the part's last gid b: b+1 is the first
    ghost the part touches (lid noids).  The last group of part k (same
    sizes) ends with a run from b + FAR, gids no earlier row touches: the
    last lids of x; in the last part with a run that ends at column n."""
    rng = np.random.default_rng([SEED, seed, n, nparts])
    I, J = [], []
    nt = no = 0  # triple / other groups so far (each kind cycles through its lengths and GROUP_SIZES on its own)
    q = 0

    def emit(i, g, starts, runs):
        for r in range(g):
            for s, L in zip(starts, runs):
                I.extend([i + r] * L)
                J.extend(range(int(s) + r, int(s) + r + L))

    def draw(lo, hi, k):
        """k run starts in [lo, hi + 1], ascending, at least 7 apart"""
        slots = np.sort(rng.choice((hi - lo) // 8 + 1, size=k, replace=False))
        return lo + 8 * slots + rng.integers(0, 2, k)

    for k, (a, b) in enumerate(linear_bounds(n, nparts)):
        gh = 2 if k % 2 == 0 else 1  # rows of the part's hand-placed groups
        last = k == nparts - 1
        assert b - a + 1 >= 2 * RUN_REACH + 2 * gh and (last or n - b >= FAR + 8)
        hand = (3,) * HAND_NTRI
        # first group: lid 0, and the straddle of the owned/ghost boundary
        starts = draw(a + 8, a + RUN_REACH, HAND_NTRI)
        starts[0] = a
        if not last:
            starts[-1] = b - 1
        emit(a, gh, starts, hand)
        i = a + gh
        end = b - gh  # last row of the generated groups
        while i <= end:
            other = q % 4 == 3
            if other:
                runs, g = OTHER_RUNS[no % len(OTHER_RUNS)], GROUP_SIZES[no % len(GROUP_SIZES)]
                no += 1
            else:
                runs, g = (3,) * TRI_LENS[nt % len(TRI_LENS)], GROUP_SIZES[nt % len(GROUP_SIZES)]
                nt += 1
            q += 1
            g = min(g, end - i + 1)
            starts = draw(max(1, i - RUN_REACH), min(n - 7, i + RUN_REACH), len(runs))
            emit(i, g, starts, runs)
            i += g
        # last group: the run that ends at the last lid of x
        i = b - gh + 1
        starts = draw(b - RUN_REACH, b - 16, HAND_NTRI)
        starts[-1] = (n - (gh - 1) - 2) if last else b + FAR
        emit(i, gh, starts, hand)
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    assert J.min() >= 1 and J.max() <= n and np.all(np.diff(I) >= 0)
    assert np.all((np.diff(J) > 0) | (np.diff(I) > 0))
    return I, J, rand(rng, len(I), dtype), rand(rng, n, dtype)


def reach_rows(per, probes):
    """The probe rows of reach_coo: {row: extra owned column} in four
    different 256-row blocks (rows without a ghost column, i % 3 == 1), and
    for probes == "ghost" {row: ghost rows back}: the last ghost row of a
    256-row block (block 192 or later) reads the ghost first touched 32766,
    or 32767, ghost rows earlier."""
    own = {256 * 2 + 8: 16383, 256 * 4 + 9: 16384, 256 * 70 + 9: -16384, 256 * 72 + 10: -16385}
    assert all(i % 3 == 1 for i in own)
    back = {}
    if probes == "ghost":
        for blk, g in ((196, 32766), (200, 32767)):
            i = 256 * (blk + 1)
            back[i if i % 3 != 1 else i - 1] = g
    assert probes in ("owned", "ghost") and max(list(own) + list(back)) <= per
    return {i: i + d for i, d in own.items()}, back


def reach_coo(per, dtype, probes):
    """Two linear parts of `per` rows.  Every row has one triple at row +
    jitter (|jitter| <= 100, clipped to its own part); the rows i of part 1
    with i % 3 != 1 also read the ghost column per + i, so the ghost lids
    ascend with the row; part 2 has no ghosts.  probes: reach_rows."""
    n = 2 * per
    rng = np.random.default_rng([SEED, 99, per])
    own, back = reach_rows(per, probes)
    i = np.arange(1, n + 1, dtype=np.int64)
    lo = np.where(i <= per, 1, per + 1)
    s = np.clip(i + rng.integers(-100, 101, n), lo, lo + per - 3)
    grows = i[(i <= per) & (i % 3 != 1)]
    rows = [i, i, i, grows]
    cols = [s, s + 1, s + 2, per + grows]
    for r, c in own.items():
        assert not s[r - 1] <= c <= s[r - 1] + 2
        rows.append([r])
        cols.append([c])
    for r, g in back.items():
        k = int(np.searchsorted(grows, r))
        assert grows[k] == r
        rows.append([r])
        cols.append([per + grows[k - g]])
    I, J = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64)
    o = np.lexsort((J, I))
    I, J = I[o], J[o]
    assert J.min() >= 1 and J.max() <= n
    return I, J, rand(rng, len(I), dtype), rand(rng, n, dtype)


def rows_of_csc(M, noids):
    """The 0-based column lids of each of the first noids rows of a CSC
    matrix (the oracle's, 1-based rowval), ascending: the storage order of
    the device's rows."""
    colptr, rowval = np.asarray(M.colptr), np.asarray(M.rowval) - 1
    cols = np.repeat(np.arange(M.n), np.diff(colptr))
    o = np.lexsort((cols, rowval))
    r, c = rowval[o], cols[o]
    cut = np.searchsorted(r, np.arange(noids + 1))
    return [c[cut[k]:cut[k + 1]] for k in range(noids)]


def classify_rows(lids_per_row, noids):
    """Per row (its 0-based column lids in storage order): (entries, regular,
    lids); regular: entries % 3 == 0, at least one triple and every triple
    (c, c+1, c+2) consecutive lids (an owned/ghost straddle counts: ghost
    lids follow the owned ones)."""
    out = []
    for c in lids_per_row[:noids]:
        c = np.asarray(c, np.int64)
        t = c[:len(c) - len(c) % 3].reshape(-1, 3)
        reg = len(c) > 0 and len(c) % 3 == 0 and bool(np.all(t[:, 1:] == t[:, :1] + (1, 2)))
        out.append((len(c), reg, c))
    return out


def slice_fit(rows, H, noids):
    """The delta16 rule per H-row slice: every owned column within [-16384,
    16383] of its row, every ghost column within 32766 of the slice's
    smallest ghost column.  Returns fit, dmin, dmax, ghost span per slice
    (0 where the slice has no owned, or no ghost, column)."""
    ns = -(-noids // H)
    fit, dmin, dmax, span = np.ones(ns, bool), np.zeros(ns, np.int64), np.zeros(ns, np.int64), np.zeros(ns, np.int64)
    for s in range(ns):
        sl = [np.asarray(c, np.int64) for c in rows[s * H:(s + 1) * H]]
        c = np.concatenate(sl)
        r = np.repeat(np.arange(s * H, s * H + len(sl)), [len(c) for c in sl])
        d, g = (c - r)[c < noids], c[c >= noids]
        if d.size:
            dmin[s], dmax[s] = d.min(), d.max()
        if g.size:
            span[s] = g.max() - g.min()
        fit[s] = dmin[s] >= -16384 and dmax[s] <= 16383 and span[s] <= 32766
    return fit, dmin, dmax, span


def predict_triple_sell(classes, H, R, tri_order, pairs_on):
    """The triple SELL of rows classified by classify_rows:
    [(kind, length, real rows, shortest real row)] per slice, kind "other" /
    "tri" / "pair".
    Pairs: rows i, i + 1 both regular, of one length, row i + 1's lids row
    i's plus one, taken greedily in oid order (pairs_on: 2 rows per lane and
    spmv_tri_pack bit 2).  Singles: others and regular rows (tri_order 0:
    regular first), each by length descending, then oid, H per slice; a
    slice is "tri" when all its rows are regular and its length divides by
    3.  Pairs by length descending, then oid, from a slice boundary, 64 per
    slice.  [] when fewer than a quarter of the rows are regular."""
    n = len(classes)
    paired = np.zeros(n, bool)
    pairs = []
    for i in range(n - 1 if pairs_on and R == 2 else 0):
        (la, ra, ca), (lb, rb, cb) = classes[i], classes[i + 1]
        if not paired[i] and ra and rb and la == lb and np.array_equal(ca + 1, cb):
            pairs.append(i)
            paired[i] = paired[i + 1] = True
    if 4 * sum(1 for c in classes if c[1]) < n:
        return []
    first = (lambda c: not c[1]) if tri_order == 0 else (lambda c: c[1])  # sorts False first
    singles = sorted((i for i in range(n) if not paired[i]), key=lambda i: (first(classes[i]), -classes[i][0], i))
    out = []
    for k in range(0, len(singles), H):
        cs = [classes[i] for i in singles[k:k + H]]
        L = max(c[0] for c in cs)
        out.append(("tri" if all(c[1] for c in cs) and L % 3 == 0 else "other", L, len(cs), min(c[0] for c in cs)))
    pairs.sort(key=lambda i: (-classes[i][0], i))
    for k in range(0, len(pairs), 64):
        Ls = [classes[i][0] for i in pairs[k:k + 64]]
        out.append(("pair", max(Ls), 2 * len(Ls), min(Ls)))
    return out


def triple_counters(layout):
    """info()'s tri_slices, tri_rows, pair_slices, pair_rows of a predicted layout."""
    tri = [s for s in layout if s[0] != "other"]
    pair = [s for s in layout if s[0] == "pair"]
    return {"tri_slices": len(tri), "tri_rows": sum(s[2] for s in tri),
            "pair_slices": len(pair), "pair_rows": sum(s[2] for s in pair)}
