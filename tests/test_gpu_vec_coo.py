"""PVector(I, V, rows; ids) and local_view / global_view on the device
(Interfaces.jl:1887-1932, 1994-2069): pa_vec_scatter / pa_vec_gather against
the sequential restatement of tests/vec_coo_ref.py.  Every comparison is bit
for bit (sign of zero included); the only exception is the payload of a NaN
the hardware generates (Inf - Inf), where the positions of the NaNs are
compared."""
import numpy as np
import pytest

import vec_coo_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
NL, N = 1000, 70001  # lids of the part; entries: more than one grid pass (65,536 threads), no multiple of 64


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


def pdata(parts, values):
    return type(parts)(parts.backend, parts.part_ids, list(values), parts.shape)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


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


_ORDER = {}


def order_case(dtype):
    """(lids, V, expected, share of the lids whose bits change when the
    entries are summed in reverse input order); computed once per type"""
    if dtype not in _ORDER:
        rng = np.random.default_rng(7)
        lids = rng.integers(1, NL + 1, size=N)
        V = entries(dtype, N, rng)
        want = R.from_coo(NL, lids, V, dtype)
        rev = R.from_coo(NL, lids[::-1], V[::-1], dtype)
        changed = (R.bits(want).reshape(NL, -1) != R.bits(rev).reshape(NL, -1)).any(axis=1).mean()
        for a in (lids, V, want):
            a.setflags(write=False)
        _ORDER[dtype] = lids, V, want, changed
    return _ORDER[dtype]


@pytest.mark.parametrize("wide", [0, 1], ids=["keys32", "keys64"])
@pytest.mark.parametrize("idkind", ["local32", "local64", "global"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_order_sensitive_accumulation(be, pamd, dtype, idkind, wide):
    lids, V, want, changed = order_case(dtype)
    print(f"{np.dtype(dtype).name}: reverse order changes {100 * changed:.1f} % of the lids")
    assert changed >= 0.5  # an unordered sum would not reproduce `want`
    parts, rows = one_part_rows(pamd, be, NL)
    s = rows.partition.parts[0]
    if idkind == "global":
        I, ids = s.lid_to_gid[lids - 1].copy(), "global"
    else:
        I, ids = lids.astype(np.int32 if idkind == "local32" else np.int64), "local"
    prev = pamd._lib.tune("scatter_wide", wide)
    try:
        v = pamd.PVector.from_coo(pdata(parts, [I]), pdata(parts, [V]), rows, ids=ids)
    finally:
        pamd._lib.tune("scatter_wide", prev)
    assert same_bits(v.to_host().parts[0], want)
    if idkind == "global":  # translated in place, as to_lids!
        assert np.array_equal(I, lids)


def test_edges(be, pamd):
    parts, rows = one_part_rows(pamd, be, 37)
    mk = lambda a: pdata(parts, [a])
    s = rows.partition.parts[0]
    # n = 0
    for ids in ("local", "global"):
        v = pamd.PVector.from_coo(mk(np.zeros(0, np.int64)), mk(np.zeros(0)), rows, ids=ids)
        assert same_bits(v.to_host().parts[0], np.zeros(37))
    # all entries on one lid; untouched lids are exactly zero
    rng = np.random.default_rng(11)
    for dtype in DTYPES:
        V = entries(dtype, 5000, rng)
        I = np.full(5000, 17, np.int32)
        v = pamd.PVector.from_coo(mk(I), mk(V), rows, ids="local")
        got = v.to_host().parts[0]
        assert same_bits(got, R.from_coo(37, I, V, dtype))
        assert not R.bits(np.delete(got, 16)).any()
    # a single -0.0 entry gives +0.0 (zero(T) + -0.0); -0.0 added onto -0.0 stays -0.0
    for dtype in (np.float32, np.float64):
        v = pamd.PVector.from_coo(mk(np.array([5])), mk(np.array([-0.0], dtype)), rows, ids="local")
        got = v.to_host().parts[0]
        assert not R.bits(got).any()
        w = pamd.PVector.from_host(mk(np.full(37, -0.0, dtype)), rows)
        pamd.add_coo_(w, mk(np.array([5, 9, 5])), mk(np.array([-0.0, 1.5, -0.0], dtype)), ids="local")
        want = R.scatter_add(np.full(37, -0.0, dtype), [5, 9, 5], np.array([-0.0, 1.5, -0.0], dtype))
        got = w.to_host().parts[0]
        assert same_bits(got, want) and np.signbit(got[4]) and np.signbit(got[0])
    # NaN and Inf propagate
    I = np.array([1, 2, 2, 3, 3, 4, 4, 2], np.int64)
    V = np.array([np.nan, np.inf, 1.0, np.inf, -np.inf, -np.inf, 3.0, 2.0])
    got = pamd.PVector.from_coo(mk(s.lid_to_gid[I - 1].copy()), mk(V), rows, ids="global").to_host().parts[0]
    with np.errstate(invalid="ignore"):
        want = R.from_coo(37, I, V, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and list(np.flatnonzero(np.isnan(want))) == [0, 2]
    ok = ~np.isnan(want)
    assert same_bits(got[ok], want[ok]) and got[1] == np.inf and got[3] == -np.inf


def test_parts_without_lids(be, pamd):
    parts = be.get_part_ids(4)
    rows = pamd.prange_linear(parts, 2)  # parts 1 and 2 own nothing
    nl = [s.num_lids for s in rows.partition.parts]
    assert nl == [0, 0, 1, 1]
    I = pdata(parts, [np.zeros(0, np.int64), np.zeros(0, np.int64), np.array([1, 1]), np.array([2, 2, 2])])
    V = pdata(parts, [np.zeros(0), np.zeros(0), np.array([0.1, 0.2]), np.array([0.1, 0.2, 0.3])])
    v = pamd.PVector.from_coo(I, V, rows, ids="global")
    got = v.to_host().parts
    assert got[0].shape == (0,) and got[1].shape == (0,)
    assert same_bits(got[2], np.array([0.1 + 0.2])) and same_bits(got[3], np.array([(0.1 + 0.2) + 0.3]))
    assert pamd.local_view(v).parts[0].get(np.zeros(0, np.int64)).shape == (0,)
    # an entry for a part without lids has no lid to land on
    dv = v.values.parts[0]
    with pytest.raises(pamd.PAError):
        pamd.local_view(v).parts[0].add_([1], [1.0])
    with pytest.raises(pamd.PAError):
        pamd.global_view(v).parts[0].add_([1], [1.0])
    assert dv.download().shape == (0,)


def layout_rows(pamd, parts, kind, rng):
    if kind == "with_ghost":  # owned and ghost lids interleave
        return pamd.prange_cartesian(parts, (9, 7), with_ghost=True)
    rows = pamd.prange_cartesian(parts, (9, 7))  # ghosts appended by add_gids!
    touched = pdata(parts, [rng.integers(1, 64, size=40) for _ in parts.part_ids])
    return pamd.add_gids_(rows, touched)


@pytest.mark.parametrize("kind", ["add_gids", "with_ghost"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex64], ids=lambda d: d.__name__)
def test_layouts_with_ghosts_and_assemble(be, pamd, kind, dtype):
    parts = be.get_part_ids((2, 2))
    rng = np.random.default_rng(5)
    rows = layout_rows(pamd, parts, kind, rng)
    sets = rows.partition.parts
    assert all(s.num_hids > 0 for s in sets)
    lids = [rng.integers(1, s.num_lids + 1, size=333) for s in sets]
    V = [entries(dtype, 333, rng) for _ in sets]
    want = [R.from_coo(s.num_lids, l, w, dtype) for s, l, w in zip(sets, lids, V)]
    assert all(R.bits(w[s.hid_to_lid - 1]).any() for s, w in zip(sets, want))  # entries land on ghost lids
    G = [s.lid_to_gid[l - 1].copy() for s, l in zip(sets, lids)]
    b = pamd.PVector.from_coo(pdata(parts, G), pdata(parts, V), rows, ids="global")
    b2 = pamd.PVector.from_coo(pdata(parts, [l.astype(np.int32) for l in lids]), pdata(parts, V), rows, ids="local")
    for p in range(4):
        assert same_bits(b.to_host().parts[p], want[p]) and same_bits(b2.to_host().parts[p], want[p])
        assert np.array_equal(G[p], lids[p])
    h = pamd.PVector.from_host(pdata(parts, want), rows)
    pamd.assemble_(b)
    pamd.assemble_(h)
    for p in range(4):
        assert same_bits(b.to_host().parts[p], h.to_host().parts[p])
    assert any(R.bits(x).any() for x in b.to_host().parts)


def test_set_with_duplicates_and_get(be, pamd):
    parts, rows = one_part_rows(pamd, be, 50)
    s = rows.partition.parts[0]
    rng = np.random.default_rng(13)
    for dtype in DTYPES:
        start = entries(dtype, 50, rng)
        v = pamd.PVector.from_host(pdata(parts, [start]), rows)
        lids = rng.integers(1, 51, size=2001)
        V = entries(dtype, 2001, rng)
        want = R.scatter_set(start.copy(), lids, V)
        assert len(np.unique(lids)) < len(lids)
        ids0 = lids.copy()
        pamd.local_view(v).parts[0].set_(lids, V)
        assert np.array_equal(lids, ids0)  # a view leaves the caller's ids alone
        assert same_bits(v.to_host().parts[0], want)
        # the same through global ids, on top
        V2 = entries(dtype, 2001, rng)
        g = s.lid_to_gid[lids - 1]
        g0 = g.copy()
        pamd.global_view(v, v.rows).parts[0].set_(g, V2)
        assert np.array_equal(g, g0)
        want = R.scatter_set(want, lids, V2)
        assert same_bits(v.to_host().parts[0], want)
        # get returns the stored values (Int32, Int64 lids and gids)
        q = rng.integers(1, 51, size=777)
        for ids in (q.astype(np.int32), q.astype(np.int64)):
            assert same_bits(pamd.local_view(v, v.rows).parts[0].get(ids), R.gather(want, q))
        assert same_bits(pamd.global_view(v).parts[0].get(s.lid_to_gid[q - 1]), R.gather(want, q))
        # add_ through a view, duplicates in input order
        V3 = entries(dtype, 2001, rng)
        pamd.global_view(v).parts[0].add_(g, V3)
        assert same_bits(v.to_host().parts[0], R.scatter_add(want, lids, V3))
    other = pamd.prange_linear(parts, 50)
    with pytest.raises(NotImplementedError):
        pamd.global_view(v, other)


def kat_vector(pamd, be):
    """test_interfaces.jl:308-346, 501-503 on its 4 parts: the three
    constructor calls; returns (parts, v, the states of gids)"""
    parts = be.get_part_ids(4)
    g = [[1, 4, 6], [3, 1, 2, 8], [1, 9, 6], [3, 2, 8, 10]]
    gids = pdata(parts, [np.array(x, np.int64) for x in g])
    ids3 = pamd.add_gids(pamd.prange_linear(parts, 10), gids)
    fcopy = lambda: pdata(parts, [a.astype(np.float64) for a in gids.parts])
    states = [[a.copy() for a in gids.parts]]
    vs = []
    for rows_or_n, ids in ((ids3, "global"), (ids3, "local"), (10, "global")):
        V = fcopy()
        vs.append((pamd.PVector.from_coo(gids, V, rows_or_n, ids=ids), [a.copy() for a in V.parts]))
        states.append([a.copy() for a in gids.parts])
    return parts, ids3, vs, states


def test_kat_sequence_test_interfaces_501_520(be, pamd):
    parts, ids3, vs, states = kat_vector(pamd, be)
    sets3 = ids3.partition.parts
    # I becomes lids after the first call
    assert [list(a) for a in states[1]] == [list(R.to_lids(s.lid_to_gid, a)) for s, a in zip(sets3, states[0])]
    assert [list(a) for a in states[1]] == [[1, 3, 4], [1, 3, 4, 5], [4, 5, 2], [4, 5, 1, 3]]
    assert [list(a) for a in states[2]] == [list(a) for a in states[1]]  # ids=:local leaves I alone
    (v1, V1), (v2, V2), (v3, V3) = vs
    for p, s in enumerate(sets3):
        assert same_bits(v1.to_host().parts[p], R.from_coo(s.num_lids, states[1][p], V1[p], np.float64))
        assert same_bits(v2.to_host().parts[p], R.from_coo(s.num_lids, states[1][p], V2[p], np.float64))
    for p, s in enumerate(v3.rows.partition.parts):
        assert list(states[3][p]) == list(R.to_lids(s.lid_to_gid, states[2][p]))
        assert same_bits(v3.to_host().parts[p], R.from_coo(s.num_lids, states[3][p], V3[p], np.float64))
    assert pamd.maximum(v3) == 5 and pamd.minimum(v3) == 0


def test_local_view_over_a_permuted_subrange(be, pamd):
    """test_interfaces.jl:594-609: [6, 7, 8] written through local_view(subv,
    v.rows) land at perm, and read back; ids subv does not store read zero"""
    parts, _, vs, _ = kat_vector(pamd, be)
    v = vs[2][0]
    perm = np.array([3, 1, 2])
    sub = pamd.map_parts(lambda s: pamd.IndexSet(s.part, s.lid_to_gid[perm - 1], s.lid_to_part[perm - 1]),
                         v.rows.partition)
    subrows = pamd.prange_from_partition(len(v.rows), sub, ghost=False)
    subv = pamd.PVector.full(1.0, subrows)
    views = pamd.local_view(subv, v.rows)
    for w in views.parts:
        w.set_([1, 2, 3], [6.0, 7.0, 8.0])
    for a in subv.to_host().parts:
        assert list(a[np.array([2, 3, 1]) - 1]) == [6.0, 7.0, 8.0]
    for w, s in zip(views.parts, v.rows.partition.parts):
        assert same_bits(w.get([1, 2, 3]), np.array([6.0, 7.0, 8.0]))
        assert s.num_lids >= 4
        assert same_bits(w.get([4, 1, s.num_lids]), np.array([0.0, 6.0, 0.0]))  # absent ids read as zero
        before = subv.values.parts[s.part - 1].download()
        with pytest.raises(pamd.PAError):  # ... and cannot be written (Interfaces.jl:2027-2031)
            w.set_([1, 4], [9.0, 9.0])
        with pytest.raises(pamd.PAError):
            w.add_([2, 4, 2], [9.0, 9.0, 9.0])
        with pytest.raises(pamd.PAError):
            w.get([0])
        assert same_bits(subv.values.parts[s.part - 1].download(), before)


def test_errors_leave_the_vector_unchanged(be, pamd):
    parts, rows = one_part_rows(pamd, be, 64)
    s = rows.partition.parts[0]
    rng = np.random.default_rng(17)
    mk = lambda a: pdata(parts, [a])
    for dtype in (np.float32, np.complex128):
        start = entries(dtype, 64, rng)
        v = pamd.PVector.from_host(mk(start), rows)
        V = entries(dtype, 300, rng)
        good = rng.integers(1, 65, size=300)
        for bad_lid in (0, 65):
            I = good.copy()
            I[250] = bad_lid
            for ids in (I.astype(np.int32), I.astype(np.int64)):
                with pytest.raises(pamd.PAError, match="BoundsError"):
                    pamd.add_coo_(v, mk(ids), mk(V), ids="local")
                with pytest.raises(pamd.PAError, match="BoundsError"):
                    pamd.local_view(v).parts[0].set_(ids, V)
                with pytest.raises(pamd.PAError, match="BoundsError"):
                    pamd.local_view(v).parts[0].get(ids)
                assert same_bits(v.to_host().parts[0], start)
        G = s.lid_to_gid[good - 1].copy()
        G[7] = 1000  # not a gid of the part
        G0 = G.copy()
        with pytest.raises(pamd.PAError, match="KeyError"):
            pamd.add_coo_(v, mk(G), mk(V), ids="global")
        assert np.array_equal(G, G0)  # not translated either
        with pytest.raises(pamd.PAError, match="KeyError"):
            pamd.global_view(v).parts[0].set_(G, V)
        with pytest.raises(pamd.PAError, match="KeyError"):
            pamd.global_view(v).parts[0].get(G)
        with pytest.raises(pamd.PAError, match="KeyError"):
            pamd.PVector.from_coo(mk(G), mk(V), rows, ids="global")
        assert same_bits(v.to_host().parts[0], start)


def test_device_inputs_give_the_same_bits(be, pamd):
    parts, rows = one_part_rows(pamd, be, 200)
    s = rows.partition.parts[0]
    ctx = pamd.device.contexts(rows.partition)[0]
    rng = np.random.default_rng(19)
    DV = pamd.device.DeviceVector

    def on_device(a):
        """the array's bytes in a DeviceVector of 4-byte words: the address of
        its values is what a caller with its own device arrays passes"""
        words = np.ascontiguousarray(a).view(np.float32)
        holder = DV(ctx, np.float32, words.size)
        holder.upload(words)
        return holder, holder.as_array(a.dtype)

    for dtype in DTYPES:
        lids = rng.integers(1, 201, size=4099)
        V = entries(dtype, 4099, rng)
        G = s.lid_to_gid[lids - 1].copy()
        host = pamd.PVector.from_coo(pdata(parts, [G.copy()]), pdata(parts, [V]), rows, ids="global")
        want = host.to_host().parts[0]
        assert same_bits(want, R.from_coo(200, lids, V, dtype))
        hv, dVals = on_device(V)
        for ids, glob, idt in ((G, "global", np.int64), (lids.astype(np.int32), "local", np.int32),
                               (lids.astype(np.int64), "local", np.int64)):
            hi, dI = on_device(ids)
            dev = pamd.PVector.from_coo(pdata(parts, [dI]), pdata(parts, [dVals]), rows, ids=glob)
            assert same_bits(dev.to_host().parts[0], want)
            # gids are translated in place on the device; lids stay
            assert np.array_equal(hi.download().view(idt), lids.astype(idt))
            out = DV(ctx, dtype, 4099)
            idx = pamd.device.device_index(ctx, s)
            dev.values.parts[0].gather(idx, dI, out=out.as_array())
            assert same_bits(out.download(), R.gather(want, lids))


@pytest.mark.parametrize("shape", [(2, 2), 4], ids=["cartesian", "linear"])
def test_driver_rhs_from_coo(be, pamd, shape):
    parts = be.get_part_ids(shape)
    A, b, x0, _ = pamd.drivers.fem_sa_problem(parts, 10)
    parts = be.get_part_ids(shape)
    A2, b2, x02, _ = pamd.drivers.fem_sa_problem_coo_rhs(parts, 10)
    for p, q in zip(b.to_host().parts, b2.to_host().parts):
        assert same_bits(p, q) and R.bits(p).any()
    pamd.cg_(x0, A, b)
    pamd.cg_(x02, A2, b2)
    for p, q in zip(x0.to_host().parts, x02.to_host().parts):
        assert same_bits(p, q)
