"""exchange!(I, J, V, rows) on the device (Interfaces.jl:2494-2592,
pa_coo_exchange_all): the triplets of the rows other parts hold as ghosts go
to those parts (segments in rows.exchanger.parts_snd order, input order
inside; a row several neighbours hold goes to the last of them only), the
sender keeps its entry, an unsent ghost-row triplet's value becomes +0, and
every part appends what it receives in parts_rcv order.  Compared bit for
bit against the literal restatement of the reference (coo_exchange_ref.py,
pinned by tests/test_coo_exchange_host.py)."""
import numpy as np
import pytest

from coo_exchange_ref import classify, exchange_coo_, oracle_lists, problem

pytestmark = pytest.mark.gpu

SEED = 20250114


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


def _check(pamd, O, parts, oparts, rows, orows, I, J, V, mk):
    """device against the restatement: I, J as lists, V by bytes, per part.
    Returns (moved, zeroed, sent triplets whose lid sits in >= 2 segments)."""
    coo = pamd.COO.from_host(mk(I), mk(J), mk(V), rows)
    assert pamd.exchange_(coo, rows) is coo
    gI, gJ, gV = coo.to_host()
    rI, rJ, rV = exchange_coo_(O, *oracle_lists(O, parts.part_ids, oparts, I, J, V), orows)
    cls = classify(orows, parts.part_ids, I)
    moved = zeroed = multi = 0
    for p in parts.part_ids:
        assert gI.local(p).tolist() == list(rI[p]), f"part {p}: I differs"
        assert gJ.local(p).tolist() == list(rJ[p]), f"part {p}: J differs"
        ref = np.asarray(rV[p], dtype=gV.local(p).dtype)
        assert gV.local(p).dtype == V[p].dtype
        assert gV.local(p).tobytes() == ref.tobytes(), f"part {p}: V differs"
        kind, nlisted = cls[p]
        moved += len(gI.local(p)) - len(I[p])
        zeroed += int((kind == 2).sum())
        multi += int(((kind == 1) & (nlisted >= 2)).sum())
    return moved, zeroed, multi


CASES = [
    (4, 2000, 1500, False, np.float64),
    (4, 2000, 1500, False, np.complex128),
    ((2, 2), (30, 28), 1500, True, np.float64),
    ((2, 2), (30, 28), 1500, True, np.float32),
    ((2, 2, 2), (12, 10, 8), 1200, True, np.float64),
    (6, 900, 700, False, np.complex64),
]


@pytest.mark.parametrize("nparts,ngids,m,with_ghost,dtype", CASES)
def test_coo_exchange_bitexact(be, pamd, O, nparts, ngids, m, with_ghost, dtype):
    args = problem(pamd, O, be, nparts, ngids, m, dtype, SEED, with_ghost=with_ghost)
    moved, zeroed, multi = _check(pamd, O, *args)
    assert moved > 0, "no triplet moved"
    assert zeroed > 0, "no ghost-row value zeroed"
    assert multi > 0, "no sent triplet whose lid sits in two or more send segments"


def test_coo_exchange_nan_inf_and_empty_part(be, pamd, O):
    """a sent NaN/Inf keeps its bits on both sides, an unsent ghost-row NaN
    becomes +0 (zero(Tv), Interfaces.jl:2530: not v*0), and a part without
    triplets still receives."""
    parts, oparts, rows, orows, I, J, V, mk = problem(pamd, O, be, 4, 2000, 1500, np.float64, SEED + 1)
    # part 3 keeps the ghost rows add_gids!(rows, I) gave it and loses its
    # triplets: it sends nothing and receives its ghost rows' triplets
    I[3], J[3], V[3] = I[3][:0], J[3][:0], V[3][:0]
    cls = classify(orows, parts.part_ids, I)
    nan = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]  # a NaN with a payload
    sent_at, zero_at = {}, {}
    for p in parts.part_ids:
        kind, _ = cls[p]
        if len(kind) == 0:
            continue
        s, z = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
        assert len(s) >= 3 and len(z) >= 2
        V[p][s[0]], V[p][s[1]], V[p][s[2]] = nan, np.inf, -np.nan
        V[p][z[0]], V[p][z[1]] = nan, -np.inf
        sent_at[p], zero_at[p] = s[:3], z[:2]
    coo = pamd.COO.from_host(mk(I), mk(J), mk(V), rows)
    pamd.exchange_(coo, rows)
    gI, gJ, gV = coo.to_host()
    rI, rJ, rV = exchange_coo_(O, *oracle_lists(O, parts.part_ids, oparts, I, J, V), orows)
    nan_arrived = 0
    for p in parts.part_ids:
        n = len(I[p])
        got = gV.local(p)
        assert gI.local(p).tolist() == list(rI[p]) and gJ.local(p).tolist() == list(rJ[p])
        assert got.tobytes() == rV[p].tobytes(), f"part {p}: V differs"
        if n:
            assert got[sent_at[p]].tobytes() == V[p][sent_at[p]].tobytes()        # the sender's side
            assert got[zero_at[p]].tobytes() == np.zeros(2).tobytes()             # +0, sign bit clear
        nan_arrived += int((got[n:].view(np.uint64) == np.uint64(0x7FF8000000000123)).sum())
    assert nan_arrived == 3  # one per sending part, bits kept on the receiver's side
    assert len(I[3]) == 0 and len(gI.local(3)) > 0


def test_coo_assemble_exchange_then_sparse_equals_oracle(be, pamd, O):
    """the chain a user runs: assemble!(I, J, V, rows), exchange!(I, J, V,
    rows), PSparseMatrix(I, J, V, rows, cols; ids=:global), mul! — against
    the oracle's assemble_coo_, the restatement, psparse_from_coo and mul!"""
    N = (30, 28)
    parts, oparts, rows, orows, I, J, V, mk = problem(pamd, O, be, (2, 2), N, 1500, np.float64, SEED + 2,
                                                      with_ghost=True)
    coo = pamd.COO.from_host(mk(I), mk(J), mk(V), rows)
    pamd.assemble_(coo, rows)
    pamd.exchange_(coo, rows)
    gI, gJ, gV = coo.to_host()
    rI, rJ, rV = O.assemble_coo_(*oracle_lists(O, parts.part_ids, oparts, I, J, V), orows)
    n_assembled = {p: len(rI[p]) for p in parts.part_ids}
    rI, rJ, rV = exchange_coo_(O, rI, rJ, rV, orows)
    for p in parts.part_ids:
        assert gI.local(p).tolist() == list(rI[p]), f"part {p}: I differs"
        assert gJ.local(p).tolist() == list(rJ[p]), f"part {p}: J differs"
        assert gV.local(p).tobytes() == rV[p].tobytes(), f"part {p}: V differs"
    assert sum(len(rI[p]) - n_assembled[p] for p in parts.part_ids) > 0
    cols = pamd.prange_cartesian(parts, N)
    ocols = O.prange_cartesian(oparts, N)
    pamd.add_gids_(cols, coo.global_cols())
    A = pamd.PSparseMatrix.from_coo(coo, None, None, rows, cols, ids="global")
    O.add_gids_(ocols, rJ)
    OA = O.psparse_from_coo(rI, rJ, rV, orows, ocols, ids="global")
    rng = np.random.default_rng(SEED + 3)
    xs = {p: rng.uniform(-1, 1, cols.partition.local(p).num_lids) for p in parts.part_ids}
    x = pamd.PVector.from_host(pamd.map_parts(lambda s: xs[s.part], cols.partition), cols)
    y = pamd.PVector.undef(rows)
    pamd.mul_(y, A, x)
    ox = O.PVector(O.map_parts(lambda s: xs[s.part].copy(), OA.cols.partition), OA.cols)
    oy = O.pvector_undef(OA.rows)
    O.mul_(oy, OA, ox)
    got = y.to_host()
    for p in parts.part_ids:
        own = rows.partition.local(p).oid_to_lid - 1
        assert len(own) > 0
        assert np.array_equal(got.local(p)[own], oy.values[p][own]), f"part {p}: mul! differs"


def test_coo_exchange_unknown_row_gid(be, pamd):
    parts = be.get_part_ids(2)
    rows = pamd.prange_linear(parts, 10)
    I = pamd.PData(parts.backend, parts.part_ids, [np.array([1, 2, 7]), np.array([6, 7])], parts.shape)
    pamd.add_gids_(rows, I)
    bad = pamd.PData(parts.backend, parts.part_ids, [np.array([1, 2, 9]), np.array([6, 7])], parts.shape)
    J = pamd.PData(parts.backend, parts.part_ids, [np.array([1, 1, 1]), np.array([1, 1])], parts.shape)
    V = pamd.PData(parts.backend, parts.part_ids, [np.ones(3), np.ones(2)], parts.shape)
    coo = pamd.COO.from_host(bad, J, V, rows)
    with pytest.raises(pamd.PAError, match="KeyError"):
        pamd.exchange_(coo, rows)


def test_coo_exchange_exchanger_mismatch(be, pamd, O):
    """part 2 sends to part 1, whose parts_rcv does not list it: the
    reference's delivery has no slot for that segment
    (SequentialBackend.jl:154-165), an error and not a segment dropped"""
    parts, oparts, rows, orows, I, J, V, mk = problem(pamd, O, be, 4, 2000, 1500, np.float64, SEED + 7)
    coo = pamd.COO.from_host(mk(I), mk(J), mk(V), rows)
    ctxs = pamd.device.contexts(rows.partition)
    idx = [pamd.device.device_index_gids(c, rows.partition.local(p)) for c, p in zip(ctxs, parts.part_ids)]
    xg = [pamd.device.device_exchanger(c, rows.exchanger, p) for c, p in zip(ctxs, parts.part_ids)]
    ex = rows.exchanger
    assert 1 in list(ex.parts_snd.local(2))
    empty = pamd.Table(np.zeros(0, np.int32), np.ones(1, np.int32))
    xg[0] = pamd.device.DeviceExchanger(ctxs[0], [], empty, ex.parts_snd.local(1), ex.lids_snd.local(1))
    with pytest.raises(pamd.PAError, match="exchanger mismatch"):
        pamd._lib.call("pa_coo_exchange_all", len(ctxs), pamd._lib.ptr_array([c.h for c in coo.values.parts]),
                       pamd._lib.ptr_array([d.h for d in idx]), pamd._lib.ptr_array([d.h for d in xg]))


def test_coo_exchange_needs_rows(be, pamd):
    parts = be.get_part_ids(2)
    rows = pamd.prange_linear(parts, 10)
    mk = lambda a, b: pamd.PData(parts.backend, parts.part_ids, [np.array(a), np.array(b)], parts.shape)
    coo = pamd.COO.from_host(mk([1, 2], [6]), mk([1, 1], [1]), mk([1.0, 2.0], [3.0]), rows)
    with pytest.raises(TypeError):
        pamd.exchange_(coo)


@pytest.mark.parametrize("nparts,ngids,m,with_ghost", [(4, 2000, 1500, False), ((2, 2, 2), (12, 10, 8), 1200, True)])
def test_rccl_coo_exchange_bitexact(be_rccl, pamd, O, nparts, ngids, m, with_ghost):
    """every count and every (I, J, V) segment through the grouped RCCL
    send/recv (to self on one GPU: pa_coo_exchange_all's cross-process path),
    bit-exact; the halo counters count mul!/exchange!(v) segments only"""
    args = problem(pamd, O, be_rccl, nparts, ngids, m, np.float64, SEED + 7, with_ghost=with_ghost)
    parts = args[0]
    s0 = {p: parts.backend.context(p).comm_stats() for p in parts.part_ids}
    moved, zeroed, multi = _check(pamd, O, *args)
    assert moved > 0 and zeroed > 0 and multi > 0
    assert {p: parts.backend.context(p).comm_stats() for p in parts.part_ids} == s0
