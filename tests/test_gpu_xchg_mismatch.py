"""Exchangers that do not match each other, through the vector transport
(pa_exchange_all) and mul! (pa_spmv_all): the receiver's lookup of its
segment in the sender's opposite list fails on the host, before the transport
is issued, with the reference's two complaints (SequentialBackend.jl:154-165,
187), and the contexts and vectors stay usable.

Two parts on one device over a Cartesian range of 12 gids with its ghost
layer: 6 owned ids and one ghost each, one segment in each direction — the
smallest case in which both lists of both parts are non-empty.  The
exchangers are built by hand (pamd.device.DeviceExchanger); `reverse` swaps
the roles of the two lists, so the same check fires in the other direction;
halo_pull 1 reaches the check of the pull table's build, halo_pull 0 the one
of the staging copies."""
import re

import numpy as np
import pytest

from matrix_cases import with_ghost_coo

pytestmark = pytest.mark.gpu

SEED = 20250114
NGIDS = (12,)
NO_SENDER = "exchanger mismatch: a receiver lists a sender that does not send to it"
LENGTHS = "segment lengths differ"


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


@pytest.fixture(scope="module")
def setup(be, pamd, O):
    parts = be.get_part_ids((2,))
    rows = pamd.prange_cartesian(parts, NGIDS, with_ghost=True)
    oparts = O.get_part_ids((2,))
    orows = O.prange_cartesian(oparts, NGIDS, with_ghost=True)
    ex = rows.exchanger
    for p in (1, 2):
        s = rows.partition.local(p)
        assert s.num_oids == 6 and 1 <= s.num_hids <= 2
        assert list(ex.parts_rcv.local(p)) == [3 - p] and list(ex.parts_snd.local(p)) == [3 - p]
    rng = np.random.default_rng(SEED)
    xs = {}
    for p in (1, 2):
        s = rows.partition.local(p)
        xs[p] = rng.uniform(-1, 1, s.num_lids)
        xs[p][s.hid_to_lid - 1] = -7.0
    ox = O.PVector(O.map_parts(lambda s: xs[s.part].copy(), orows.partition), orows)
    O.exchange_pvector_(ox)
    ctxs = pamd.device.contexts(rows.partition)
    good = [pamd.device.device_exchanger(c, ex, p) for c, p in zip(ctxs, (1, 2))]
    v = pamd.PVector.undef(rows)
    return dict(parts=parts, oparts=oparts, rows=rows, orows=orows, ctxs=ctxs, good=good, v=v, xs=xs, ref=ox.values)


def _lists(pamd, rows, reverse):
    """per part: (the list a transfer lands on, the list it leaves from), each
    (parts, lids table); forward: (rcv, snd), reverse: (snd, rcv)"""
    ex = rows.exchanger
    out = {}
    for p in (1, 2):
        rcv = (ex.parts_rcv.local(p), ex.lids_rcv.local(p))
        snd = (ex.parts_snd.local(p), ex.lids_snd.local(p))
        out[p] = (snd, rcv) if reverse else (rcv, snd)
    return out


def _empty(pamd):
    return ([], pamd.Table(np.zeros(0, np.int32), np.ones(1, np.int32)))


def _xchg(pamd, ctx, into, frm, reverse):
    rcv, snd = (frm, into) if reverse else (into, frm)
    return pamd.device.DeviceExchanger(ctx, rcv[0], rcv[1], snd[0], snd[1])


def _mismatched(pamd, case, rows, ctxs, reverse):
    """the two parts' exchangers of a case, and the names of the lists a
    transfer leaves from and lands on"""
    L = _lists(pamd, rows, reverse)
    (into1, from1), (into2, from2) = L[1], L[2]
    if case == "no_sender":  # part 1 receives from part 2, which sends to nobody
        from2 = _empty(pamd)
    elif case == "lengths":  # part 1 expects 2 slots from part 2, which sends 1
        assert len(from2[1].data) == 1
        into1 = ([2], pamd.Table(np.array([6, 7], np.int32), np.array([1, 3], np.int32)))
    elif case == "list_back":  # part 1 sends to part 2, which receives from nobody
        into2 = _empty(pamd)
    return [_xchg(pamd, ctxs[0], into1, from1, reverse), _xchg(pamd, ctxs[1], into2, from2, reverse)]


def _exchange(pamd, v, xg, op, reverse):
    hs = pamd._lib.ptr_array
    pamd._lib.call("pa_exchange_all", 2, hs([d.h for d in v.values.parts]), hs([d.h for d in xg]),
                   hs([None, None]), op, reverse, 0)


def _good_exchange_matches(pamd, S):
    """a correct exchange on the same contexts and vectors: the oracle's values"""
    v = S["v"]
    for p, dv in zip((1, 2), v.values.parts):
        dv.upload(S["xs"][p])
    _exchange(pamd, v, S["good"], pamd._lib.PA_REPLACE, 0)
    got = v.to_host()
    for p in (1, 2):
        assert got.local(p).tobytes() == np.asarray(S["ref"][p]).tobytes(), f"part {p}: exchanged values differ"


def _message(case, reverse):
    if case == "no_sender":
        return NO_SENDER
    if case == "lengths":
        return LENGTHS
    to, frm = ("parts_rcv", "parts_snd") if reverse else ("parts_snd", "parts_rcv")
    return f"exchanger mismatch (a part in {to} does not list this part in {frm})"


@pytest.mark.parametrize("halo_pull", [1, 0])
@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("case", ["no_sender", "lengths", "list_back"])
def test_exchange_mismatch_is_an_error(pamd, setup, case, reverse, halo_pull):
    """no_sender, lengths: the receiver's lookup.  list_back: a sending
    segment whose receiver does not list the sender back would be dropped
    silently (the COO exchange's check, in its wording)."""
    S = setup
    prev = pamd._lib.tune("halo_pull", halo_pull)
    try:
        xg = _mismatched(pamd, case, S["rows"], S["ctxs"], reverse)
        for dv, p in zip(S["v"].values.parts, (1, 2)):
            dv.upload(S["xs"][p])
        op = pamd._lib.PA_ADD if reverse else pamd._lib.PA_REPLACE
        with pytest.raises(pamd.PAError, match=re.escape(_message(case, reverse))):
            _exchange(pamd, S["v"], xg, op, reverse)
        _good_exchange_matches(pamd, S)
    finally:
        pamd._lib.tune("halo_pull", prev)


@pytest.mark.parametrize("case", ["no_sender", "lengths"])
def test_mul_mismatch_is_an_error(pamd, O, setup, case):
    """mul! of a two-part matrix (7 lids per part: parts of one device share
    a stream pair, so the call asks for the grouped direct pull) with
    mismatched exchangers of x.  build_direct's copy of the check is reached
    first, but group_ok takes any failure of it as "not this path" and turns
    the set away; the per-part path's transport plan then meets the same
    mismatch in build_pull and raises: the message pinned is that one's (the
    two are word for word the same)."""
    S = setup
    parts, rows, orows = S["parts"], S["rows"], S["orows"]
    rng = np.random.default_rng(SEED + 1)
    I, J, V = with_ghost_coo(rows, parts, NGIDS, None, rng)
    mk = lambda d: pamd.PData(parts.backend, parts.part_ids, [d[p] for p in parts.part_ids], parts.shape)
    A = pamd.PSparseMatrix.from_coo(mk(I), mk(J), mk(V), rows, rows, ids="global")
    omk = lambda d, f: O.PData([f(d[p]) for p in parts.part_ids], S["oparts"].shape)
    OA = O.psparse_from_coo(omk(I, lambda a: [int(v) for v in a]), omk(J, lambda a: [int(v) for v in a]),
                            omk(V, lambda a: a.copy()), orows, orows, ids="global")
    x = pamd.PVector.from_host(pamd.map_parts(lambda s: S["xs"][s.part], rows.partition), rows)
    y = pamd.PVector.undef(rows)
    xg = _mismatched(pamd, case, rows, S["ctxs"], 0)
    args = list(pamd.pvector._spmv_args_build(y, A, x, 1.0, 0.0))
    args[6] = pamd._lib.ptr_array([d.h for d in xg])
    with pytest.raises(pamd.PAError, match=re.escape(_message(case, 0))):
        pamd._lib.call("pa_spmv_all", *args)
    pamd.mul_(y, A, x)
    ox = O.PVector(O.map_parts(lambda s: S["xs"][s.part].copy(), orows.partition), orows)
    oy = O.pvector_undef(orows)
    O.mul_(oy, OA, ox)
    got = y.to_host()
    for p in parts.part_ids:
        own = rows.partition.local(p).oid_to_lid - 1
        assert got.local(p)[own].tobytes() == np.asarray(oy.values[p])[own].tobytes(), f"part {p}: SpMV differs"
