"""The partitions, exchangers and values of tests/test_gpu_exchange.py, built
with numpy alone (seeded) so that the reference side needs no device: what a
case hands to the device is exactly what it hands to exchange_ref.

A case holds, per part (position part - 1): the index set (lid_to_gid,
lid_to_part, hids = 1-based ghost lids) and the four exchanger tables as
(data, ptrs) pairs of 1-based int32 arrays."""
import numpy as np

import exchange_ref as R

SEED = 20250114
DTYPES = [np.float32, np.float64, np.complex64, np.complex128]
# (op, reverse, zero_ghosts): exchange_ is (REPLACE, 0, 0), assemble_ (ADD, 1, 1)
MODES = [(op, rev, z) for op in (R.REPLACE, R.ADD) for rev in (0, 1) for z in (0, 1)]
MODE_IDS = [f"{op}-{'rev' if rev else 'fwd'}-{'zero' if z else 'keep'}" for op, rev, z in MODES]
SENTINEL = 12345.625  # exact in every element type


class Case:
    def __init__(self, name, sizes, lid_to_gid, lid_to_part, tables=None):
        self.name = name
        self.sizes = list(sizes)
        self.nparts = len(sizes)
        self.lid_to_gid = lid_to_gid
        self.lid_to_part = lid_to_part
        self.hids = [np.flatnonzero(o != p + 1) + 1 for p, o in enumerate(lid_to_part)]
        self.ngids = int(sum(np.count_nonzero(o == p + 1) for p, o in enumerate(lid_to_part)))
        if tables is not None:
            self.set_tables(*tables)

    def set_tables(self, parts_rcv, lids_rcv, parts_snd, lids_snd):
        self.parts_rcv, self.lids_rcv, self.parts_snd, self.lids_snd = parts_rcv, lids_rcv, parts_snd, lids_snd
        for n, tabs in zip(self.sizes, zip(lids_rcv, lids_snd)):  # nothing the device gets may leave the vectors
            for data, ptrs in tabs:
                assert ptrs[0] == 1 and ptrs[-1] == len(data) + 1 and np.all(np.diff(ptrs) >= 0)
                assert len(data) == 0 or (data.min() >= 1 and data.max() <= n)

    @property
    def tables(self):
        return self.parts_rcv, self.lids_rcv, self.parts_snd, self.lids_snd

    def into(self, reverse):
        """the lists a transfer lands on"""
        return self.lids_snd if reverse else self.lids_rcv

    def frm(self, reverse):
        return self.lids_rcv if reverse else self.lids_snd


def make_partition(sizes, nown, rng):
    """Index sets whose ghosts are scattered among the owned lids: part p owns
    nown[p] consecutive gids; its other lids are ghosts, distinct gids drawn
    from the ones the other parts own, each with its owner in lid_to_part."""
    first = np.concatenate([[1], 1 + np.cumsum(nown)])
    owner_of = np.repeat(np.arange(1, len(sizes) + 1), nown)  # gid - 1 → part
    l2g, l2p = [], []
    for p, (n, no) in enumerate(zip(sizes, nown)):
        others = np.flatnonzero(owner_of != p + 1) + 1
        assert n - no <= len(others), "more ghosts asked for than the other parts own gids"
        ghosts = rng.choice(others, n - no, replace=False)
        is_ghost = np.zeros(n, bool)
        is_ghost[rng.choice(n, n - no, replace=False)] = True
        g = np.empty(n, np.int64)
        g[~is_ghost] = np.arange(first[p], first[p] + no)
        g[is_ghost] = ghosts
        l2g.append(g)
        l2p.append(owner_of[g - 1].astype(np.int32) if n else np.zeros(0, np.int32))
    return l2g, l2p


def _table(segs):
    ptrs = np.concatenate([[1], 1 + np.cumsum([len(s) for s in segs])]).astype(np.int32)
    data = np.concatenate(segs).astype(np.int32) if segs else np.zeros(0, np.int32)
    return data, ptrs


def make_tables(sizes, edges, rng, unique_rcv, forwarded=0, owned=None):
    """Exchanger tables over the edges [(sender, receiver, slots)] (neighbour
    lists ascending).  Send lids: drawn with replacement from all lids of the
    sender.  Receive lids: from a random half of the receiver's lids, with
    replacement (duplicates inside a segment and across segments), or
    unique_rcv: without, over all segments of the part.  forwarded: that many
    slots of every non-empty send segment name lids of the sender's own
    receive list instead, an owned one first when there is one."""
    np_ = len(sizes)
    rcv_segs = [dict() for _ in range(np_)]
    for q in range(np_):
        mine = [(s, n) for s, d, n in edges if d == q + 1]
        half = rng.choice(sizes[q], sizes[q] // 2, replace=False) + 1 if sizes[q] else np.zeros(0, np.int64)
        total = sum(n for _, n in mine)
        pool = rng.permutation(half)[:total] if unique_rcv else None
        assert not unique_rcv or total <= len(half), "unique receive lids do not fit into half the lids"
        at = 0
        for s, n in sorted(mine):
            rcv_segs[q][s] = pool[at:at + n] if unique_rcv else rng.choice(half, n, replace=True) if n else half[:0]
            at += n
    snd_segs = [dict() for _ in range(np_)]
    for p in range(np_):
        got = np.concatenate(list(rcv_segs[p].values())) if rcv_segs[p] else np.zeros(0, np.int64)
        for s, d, n in sorted(edges):
            if s != p + 1:
                continue
            lids = rng.integers(1, sizes[p] + 1, n) if n else np.zeros(0, np.int64)
            k = min(forwarded, n, len(got))
            if k:
                pick = rng.choice(got, k, replace=False)
                own = [l for l in got if owned[p][l - 1]]
                if own and not any(owned[p][l - 1] for l in pick):
                    pick[0] = own[0]
                lids[rng.choice(n, k, replace=False)] = pick
            snd_segs[p][d] = lids
    parts_rcv = [np.array(sorted(d), np.int32) for d in rcv_segs]
    parts_snd = [np.array(sorted(d), np.int32) for d in snd_segs]
    lids_rcv = [_table([d[k] for k in sorted(d)]) for d in rcv_segs]
    lids_snd = [_table([d[k] for k in sorted(d)]) for d in snd_segs]
    return parts_rcv, lids_rcv, parts_snd, lids_snd


# the main partition: 41, 300 and 17 lids.  Parts 1 and 3 hold a third of
# their lids as ghosts; part 2 holds every gid the other two own (38: there
# are no more distinct gids to ghost), scattered among its 262 owned lids.
SIZES, NOWN = (41, 300, 17), (27, 262, 11)
DUP_EDGES = [(1, 2, 70), (2, 1, 50), (2, 3, 40), (1, 3, 9), (3, 2, 0)]
# unique receive lids have to fit into the receiver: 50 slots do not fit into
# part 1's 41 lids nor 49 into part 3's 17, so the same edges carry fewer slots
FORWARD_EDGES = [(1, 2, 70), (2, 1, 18), (2, 3, 5), (1, 3, 3), (3, 2, 0)]
LONELY_SIZES, LONELY_NOWN = (41, 300, 0), (27, 273, 0)
LONELY_EDGES = [(1, 2, 70), (2, 1, 50)]
WIDE_SLOTS = 1_048_576 + 300  # one more grid-stride round than 4096 blocks of 256 cover
WIDE_TARGETS = 1_048_576 + 4096


def small_cases():
    rng = np.random.default_rng(SEED)
    l2g, l2p = make_partition(SIZES, NOWN, rng)
    owned = [o == p + 1 for p, o in enumerate(l2p)]
    cases = {"ghost": Case("ghost", SIZES, l2g, l2p)}  # tables: exchanger_from_ids, set by the device test
    cases["dup"] = Case("dup", SIZES, l2g, l2p, make_tables(SIZES, DUP_EDGES, rng, False))
    cases["forward"] = Case("forward", SIZES, l2g, l2p,
                            make_tables(SIZES, FORWARD_EDGES, rng, True, forwarded=5, owned=owned))
    g, p = make_partition(LONELY_SIZES, LONELY_NOWN, rng)
    t = make_tables(LONELY_SIZES, LONELY_EDGES, rng, False)
    cases["lonely"] = Case("lonely", LONELY_SIZES, g, p, t)
    return cases


def wide_case(dups):
    """Two parts, one edge 1→2.  dups False: WIDE_SLOTS slots, both lists
    without repeats (the unique kernels, forward and reverse).  dups True:
    about 1.2 M slots onto WIDE_TARGETS distinct lids on both sides (the
    ordered kernels, more targets than one grid-stride round covers)."""
    rng = np.random.default_rng(SEED + (2 if dups else 1))
    n = WIDE_TARGETS + 1000
    sizes = (n, n)
    l2g = [np.arange(1, n + 1, dtype=np.int64), np.arange(n + 1, 2 * n + 1, dtype=np.int64)]
    l2p = [np.full(n, 1, np.int32), np.full(n, 2, np.int32)]

    def lids():
        if not dups:
            return rng.permutation(n)[:WIDE_SLOTS] + 1
        base = rng.permutation(n)[:WIDE_TARGETS] + 1
        return rng.permutation(np.concatenate([base, rng.choice(base, 150_000, replace=True)]))
    snd, rcv = lids(), lids()
    e = _table([])
    tables = ([np.zeros(0, np.int32), np.array([1], np.int32)], [e, _table([rcv])],
              [np.array([2], np.int32), np.zeros(0, np.int32)], [_table([snd]), e])
    return Case("wide_dup" if dups else "wide", sizes, l2g, l2p, tables)


# ---------------------------------------------------------------------------
# values

def family(rng, n, dtype):
    """±u·2^k, u in [1, 2), k in -8..8: sums of them round, so the order of a
    fold shows in the bits"""
    def one():
        return rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * 2.0 ** rng.integers(-8, 9, n)
    dtype = np.dtype(dtype)
    return (one() + 1j * one()).astype(dtype) if dtype.kind == "c" else one().astype(dtype)


def _specials(dtype):
    """a quiet NaN with a payload, ±Inf and -0.0 in the element type"""
    dtype = np.dtype(dtype)
    real = np.float32 if dtype.itemsize // (2 if dtype.kind == "c" else 1) == 4 else np.float64
    nan = (np.array([0x7FC00123], np.uint32).view(np.float32) if real == np.float32
           else np.array([0x7FF8000000000123], np.uint64).view(np.float64))[0]
    s = np.array([nan, np.inf, -np.inf, -0.0], dtype=real)
    if dtype.kind != "c":
        return s
    c = np.empty(4, dtype)
    c.real, c.imag = s, s[::-1]
    return c


def start_values(case, dtype, mode):
    """The vectors before the call.  Lids that no list names hold SENTINEL.
    REPLACE: NaN, ±Inf and -0.0 sit in up to four lids that are sent.
    zero_ghosts: up to four ghost lids hold NaN (REPLACE runs, or ghosts that
    an ADD run does not send: no NaN enters an add that is compared) or -1."""
    op, reverse, zero = mode
    rng = np.random.default_rng([SEED, sum(map(ord, case.name)), np.dtype(dtype).num, MODES.index(mode)])
    vals = []
    sp = _specials(dtype)
    for p, n in enumerate(case.sizes):
        v = family(rng, n, dtype)
        named = np.zeros(n, bool)
        for t in (case.lids_rcv[p], case.lids_snd[p]):
            named[t[0] - 1] = True
        v[~named] = SENTINEL
        sent = np.unique(case.frm(reverse)[p][0])
        if op == R.REPLACE and len(sent):
            pick = rng.choice(sent, min(4, len(sent)), replace=False)
            v[pick - 1] = sp[:len(pick)]
        if zero and len(case.hids[p]):
            pick = rng.choice(case.hids[p], min(4, len(case.hids[p])), replace=False)
            for i, l in enumerate(pick):
                v[l - 1] = sp[0] if (op == R.REPLACE or l not in sent) and i % 2 == 0 else -1.0
        vals.append(v)
    return vals


def expected(case, start, mode, order="ascending", zero=True):
    op, reverse, z = mode
    v = [a.copy() for a in start]
    R.exchange(v, *case.tables, op, bool(reverse), order)
    if z and zero:
        R.zero(v, case.hids)
    return v


def fold_order_stats(case, dtype, modes):
    """Over the runs `modes` of a case: the targets with two or more
    contributions; among those of the ADD runs, how many change their bits
    when folded in descending slot order."""
    multi = multi_add = changed = 0
    for mode in modes:
        op, reverse, _ = mode
        several = [R.multiplicity(t[0], n) >= 2 for t, n in zip(case.into(reverse), case.sizes)]
        multi += int(sum(s.sum() for s in several))
        if op != R.ADD:
            continue
        start = start_values(case, dtype, mode)
        up = expected(case, start, mode, zero=False)
        down = expected(case, start, mode, "descending", zero=False)
        for s, a, b in zip(several, up, down):
            w = a.dtype.itemsize
            differ = (a.view(np.uint8).reshape(-1, w) != b.view(np.uint8).reshape(-1, w)).any(axis=1)
            multi_add += int(s.sum())
            changed += int(differ[s].sum())
            assert not differ[~s].any()  # one contribution: no order
    return multi, multi_add, changed
