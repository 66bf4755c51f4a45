"""exchange!(combine_op, values::AbstractPData{<:Table}, exchanger) restated
in numpy (Interfaces.jl:899-961): the independent reference of the device
table exchange tests.  It imports exchange_ref and nothing else of the
project.

A table is a `(data, ptrs)` pair (or anything with `.data` and `.ptrs`); ptrs
are 1-based, row lid holds data[ptrs[lid-1]-1 : ptrs[lid]-1].  The table
exchanger replaces every lid of lids_rcv / lids_snd by the 1-based data
positions of its row (_table_lids_snd, 928-961), segment by segment, and the
vector exchange of exchange_ref runs over the data with those lists.

The module also draws row lengths for a set of exchanger tables.  Slot for
slot the sender's row and the receiver's row must be equally long, so a
length belongs to an equivalence class of (part, lid) pairs under "shares a
slot pair": `classes` finds them, `row_lengths` draws one length per class."""
import numpy as np

import exchange_ref as R

LENGTHS = (0, 1, 2, 3, 65, 300)  # empty rows, a row longer than a wave, a row longer than a block


def _pair(t):
    data, ptrs = (t.data, t.ptrs) if hasattr(t, "ptrs") else t
    return np.asarray(data, dtype=np.int64), np.asarray(ptrs, dtype=np.int64)


def expand(lids, tptrs):
    """_table_lids_snd for one part: the (data, ptrs) pair of 1-based data
    positions that the rows named by `lids` hold, in slot order"""
    data, ptrs = _pair(lids)
    tptrs = np.asarray(tptrs, dtype=np.int64)
    first = tptrs[data - 1]
    count = tptrs[data] - first
    start = np.concatenate([[0], np.cumsum(count)])  # expanded offset of every slot
    within = np.arange(start[-1]) - np.repeat(start[:-1], count)
    out = np.repeat(first, count) + within
    return out, start[ptrs - 1] + 1


def table_exchanger(tptrs, lids_rcv, lids_snd):
    """_table_exchanger: both lists of every part expanded by its table's ptrs"""
    return ([expand(l, t) for l, t in zip(lids_rcv, tptrs)], [expand(l, t) for l, t in zip(lids_snd, tptrs)])


def exchange(data, tptrs, parts_rcv, lids_rcv, parts_snd, lids_snd, op, reverse=False, order="ascending"):
    """the table exchange in place on the list of per-part data arrays"""
    xr, xs = table_exchanger(tptrs, lids_rcv, lids_snd)
    return R.exchange(data, parts_rcv, xr, parts_snd, xs, op, reverse, order)


def zero(data, tptrs, lids):
    """the data of the rows named by every part's `lids` table become +0.0"""
    return R.zero(data, [expand(l, t)[0] for l, t in zip(lids, tptrs)])


def multiplicity(tptrs, lids):
    """per part: how many expanded slots name each data entry"""
    return [R.multiplicity(expand(l, t)[0], int(np.asarray(t)[-1]) - 1) for l, t in zip(lids, tptrs)]


# ---------------------------------------------------------------------------
# row lengths

def _slot_pairs(parts_rcv, lids_rcv, parts_snd, lids_snd):
    """((sender part, lid), (receiver part, lid)) of every slot pair; parts
    and lids 1-based"""
    rcv = [_pair(t) for t in lids_rcv]
    snd = [_pair(t) for t in lids_snd]
    for q in range(len(rcv)):
        for k, p in enumerate(parts_rcv[q]):
            p = int(p)
            m = [int(x) for x in parts_snd[p - 1]].index(q + 1)
            a = rcv[q][0][rcv[q][1][k] - 1:rcv[q][1][k + 1] - 1]
            b = snd[p - 1][0][snd[p - 1][1][m] - 1:snd[p - 1][1][m + 1] - 1]
            assert len(a) == len(b), f"segment {p}→{q + 1} has different lengths on its two sides"
            for la, lb in zip(a, b):
                yield (p, int(lb)), (q + 1, int(la))


def classes(sizes, parts_rcv, lids_rcv, parts_snd, lids_snd):
    """Per part an int array over its lids: the class of (part, lid) under
    "shares a slot pair" (numbered from 0 in order of first appearance), -1
    for a lid that no list names."""
    base = np.concatenate([[0], np.cumsum(sizes)])
    parent = np.arange(base[-1])

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    named = np.zeros(base[-1], bool)
    for (p, lp), (q, lq) in _slot_pairs(parts_rcv, lids_rcv, parts_snd, lids_snd):
        a, b = base[p - 1] + lp - 1, base[q - 1] + lq - 1
        named[a] = named[b] = True
        parent[find(a)] = find(b)
    ids, out = {}, np.full(base[-1], -1)
    for x in np.flatnonzero(named):
        out[x] = ids.setdefault(find(x), len(ids))
    return [out[base[p]:base[p + 1]] for p in range(len(sizes))]


def row_lengths(sizes, tables, rng, lengths=LENGTHS):
    """Per part the 1-based Int32 ptrs of a table whose travelling rows have
    one length per class: every value of `lengths` is given to one class
    first (the classes in random order), the others draw with the short
    lengths three times as likely as the long ones; rows that do not travel
    draw the same way."""
    cls = classes(sizes, *tables)
    ncls = 1 + max([int(c.max()) for c in cls if len(c)], default=-1)
    assert ncls >= len(lengths), "fewer classes than lengths to place"
    lengths = np.asarray(lengths)
    w = np.where(lengths <= 3, 3.0, 1.0)
    per_class = rng.choice(lengths, ncls, p=w / w.sum())
    per_class[rng.permutation(ncls)[:len(lengths)]] = lengths
    ptrs = []
    for c in cls:
        n = np.where(c >= 0, per_class[np.maximum(c, 0)], rng.choice(lengths, len(c), p=w / w.sum()))
        ptrs.append(np.concatenate([[1], 1 + np.cumsum(n)]).astype(np.int32))
    return ptrs


def check_lengths(sizes, tables, tptrs, lengths=LENGTHS):
    """the class and length conditions of a set of row pointers: equal
    lengths on both sides of every slot pair, and every value of `lengths`
    among the travelling rows; returns (travelling lids, classes, largest class)"""
    n = [np.diff(np.asarray(t, dtype=np.int64)) for t in tptrs]
    seen = set()
    for (p, lp), (q, lq) in _slot_pairs(*tables):
        assert n[p - 1][lp - 1] == n[q - 1][lq - 1], f"({p}, {lp}) and ({q}, {lq}) share a slot pair, lengths differ"
        seen.update((int(n[p - 1][lp - 1]),))
    assert seen >= set(int(x) for x in lengths), f"lengths among the travelling rows: {sorted(seen)}"
    cls = np.concatenate(classes(sizes, *tables))
    cls = cls[cls >= 0]
    return len(cls), len(np.unique(cls)), int(np.bincount(cls).max())
