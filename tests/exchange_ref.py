"""exchange!(combine_op, values, exchanger) restated in numpy (Interfaces.jl:
846-889 with the delivery of SequentialBackend.jl:154-200): the independent
reference of the device exchange tests.  It imports nothing from the package
or from the oracle.

Conventions: parts are numbered from 1 and sit at list position part - 1;
lids and table pointers are 1-based, as in the reference.  A table is
anything with `.data` and `.ptrs`, or a `(data, ptrs)` pair.

    exchange(values, parts_rcv, lids_rcv, parts_snd, lids_snd, op, reverse)

1. every part packs its send segments (data_snd.data[p] = values[lids_snd.
   data[p]]), all of them before anything is unpacked, so a lid that is both
   sent and received travels with its old value;
2. segment p→q is delivered to q's slot for p (missing partner or unequal
   lengths: ValueError, the reference's @check);
3. every part folds values[lid] = op(values[lid], data_rcv.data[p]) for p
   ascending over its receive buffer.

The arithmetic is numpy's in the element type of `values`: one rounding per
add (complex: per component), no wider accumulator.  Targets named several
times are folded in rounds: round r applies every target's r-th contribution
in buffer order, each target at most once per round, so a round is one
vectorised gather/op/scatter and the order inside a target is the buffer's.
`order="descending"` folds in the opposite order; the device tests use it only
to show that their values make the order visible."""
import numpy as np

REPLACE = "replace"
ADD = "add"


def _table(t):
    data, ptrs = (t.data, t.ptrs) if hasattr(t, "ptrs") else t
    return np.asarray(data, dtype=np.int64), np.asarray(ptrs, dtype=np.int64)


def _segment(ptrs, k):
    return slice(int(ptrs[k]) - 1, int(ptrs[k + 1]) - 1)


def deliver(values, parts_rcv, lids_rcv, parts_snd, lids_snd):
    """steps 1 and 2: per part, its receive buffer (a copy, in the element
    type) laid out by lids_rcv.ptrs"""
    n = len(values)
    if not (len(parts_rcv) == len(parts_snd) == len(lids_rcv) == len(lids_snd) == n):
        raise ValueError("exchange: the lists cover different numbers of parts")
    snd = [_table(t) for t in lids_snd]
    rcv = [_table(t) for t in lids_rcv]
    for t, parts in zip(snd + rcv, list(parts_snd) + list(parts_rcv)):
        if len(t[1]) != len(parts) + 1:
            raise ValueError("exchange: a table has not one segment per neighbour")
    data_snd = [np.asarray(values[p])[snd[p][0] - 1].copy() for p in range(n)]  # every pack first
    for p in range(n):  # _check_rcv_and_snd_match
        for q in parts_rcv[p]:
            if not 1 <= int(q) <= n or [int(x) for x in parts_snd[int(q) - 1]].count(p + 1) != 1:
                raise ValueError(f"exchange: part {p + 1} receives from part {int(q)}, which does not send to it")
        for q in parts_snd[p]:
            if not 1 <= int(q) <= n or [int(x) for x in parts_rcv[int(q) - 1]].count(p + 1) != 1:
                raise ValueError(f"exchange: part {p + 1} sends to part {int(q)}, which does not receive from it")
    data_rcv = []
    for q in range(n):
        ptrs_rcv = rcv[q][1]
        buf = np.empty(len(rcv[q][0]), dtype=np.asarray(values[q]).dtype)
        for i, p in enumerate(parts_rcv[q]):
            p = int(p) - 1
            j = [int(x) for x in parts_snd[p]].index(q + 1)
            a, b = _segment(ptrs_rcv, i), _segment(snd[p][1], j)
            if a.stop - a.start != b.stop - b.start:
                raise ValueError(f"exchange: segment {p + 1}→{q + 1} has different lengths on its two sides")
            buf[a] = data_snd[p][b]
        data_rcv.append(buf)
    return data_rcv


def fold(v, lids, data, op, order="ascending"):
    """step 3 for one part: v[lid] = op(v[lid], data[p]) over the buffer"""
    if op not in (REPLACE, ADD):
        raise ValueError(f"exchange: unknown combine op {op!r}")
    if order not in ("ascending", "descending"):
        raise ValueError(f"exchange: unknown order {order!r}")
    lids = np.asarray(lids, dtype=np.int64) - 1
    if len(lids) == 0:
        return v
    o = np.argsort(lids, kind="stable")  # grouped by target, buffer order inside
    sl = lids[o]
    start = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]])
    count = np.diff(np.r_[start, len(sl)])
    rank = np.arange(len(sl)) - np.repeat(start, count)  # position inside its target's group
    if order == "descending":
        rank = np.repeat(count, count) - 1 - rank
    for r in range(int(count.max())):
        sel = o[rank == r]  # one slot per target at most
        t = lids[sel]
        v[t] = v[t] + data[sel] if op == ADD else data[sel]
    return v


def exchange(values, parts_rcv, lids_rcv, parts_snd, lids_snd, op, reverse=False, order="ascending"):
    """exchange!(op, values, exchanger) in place on the list of per-part
    arrays `values`; reverse: with reverse(exchanger) (Interfaces.jl:796-798)"""
    if reverse:
        parts_rcv, lids_rcv, parts_snd, lids_snd = parts_snd, lids_snd, parts_rcv, lids_rcv
    data_rcv = deliver(values, parts_rcv, lids_rcv, parts_snd, lids_snd)
    for v, t, d in zip(values, lids_rcv, data_rcv):
        fold(v, _table(t)[0], d, op, order)
    return values


def zero(values, lids):
    """values[lid] = +0.0 for every part's lids (a store: NaN and -0.0 become
    +0.0, which v*0 would not give)"""
    for v, l in zip(values, lids):
        v[np.asarray(l, dtype=np.int64) - 1] = 0
    return values


def multiplicity(lids, nlids):
    """how many buffer slots name each lid (1-based lids)"""
    return np.bincount(np.asarray(lids, dtype=np.int64) - 1, minlength=nlids)
