"""The cases of the table exchange tests: the exchanger cases of
tests/exchange_cases.py that suit tables (ghost, forward, lonely), the case
tdup built class-first, the row pointers of every part and the data the runs
start from — numpy alone (seeded), so the reference side needs no device.

A row length belongs to a class of (part, lid) pairs (table_exchange_ref.
classes).  exchange_cases' dup draws its lids with replacement, which chains
nearly all of them into one class (151 of its 156 travelling lids): its rows
would all be equally long, so it is not used here.  tdup keeps dup's point —
several contributions to one target, some from inside one segment — with one
class per target:

  three parts of 41 / 300 / 17 lids, 41 classes, every lid in at most one;
  25 classes: target on part 1, 2-4 source rows on part 2 (every such class
     has two slots of segment 2→1 naming one target);
   8 classes: target on part 3, 1-3 sources on part 2, three of them one more
     on part 1;
   8 classes: target on part 2, sources (1, 1, 3) or (1, 3).
  The slots of a segment are shuffled (both sides alike)."""
import numpy as np

import exchange_cases as X
import exchange_ref as R
import table_exchange_ref as T

CASES = ("ghost", "forward", "lonely", "tdup")
TDUP_SIZES = (41, 300, 17)


def tdup_case():
    rng = np.random.default_rng(X.SEED + 11)
    free = [list(rng.permutation(n) + 1) for n in TDUP_SIZES]  # unused lids of every part
    take = lambda part: int(free[part - 1].pop())
    classes = []  # (target part, target lid, [(source part, source lid)])
    for _ in range(25):
        classes.append((1, take(1), [(2, take(2)) for _ in range(int(rng.integers(2, 5)))]))
    for i in range(8):
        src = [(2, take(2)) for _ in range(int(rng.integers(1, 4)))] + ([(1, take(1))] if i < 3 else [])
        if len(src) < 2:
            src.append((2, take(2)))
        classes.append((3, take(3), src))
    for i in range(8):
        classes.append((2, take(2), [(1, take(1)), (3, take(3))] + ([(1, take(1))] if i < 4 else [])))
    segs = {}  # (sender, receiver) → [(send lid, receive lid)]
    for q, lt, src in classes:
        assert 2 <= len(src) <= 4 and all(p != q for p, _ in src)
        for p, ls in src:
            segs.setdefault((p, q), []).append((ls, lt))
    for k in segs:
        segs[k] = [segs[k][i] for i in rng.permutation(len(segs[k]))]
    nparts = len(TDUP_SIZES)
    parts_rcv = [np.array(sorted(p for p, q in segs if q == r + 1), np.int32) for r in range(nparts)]
    parts_snd = [np.array(sorted(q for p, q in segs if p == r + 1), np.int32) for r in range(nparts)]
    lids_rcv = [X._table([[b for _, b in segs[(int(p), r + 1)]] for p in parts_rcv[r]]) for r in range(nparts)]
    lids_snd = [X._table([[a for a, _ in segs[(r + 1, int(q))]] for q in parts_snd[r]]) for r in range(nparts)]
    # an index set to carry the lists: every lid owned, consecutive gids
    first = np.concatenate([[1], 1 + np.cumsum(TDUP_SIZES)])
    l2g = [np.arange(first[p], first[p] + n, dtype=np.int64) for p, n in enumerate(TDUP_SIZES)]
    l2p = [np.full(n, p + 1, np.int32) for p, n in enumerate(TDUP_SIZES)]
    case = X.Case("tdup", TDUP_SIZES, l2g, l2p, (parts_rcv, lids_rcv, parts_snd, lids_snd))
    case.classes = classes
    return case


def small_cases():
    """ghost, forward, lonely of exchange_cases (ghost's tables: set by the
    caller from exchanger_from_ids) and tdup"""
    c = X.small_cases()
    out = {k: c[k] for k in ("ghost", "forward", "lonely")}
    out["tdup"] = tdup_case()
    return out


def table_ptrs(case, variant=0):
    """the row pointers of a case (seeded by its name; variant: another draw)"""
    rng = np.random.default_rng([X.SEED, 31, sum(map(ord, case.name)), variant])
    return T.row_lengths(case.sizes, case.tables, rng)


def start_data(case, tptrs, dtype, mode, salt=0):
    """The data before the call: family values in the rows that travel,
    SENTINEL in the others.  REPLACE: NaN, ±Inf and -0.0 sit in up to four
    entries that are sent.  (zero_sent zeroes the rows a transfer left from:
    REPLACE runs may hold the NaN there, ADD runs compare no NaN.)"""
    op, reverse, _ = mode
    rng = np.random.default_rng([X.SEED, 37, sum(map(ord, case.name)), np.dtype(dtype).num, X.MODES.index(mode), salt])
    sp = X._specials(dtype)
    out = []
    for p in range(case.nparts):
        n = int(tptrs[p][-1]) - 1
        v = X.family(rng, n, dtype)
        named = np.zeros(n, bool)
        for t in (case.lids_rcv[p], case.lids_snd[p]):
            named[T.expand(t, tptrs[p])[0] - 1] = True
        v[~named] = X.SENTINEL
        sent = np.unique(T.expand(case.frm(reverse)[p], tptrs[p])[0])
        if op == R.REPLACE and len(sent):
            pick = rng.choice(sent, min(4, len(sent)), replace=False)
            v[pick - 1] = sp[:len(pick)]
        out.append(v)
    return out


def expected(case, tptrs, start, mode, order="ascending", zero=True):
    op, reverse, z = mode
    v = [a.copy() for a in start]
    T.exchange(v, tptrs, *case.tables, op, bool(reverse), order)
    if z and zero:
        T.zero(v, tptrs, case.frm(reverse))
    return v


def fold_order_stats(case, tptrs, dtype, modes):
    """Over the ADD runs among `modes`: the data entries with two or more
    contributions and how many of them change their bits when folded in
    descending slot order."""
    multi_add = changed = 0
    for mode in modes:
        op, reverse, _ = mode
        if op != R.ADD:
            continue
        several = [m >= 2 for m in T.multiplicity(tptrs, case.into(reverse))]
        start = start_data(case, tptrs, dtype, mode)
        up = expected(case, tptrs, start, mode, zero=False)
        down = expected(case, tptrs, start, mode, "descending", zero=False)
        for s, a, b in zip(several, up, down):
            w = a.dtype.itemsize
            differ = (a.view(np.uint8).reshape(-1, w) != b.view(np.uint8).reshape(-1, w)).any(axis=1)
            multi_add += int(s.sum())
            changed += int(differ[s].sum())
            assert not differ[~s].any()  # one contribution: no order
    return multi_add, changed
