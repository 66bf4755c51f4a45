"""tests/table_exchange_ref.py, the numpy reference of the device table
exchange tests, pinned to the oracle's literal restatement of
async_exchange!(combine_op, values::AbstractPData{<:Table}, exchanger)
(pa_oracle.exchange_table_values_, Interfaces.jl:899-961): on the reference's
own irregular partition with the rows of test_interfaces.jl:255-264, and on
the cases of tests/table_exchange_cases.py for replace and add.  The class,
length and fold-order conditions that the device tests rely on are asserted
here, on the reference side."""
import json
import os

import numpy as np
import pytest

import exchange_cases as X
import exchange_ref as R
import table_exchange_cases as TC
import table_exchange_ref as T

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "interfaces_kats.json")))
_DT = lambda d: np.dtype(d).name


def _tables(ex):
    return ([list(p) for p in ex.parts_rcv.parts], list(ex.lids_rcv.parts),
            [list(p) for p in ex.parts_snd.parts], list(ex.lids_snd.parts))


@pytest.fixture(scope="module")
def cases(O):
    c = TC.small_cases()
    g = c["ghost"]  # its exchanger: the one the index sets imply
    part = O.PData([O.IndexSet(p + 1, [int(x) for x in g.lid_to_gid[p]], [int(x) for x in g.lid_to_part[p]])
                    for p in range(g.nparts)])
    ex = O.exchanger_from_ids(part)
    tabs = lambda t: [(np.asarray(x.data, np.int32), np.asarray(x.ptrs, np.int32)) for x in t.parts]
    g.set_tables([np.asarray(p, np.int32) for p in ex.parts_rcv.parts], tabs(ex.lids_rcv),
                 [np.asarray(p, np.int32) for p in ex.parts_snd.parts], tabs(ex.lids_snd))
    return c


def test_expand_by_hand():
    """rows of 2, 0, 3 and 1 entries; the lists name lids [3, 1 | 2, 4, 3]"""
    tptrs = [1, 3, 3, 6, 7]
    data, ptrs = T.expand(([3, 1, 2, 4, 3], [1, 3, 6]), tptrs)
    assert data.tolist() == [3, 4, 5, 1, 2, 6, 3, 4, 5] and ptrs.tolist() == [1, 6, 10]
    data, ptrs = T.expand(([], [1, 1]), tptrs)
    assert data.tolist() == [] and ptrs.tolist() == [1, 1]
    data, ptrs = T.expand(([2, 2], [1, 2, 3]), tptrs)  # empty rows only
    assert data.tolist() == [] and ptrs.tolist() == [1, 1, 1]


def test_kat_rows_reach_every_ghost(O):
    """test_interfaces.jl:255-264: owned rows [100*owner + 10*gid + i], the
    ghost rows zero; after the exchange every lid holds its owner's row — and
    the oracle's run gives the same bytes"""
    k = GOLD["exchanger"]
    part = O.PData([O.IndexSet(p + 1, k["lid_to_gid"][p], k["lid_to_part"][p]) for p in range(4)])
    ex = O.exchanger_from_ids(part)

    def mk(s):
        vv = [[0, 0, 0] for _ in range(s.num_lids)]
        for lid in s.oid_to_lid:
            vv[lid - 1] = [100 * s.part + 10 * s.lid_to_gid[lid - 1] + i for i in (1, 2, 3)]
        return O.table_from(vv)
    vals = O.map_parts(mk, part)
    data = [np.asarray(t.data, np.int64).copy() for t in vals.parts]
    tptrs = [np.asarray(t.ptrs) for t in vals.parts]
    T.exchange(data, tptrs, *_tables(ex), R.REPLACE)
    O.exchange_table_values_(vals, ex)
    for s, d, t in zip(part.parts, data, vals.parts):
        assert d.tobytes() == np.asarray(t.data, np.int64).tobytes()
        for lid in range(1, s.num_lids + 1):
            gid, owner = s.lid_to_gid[lid - 1], s.lid_to_part[lid - 1]
            assert d[3 * (lid - 1):3 * lid].tolist() == [100 * owner + 10 * gid + i for i in (1, 2, 3)]


@pytest.mark.parametrize("dtype", [np.float32, np.complex128], ids=_DT)
@pytest.mark.parametrize("op", [R.REPLACE, R.ADD])
@pytest.mark.parametrize("name", TC.CASES)
def test_oracle_table_exchange_on_the_cases(O, cases, name, op, dtype):
    case = cases[name]
    tptrs = TC.table_ptrs(case)
    mode = (op, 0, 0)
    start = TC.start_data(case, tptrs, dtype, mode)
    want = TC.expected(case, tptrs, start, mode)
    mk = lambda xs: O.PData(list(xs))
    ex = O.Exchanger(mk([list(p) for p in case.parts_rcv]), mk([list(p) for p in case.parts_snd]),
                     mk([O.Table(d, p) for d, p in case.lids_rcv]), mk([O.Table(d, p) for d, p in case.lids_snd]))
    vals = mk([O.Table(d.copy(), p) for d, p in zip(start, tptrs)])
    O.exchange_table_values_(vals, ex, O._replace if op == R.REPLACE else (lambda a, b: a + b))
    for w, t in zip(want, vals.parts):
        assert w.dtype == dtype and w.tobytes() == np.asarray(t.data, dtype=dtype).tobytes()
    assert any(w.tobytes() != s.tobytes() for w, s in zip(want, start))  # something moved


def test_zero_sent_rows():
    tptrs = [[1, 3, 3, 6, 7]]
    v = [np.array([np.nan, -0.0, 1.0, 2.0, 3.0, 4.0])]
    T.zero(v, tptrs, [([1, 2, 4], [1, 4])])
    assert v[0].tobytes() == np.array([0.0, 0.0, 1.0, 2.0, 3.0, 0.0]).tobytes()


# ---- what the device tests rely on ------------------------------------------------

def test_dup_collapses_into_one_class():
    """why dup is not a table case: nearly all of its travelling lids share
    one length"""
    c = X.small_cases()["dup"]
    cls = np.concatenate(T.classes(c.sizes, *c.tables))
    cls = cls[cls >= 0]
    assert len(cls) == 156 and len(np.unique(cls)) == 3 and np.bincount(cls).max() == 151


@pytest.mark.parametrize("name", TC.CASES)
def test_classes_and_lengths(cases, name):
    case = cases[name]
    for variant in (0, 1):
        tptrs = TC.table_ptrs(case, variant)
        assert [len(t) for t in tptrs] == [n + 1 for n in case.sizes]
        lids, ncls, largest = T.check_lengths(case.sizes, case.tables, tptrs)
        print(f"{name}/{variant}: {lids} travelling lids, {ncls} classes, largest {largest}, "
              f"{sum(int(t[-1]) - 1 for t in tptrs)} data entries")
        if name == "forward":
            assert (lids, ncls, largest) == (126, 30, 9)
        if name == "lonely":
            assert (lids, ncls, largest) == (135, 18, 78)
        if name == "ghost":  # one class per ghosted gid
            assert ncls == len(np.unique(np.concatenate([case.lid_to_gid[p][case.hids[p] - 1]
                                                         for p in range(case.nparts)])))
    a, b = TC.table_ptrs(case, 0), TC.table_ptrs(case, 1)
    assert any(not np.array_equal(x, y) for x, y in zip(a, b))  # the second table has other lengths


def test_tdup_is_built_class_first(cases):
    case = cases["tdup"]
    assert tuple(case.sizes) == (41, 300, 17) and len(case.classes) >= 40
    used = set()
    for q, lt, src in case.classes:
        assert 2 <= len(src) <= 4 and all(p != q for p, _ in src)
        for key in [(q, lt)] + src:
            assert key not in used  # every lid in one class at most
            used.add(key)
    cls = T.classes(case.sizes, *case.tables)
    assert len(np.unique(np.concatenate(cls)[np.concatenate(cls) >= 0])) == len(case.classes)
    for q, lt, src in case.classes:  # a class is its target row and its source rows
        assert {int(cls[p - 1][l - 1]) for p, l in [(q, lt)] + src} == {int(cls[q - 1][lt - 1])}
    # two slots of one segment naming the same target
    inside = 0
    for q in range(case.nparts):
        data, ptrs = case.lids_rcv[q]
        dup = set()
        for k in range(len(ptrs) - 1):
            seg = data[ptrs[k] - 1:ptrs[k + 1] - 1]
            u, n = np.unique(seg, return_counts=True)
            dup.update(u[n >= 2].tolist())
        inside += len(dup)
    assert inside >= 10
    # target rows (forward) with two or more contributions
    several = sum(int((R.multiplicity(t[0], n) >= 2).sum()) for t, n in zip(case.lids_rcv, case.sizes))
    assert several >= 30


FOLD = [(n, d) for n in TC.CASES for d in X.DTYPES]


@pytest.mark.parametrize("name,dtype", FOLD, ids=[f"{n}-{_DT(d)}" for n, d in FOLD])
def test_values_make_fold_order_visible(cases, name, dtype):
    """Folding in descending slot order changes the bits of at least 10 % of
    the data entries with several contributions in the ADD runs (the existing
    exchange test's threshold), asserted wherever those runs hold at least 100
    such entries; tdup and lonely must."""
    case = cases[name]
    multi, changed = TC.fold_order_stats(case, TC.table_ptrs(case), dtype, X.MODES)
    print(f"{name} {_DT(dtype)}: {multi} entries with several contributions in ADD runs, descending order "
          f"changes {changed}")
    if name in ("tdup", "lonely"):
        assert multi >= 100
    if multi >= 100:
        assert changed >= 0.10 * multi
