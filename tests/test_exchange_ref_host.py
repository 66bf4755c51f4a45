"""tests/exchange_ref.py, the numpy reference of the device exchange tests,
pinned three ways: to values worked out by hand, to the oracle's literal
exchange_values_ loop on the reference's own irregular partition, and to the
reference's reverse-add-then-exchange sequence (test_interfaces.jl:276-287)."""
import json
import os

import numpy as np
import pytest

import exchange_ref as R

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "interfaces_kats.json")))

# Three parts of 4, 5 and 3 lids.  Segments (forward):
#   1→2: part 1 sends lids [2, 2, 4]; part 2 receives them on lids [3, 1, 3]
#   3→2: part 3 sends lids [1, 3];    part 2 receives them on lids [3, 5]
#   2→1: part 2 sends lid  [5];       part 1 receives it on lid   [2]
#   2→3: part 2 sends lids [3, 2];    part 3 receives them on lids [2, 2]
# Lid 3 of part 2 is named three times (twice inside 1→2's segment, once in
# 3→2's) and is also sent on to part 3 (forwarded: its old value travels);
# lid 2 of part 1 is sent and received as well.
PARTS_SND = [[2], [1, 3], [2]]
LIDS_SND = [([2, 2, 4], [1, 4]), ([5, 3, 2], [1, 2, 4]), ([1, 3], [1, 3])]
PARTS_RCV = [[2], [1, 3], [2]]
LIDS_RCV = [([2], [1, 2]), ([3, 1, 3, 3, 5], [1, 4, 6]), ([2, 2], [1, 3])]
START = [[1, 2, 3, 4], [10, 20, 30, 40, 50], [100, 200, 300]]

# buffers forward: part 1 gets [50]; part 2 gets [2, 2, 4 | 100, 300]; part 3 gets [30, 20]
# buffers reverse: part 1 gets [30, 10, 30] on lids [2, 2, 4]; part 2 gets [2] on lid [5] and
#                  [200, 200] on lids [3, 2]; part 3 gets [30, 50] on lids [1, 3]
HAND = {
    (R.REPLACE, False, "ascending"): [[1, 50, 3, 4], [2, 20, 100, 40, 300], [100, 20, 300]],
    (R.ADD, False, "ascending"): [[1, 52, 3, 4], [12, 20, 136, 40, 350], [100, 250, 300]],
    (R.REPLACE, True, "ascending"): [[1, 10, 3, 30], [10, 200, 200, 40, 2], [30, 200, 50]],
    (R.ADD, True, "ascending"): [[1, 42, 3, 34], [10, 220, 230, 40, 52], [130, 200, 350]],
    # the first slot in buffer order wins instead of the last
    (R.REPLACE, False, "descending"): [[1, 50, 3, 4], [2, 20, 2, 40, 300], [100, 30, 300]],
    (R.REPLACE, True, "descending"): [[1, 30, 3, 30], [10, 200, 200, 40, 2], [30, 200, 50]],
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("key", list(HAND), ids=lambda k: f"{k[0]}-{'rev' if k[1] else 'fwd'}-{k[2]}")
def test_hand_worked(key, dtype):
    op, reverse, order = key
    vals = [np.array(v, dtype=dtype) for v in START]
    if np.dtype(dtype).kind == "c":  # the imaginary parts move with the real ones
        vals = [v * (1 - 2j) for v in vals]
    got = R.exchange(vals, PARTS_RCV, LIDS_RCV, PARTS_SND, LIDS_SND, op, reverse, order)
    assert got is vals
    for g, w in zip(got, HAND[key]):
        w = np.array(w, dtype=dtype) * ((1 - 2j) if np.dtype(dtype).kind == "c" else 1)
        assert g.dtype == dtype and g.tobytes() == w.astype(dtype).tobytes()


def test_one_rounding_per_add_in_buffer_order():
    """Float32 1 + 2^24 rounds to 2^24 (ties to even), then - 2^24 gives 0;
    the other way round 1 - 2^24 is exact and + 2^24 gives back 1.  Float64
    holds every intermediate exactly: 1 both ways."""
    big = 2.0 ** 24
    for dtype, asc in ((np.float32, 0.0), (np.float64, 1.0)):
        for order, want in (("ascending", asc), ("descending", 1.0)):
            vals = [np.array([big, -big], dtype=dtype), np.array([1.0], dtype=dtype)]
            R.exchange(vals, [[], [1]], [([], [1]), ([1, 1], [1, 3])], [[2], []], [([1, 2], [1, 3]), ([], [1])],
                       R.ADD, False, order)
            assert vals[1].tobytes() == np.array([want], dtype=dtype).tobytes(), (dtype, order)


def test_special_values_travel_bit_for_bit():
    nan = np.frombuffer(np.uint64(0x7FF8_0000_DEAD_BEEF).tobytes(), np.float64)[0]
    vals = [np.array([nan, -0.0, np.inf, -np.inf]), np.array([1.0, 2.0, 3.0, 4.0, 5.0])]
    want = np.array([nan, 2.0, -np.inf, np.inf, -0.0])
    R.exchange(vals, [[], [1]], [([], [1]), ([1, 5, 4, 3], [1, 5])], [[2], []], [([1, 2, 3, 4], [1, 5]), ([], [1])],
               R.REPLACE)
    assert vals[1].tobytes() == want.tobytes()


def test_zero_is_a_store():
    v = [np.array([np.nan, -0.0, -1.0, 7.0]), np.array([np.inf + 1j * np.nan, 2.0], dtype=np.complex64)]
    R.zero(v, [[1, 2, 3], [1]])
    assert v[0].tobytes() == np.array([0.0, 0.0, 0.0, 7.0]).tobytes()
    assert v[1].tobytes() == np.array([0.0, 2.0], dtype=np.complex64).tobytes()


def test_mismatches_raise():
    vals = lambda: [np.array(v, dtype=np.float64) for v in START]
    with pytest.raises(ValueError, match="does not send to it"):
        R.exchange(vals(), PARTS_RCV, LIDS_RCV, [[2], [1, 3], []], LIDS_SND[:2] + [([], [1])], R.REPLACE)
    with pytest.raises(ValueError, match="does not receive from it"):
        R.exchange(vals(), [[2], [1, 3], []], LIDS_RCV[:2] + [([], [1])], PARTS_SND, LIDS_SND, R.REPLACE)
    with pytest.raises(ValueError, match="different lengths"):
        R.exchange(vals(), PARTS_RCV, LIDS_RCV, PARTS_SND, [([2, 4], [1, 3])] + LIDS_SND[1:], R.REPLACE)
    with pytest.raises(ValueError, match="different lengths"):  # the same check with the roles swapped
        R.exchange(vals(), PARTS_RCV, LIDS_RCV, PARTS_SND, [([2, 4], [1, 3])] + LIDS_SND[1:], R.ADD, reverse=True)
    with pytest.raises(ValueError, match="unknown combine op"):
        R.exchange(vals(), PARTS_RCV, LIDS_RCV, PARTS_SND, LIDS_SND, "max")


def test_empty_segments_and_parts():
    """a zero-length segment that both sides list, and a part without lids"""
    vals = [np.array([1.0, 2.0]), np.array([5.0]), np.zeros(0)]
    R.exchange(vals, [[2], [1], []], [([], [1, 1]), ([1], [1, 2]), ([], [1])],
               [[2], [1], []], [([2], [1, 2]), ([], [1, 1]), ([], [1])], R.ADD)
    assert [v.tolist() for v in vals] == [[1.0, 2.0], [7.0], []]


# ---------------------------------------------------------------------------
# against the oracle's literal loop on the reference's irregular partition

def _kat(O):
    k = GOLD["exchanger"]
    part = O.PData([O.IndexSet(p + 1, k["lid_to_gid"][p], k["lid_to_part"][p]) for p in range(4)])
    return part, O.exchanger_from_ids(part)


def _tables(ex):
    return ([list(p) for p in ex.parts_rcv.parts], list(ex.lids_rcv.parts),
            [list(p) for p in ex.parts_snd.parts], list(ex.lids_snd.parts))


def _values(rng, n, dtype):
    """±u·2^k, u in [1, 2), k in -8..8: sums of them round, so fold order shows"""
    def one():
        return rng.choice([-1.0, 1.0], n) * rng.uniform(1, 2, n) * 2.0 ** rng.integers(-8, 9, n)
    return (one() + 1j * one()).astype(dtype) if np.dtype(dtype).kind == "c" else one().astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("op", [R.REPLACE, R.ADD])
def test_oracle_exchange_values_on_the_kat_partition(O, op, reverse, dtype):
    part, ex = _kat(O)
    rng = np.random.default_rng(20250114)
    start = [_values(rng, s.num_lids, dtype) for s in part.parts]
    ov = O.PData([v.copy() for v in start])
    O.exchange_values_(O._replace if op == R.REPLACE else (lambda a, b: a + b), ov, ov,
                       O.reverse_exchanger(ex) if reverse else ex)
    got = R.exchange([v.copy() for v in start], *_tables(ex), op, reverse)
    changed = 0
    for g, w, s in zip(got, ov.parts, start):
        assert g.dtype == dtype and g.tobytes() == np.asarray(w, dtype=dtype).tobytes()
        changed += int(np.count_nonzero(g != s))
    assert changed >= 4  # the exchange moved something


def test_reverse_add_then_exchange(O):
    """test_interfaces.jl:276-287: exchange!(+, values, reverse(exchanger))
    then exchange!(values, exchanger); every copy of a gid ends with the
    owner's assembled value, and the oracle's run of the sequence agrees"""
    part, ex = _kat(O)
    T = _tables(ex)
    vals = [np.full(s.num_lids, 10.0 * s.part) for s in part.parts]
    R.exchange(vals, *T, R.ADD, True)
    R.exchange(vals, *T, R.REPLACE, False)
    ov = O.map_parts(lambda s: np.full(s.num_lids, 10.0 * s.part), part)
    O.exchange_values_(lambda a, b: a + b, ov, ov, O.reverse_exchanger(ex))
    O.exchange_(ov, ex)
    for v, w in zip(vals, ov.parts):
        assert v.tobytes() == np.asarray(w, dtype=np.float64).tobytes()
    tot = {}
    for s, v in zip(part.parts, vals):
        for lid in s.oid_to_lid:
            tot[s.lid_to_gid[lid - 1]] = v[lid - 1]
    holders = {}
    for s in part.parts:
        for g in s.lid_to_gid:
            holders.setdefault(g, []).append(s.part)
    for s, v in zip(part.parts, vals):
        for lid in range(1, s.num_lids + 1):
            g = s.lid_to_gid[lid - 1]
            assert v[lid - 1] == tot[g] == 10.0 * sum(holders[g])
