"""exchange!(I, J, V, rows), host side (no device): the restatement of
Interfaces.jl:2494-2592 the GPU tests compare against (coo_exchange_ref.py),
pinned by a case worked by hand from the reference's lines, and the entry
point pa_coo_exchange_all of the library."""
import ctypes as C

import numpy as np
import pytest

from coo_exchange_ref import classify, exchange_coo_, oracle_lists, problem


def _hand_case(O):
    """Three linear parts over 9 gids (part p owns 3p-2..3p).  add_gids!
    makes gid 5 (owned by part 2) a ghost of parts 1 and 3, and gid 7 (owned
    by part 3) a ghost of part 2."""
    oparts = O.get_part_ids(3)
    rows = O.prange_linear(oparts, 9)
    I = O.PData([[1, 5], [5, 4, 7], [5, 7]])
    J = O.PData([[1, 2], [5, 4, 1], [9, 7]])
    V = O.PData([np.array([1.0, np.nan]), np.array([2.0, 3.0, 4.0]), np.array([5.0, 6.0])])
    O.add_gids_(rows, O.PData([list(i) for i in I.parts]))
    return rows, I, J, V


def test_restatement_hand_worked_case(O):
    rows, I, J, V = _hand_case(O)
    ex = rows.exchanger
    # the exchanger the reference builds (Interfaces.jl:723-786): part 2 sends
    # gid 5 (its lid 2) to part 1 and to part 3, part 3 sends gid 7 to part 2
    assert [list(p) for p in ex.parts_rcv.parts] == [[2], [3], [2]]
    assert [list(p) for p in ex.parts_snd.parts] == [[], [1, 3], [2]]
    assert ex.lids_snd[2].tolist() == [[2], [2]] and ex.lids_snd[3].tolist() == [[1]]
    rI, rJ, rV = exchange_coo_(O, I, J, V, rows)
    # part 1: row 5 is a ghost row here and no send segment lists it: NaN → +0.0
    # (2529-2530).  lid_to_i[2] of part 2 was overwritten by segment 2 (part 3,
    # 2514-2520), so nothing of row 5 arrives here.
    assert rI[1] == [1, 5] and rJ[1] == [1, 2]
    assert rV[1].tobytes() == np.array([1.0, 0.0]).tobytes()
    # part 2: row 5 is sent (entry kept, value included), row 4 is held by
    # nobody, row 7 is a ghost row → +0.0; part 3's triplet of row 7 arrives
    assert rI[2] == [5, 4, 7, 7] and rJ[2] == [5, 4, 1, 7]
    assert rV[2].tobytes() == np.array([2.0, 3.0, 0.0, 6.0]).tobytes()
    # part 3: its own row-5 triplet is a ghost row's → +0.0; row 7 is sent and
    # kept; part 2's triplet of row 5 arrives here, the later neighbour only
    assert rI[3] == [5, 7, 5] and rJ[3] == [9, 7, 5]
    assert rV[3].tobytes() == np.array([0.0, 6.0, 2.0]).tobytes()


def test_restatement_unknown_row_gid_is_a_keyerror(O):
    rows, I, J, V = _hand_case(O)
    I.parts[0][1] = 9  # not a local id of part 1
    with pytest.raises(KeyError):
        exchange_coo_(O, I, J, V, rows)


def test_restatement_counts_are_not_vacuous(pamd, O):
    """the drawing the GPU tests use moves triplets, zeroes ghost rows and
    sends rows that sit in several send segments (checked on the smallest
    Cartesian case)"""
    parts, oparts, rows, orows, I, J, V, mk = problem(pamd, O, pamd.sequential, (2, 2), (30, 28), 1500, np.float64,
                                                      20250114, with_ghost=True)
    cls = classify(orows, parts.part_ids, I)
    oI, oJ, oV = oracle_lists(O, parts.part_ids, oparts, I, J, V)
    rI, rJ, rV = exchange_coo_(O, oI, oJ, oV, orows)
    sent = sum(int((cls[p][0] == 1).sum()) for p in parts.part_ids)
    moved = sum(len(rI[p]) - len(I[p]) for p in parts.part_ids)
    assert moved == sent > 0
    for p in parts.part_ids:
        kind, _ = cls[p]
        n = len(I[p])
        assert rI[p][:n] == list(map(int, I[p])) and rJ[p][:n] == list(map(int, J[p]))
        keep = kind != 2
        assert rV[p][:n][keep].tobytes() == V[p][keep].tobytes()
        assert (kind == 2).any() and rV[p][:n][~keep].tobytes() == np.zeros(int((~keep).sum())).tobytes()
    assert sum(int(((cls[p][0] == 1) & (cls[p][1] >= 2)).sum()) for p in parts.part_ids) > 0


def test_entry_point_is_bound_and_checks_its_arguments(pamd):
    L = pamd._lib.lib()
    assert "pa_coo_exchange_all" in pamd._lib.EXPORTED and hasattr(L, "pa_coo_exchange_all")
    assert pamd._lib._SIGS["pa_coo_exchange_all"] == pamd._lib._SIGS["pa_coo_assemble_all"]
    null = pamd._lib.ptr_array([None])
    with pytest.raises(pamd.PAError, match="null"):
        pamd._lib.call("pa_coo_exchange_all", 0, null, null, null)
    with pytest.raises(pamd.PAError, match="null"):
        pamd._lib.call("pa_coo_exchange_all", 1, None, None, None)
    with pytest.raises(pamd.PAError, match="null"):
        pamd._lib.call("pa_coo_exchange_all", 1, null, null, null)
    with pytest.raises(pamd.PAError, match="null"):
        pamd._lib.call("pa_coo_exchange_all", 2, C.cast(None, C.POINTER(C.c_void_p)), null, null)


def test_exchange_of_a_coo_needs_rows(pamd):
    coo = pamd.COO(None)
    with pytest.raises(TypeError, match="rows"):
        pamd.exchange_(coo)
