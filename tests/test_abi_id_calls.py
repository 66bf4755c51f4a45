"""The argument failures of the five access-by-id entries of the C-ABI
(pa_vec_scatter, pa_vec_gather, pa_mat_scatter, pa_mat_gather, pa_mat_findnz):
which failure is reported when one or two scalar arguments are bad, and the
whole pa_last_error() text.  The order is op (the scatters), ids_kind,
index_bytes, Int64 for global ids, the length, then the handles; for
pa_mat_findnz which_rows, ids_kind, then the handles.  Null handles
throughout, so nothing is computed (CPU only), and the arrays passed in stay
as they were."""
import ctypes as C
import itertools

import pytest

LOCAL, GLOBAL = 0, 1

# the messages, after the entry's "pa_…: " prefix
OP = "op must be PA_SCATTER_ADD or PA_SCATTER_SET"
KIND = "ids_kind must be PA_IDS_LOCAL or PA_IDS_GLOBAL"
BYTES = "index_bytes must be 4 or 8"
INT64 = "ids=:global needs Int64 ids (index_bytes 8)"
LENGTH = "negative length"
NULL = "null argument"
WHICH = "which_rows must be PA_NZ_OWNED_ROWS or PA_NZ_ALL_ROWS"

# the scalar arguments of the four scatter / gather entries: a valid value and
# the bad ones, in the order their failures are reported
BAD = {"op": (-1, 2), "ids_kind": (-1, 2), "index_bytes": (0, 2, 16), "n": (-1, -7)}
MESSAGE = {"op": OP, "ids_kind": KIND, "index_bytes": BYTES, "n": LENGTH}
ORDER = ["op", "ids_kind", "index_bytes", "n"]
ENTRIES = ["pa_vec_scatter", "pa_vec_gather", "pa_mat_scatter", "pa_mat_gather"]


class Arrays:
    """the arrays a call may read or write, with a pattern to find again"""

    def __init__(self):
        self.I = (C.c_int64 * 4)(11, 12, 13, 14)
        self.J = (C.c_int64 * 4)(21, 22, 23, 24)
        self.V = (C.c_double * 4)(0.5, 1.5, 2.5, 3.5)

    def unchanged(self):
        return (list(self.I) == [11, 12, 13, 14] and list(self.J) == [21, 22, 23, 24]
                and list(self.V) == [0.5, 1.5, 2.5, 3.5])


def _call(L, entry, a, ids_kind=LOCAL, index_bytes=8, op=0, n=4, on_device=0):
    """the entry with null handles; the status and the error text"""
    I, J, V = (C.cast(x, C.c_void_p) for x in (a.I, a.J, a.V))
    if entry == "pa_vec_scatter":
        rc = L.pa_vec_scatter(None, None, ids_kind, index_bytes, op, 0, on_device, n, I, V)
    elif entry == "pa_vec_gather":
        rc = L.pa_vec_gather(None, None, ids_kind, index_bytes, 0, on_device, n, I, V)
    elif entry == "pa_mat_scatter":
        rc = L.pa_mat_scatter(None, None, None, ids_kind, index_bytes, op, on_device, n, I, J, V)
    else:
        rc = L.pa_mat_gather(None, None, None, ids_kind, index_bytes, 0, on_device, n, I, J, V)
    return rc, L.pa_last_error().decode()


def _has_op(entry):
    return entry.endswith("scatter")


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_handles_with_valid_scalars(pamd, entry):
    L, a = pamd._lib.lib(), Arrays()
    for ids_kind, index_bytes in ((LOCAL, 4), (LOCAL, 8), (GLOBAL, 8)):
        for op in ((0, 1) if _has_op(entry) else (0,)):
            for n in (0, 4):
                for on_device in (0, 1):
                    rc, msg = _call(L, entry, a, ids_kind, index_bytes, op, n, on_device)
                    assert rc != 0 and msg == f"{entry}: {NULL}", (ids_kind, index_bytes, op, n, on_device)
    assert a.unchanged()


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_or_two_bad_scalars_report_the_first(pamd, entry):
    L, a = pamd._lib.lib(), Arrays()
    names = [k for k in ORDER if k != "op" or _has_op(entry)]
    seen = 0
    for k in (1, 2):
        for bad in itertools.combinations(names, k):
            for values in itertools.product(*[BAD[b] for b in bad]):
                for ids_kind in ((LOCAL, GLOBAL) if "ids_kind" not in bad else (None,)):
                    kw = dict(zip(bad, values))
                    if ids_kind is not None:
                        kw["ids_kind"] = ids_kind
                    rc, msg = _call(L, entry, a, **kw)
                    first = min(bad, key=ORDER.index)
                    # (with global ids a bad index_bytes is named before the Int64 rule)
                    assert rc != 0 and msg == f"{entry}: {MESSAGE[first]}", (kw, msg)
                    seen += 1
    assert seen >= (40 if _has_op(entry) else 20)
    assert a.unchanged()


@pytest.mark.parametrize("entry", ENTRIES)
def test_global_ids_need_int64(pamd, entry):
    L, a = pamd._lib.lib(), Arrays()
    # alone (the handles are null: the rule is named before them), and before a negative length
    for n in (4, 0, -1):
        rc, msg = _call(L, entry, a, ids_kind=GLOBAL, index_bytes=4, n=n)
        assert rc != 0 and msg == f"{entry}: {INT64}", n
    # a bad op is named before it
    if _has_op(entry):
        for op in BAD["op"]:
            rc, msg = _call(L, entry, a, ids_kind=GLOBAL, index_bytes=4, op=op)
            assert rc != 0 and msg == f"{entry}: {OP}", op
    assert a.unchanged()


def test_findnz_argument_failures(pamd):
    L = pamd._lib.lib()
    out = C.c_void_p(0)

    def call(which_rows, ids_kind, outp=C.byref(out)):
        rc = L.pa_mat_findnz(None, None, None, which_rows, ids_kind, outp)
        return rc, L.pa_last_error().decode()

    for which_rows in (0, 1):
        for ids_kind in (LOCAL, GLOBAL):
            assert call(which_rows, ids_kind) == (-1, f"pa_mat_findnz: {NULL}")
            assert call(which_rows, ids_kind, None) == (-1, f"pa_mat_findnz: {NULL}")
    for bad in (-1, 2, 7):
        for ok in (0, 1):
            assert call(bad, ok) == (-1, f"pa_mat_findnz: {WHICH}")
            assert call(ok, bad) == (-1, f"pa_mat_findnz: {KIND}")
        for bad2 in (-1, 2, 7):  # both bad: which_rows first
            assert call(bad, bad2) == (-1, f"pa_mat_findnz: {WHICH}")
    assert out.value in (None, 0)  # nothing was handed out
