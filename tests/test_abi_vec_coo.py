"""The COO-constructor / indexed-view entries of the C-ABI (include/pa_hip.h:
pa_vec_scatter, pa_vec_gather and their four constants): declared, exported,
bound with the prototype's arity, and failing loudly on bad arguments (no
compute calls: CPU only)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pa_hip.h")

ENTRIES = ["pa_vec_scatter", "pa_vec_gather"]
CONSTANTS = {"PA_IDS_LOCAL": 0, "PA_IDS_GLOBAL": 1, "PA_SCATTER_ADD": 0, "PA_SCATTER_SET": 1}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(pa_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.S)}


def test_header_declares_the_entries_and_constants():
    src = open(HEADER).read()
    protos = _prototypes()
    assert len(protos["pa_vec_scatter"]) == 10
    assert len(protos["pa_vec_gather"]) == 9
    for name, value in CONSTANTS.items():
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)\b", src, re.M)
        assert m and int(m.group(1)) == value, name


def test_library_exports_and_binding_matches(pamd):
    L = pamd._lib.lib()
    protos = _prototypes()
    for e in ENTRIES:
        assert hasattr(L, e), e
        assert e in pamd._lib.EXPORTED
        assert len(pamd._lib._SIGS[e]) == len(protos[e]), e
    for name, value in CONSTANTS.items():
        assert getattr(pamd._lib, name) == value, name


def test_bad_arguments_are_errors_with_a_message(pamd):
    L = pamd._lib.lib()
    ids = (ctypes.c_int64 * 2)(1, 2)
    vals = (ctypes.c_double * 2)(1.0, 2.0)
    pi, pv = ctypes.cast(ids, ctypes.c_void_p), ctypes.cast(vals, ctypes.c_void_p)

    def err():
        return L.pa_last_error()

    # null v (every scalar argument valid)
    assert L.pa_vec_scatter(None, None, 0, 8, 0, 1, 0, 2, pi, pv) != 0 and b"null" in err()
    assert L.pa_vec_gather(None, None, 0, 8, 0, 0, 2, pi, pv) != 0 and b"null" in err()
    # bad op
    for op in (-1, 2):
        assert L.pa_vec_scatter(None, None, 0, 8, op, 0, 0, 2, pi, pv) != 0 and b"op" in err()
    # bad index_bytes
    for ib in (0, 2, 16):
        assert L.pa_vec_scatter(None, None, 0, ib, 0, 0, 0, 2, pi, pv) != 0 and b"index_bytes" in err()
        assert L.pa_vec_gather(None, None, 0, ib, 0, 0, 2, pi, pv) != 0 and b"index_bytes" in err()
    # global ids are Int64
    assert L.pa_vec_scatter(None, None, 1, 4, 0, 0, 0, 2, pi, pv) != 0 and b"Int64" in err()
    assert L.pa_vec_gather(None, None, 1, 4, 0, 0, 2, pi, pv) != 0 and b"Int64" in err()
    # bad ids kind, negative length
    assert L.pa_vec_scatter(None, None, 2, 8, 0, 0, 0, 2, pi, pv) != 0 and b"ids_kind" in err()
    assert L.pa_vec_gather(None, None, 0, 8, 0, 0, -1, pi, pv) != 0 and b"negative" in err()
    # nothing was written to the inputs
    assert list(ids) == [1, 2] and list(vals) == [1.0, 2.0]
