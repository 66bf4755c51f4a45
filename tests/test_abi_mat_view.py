"""The entry-view entries of the C-ABI (include/pa_hip.h: pa_mat_scatter,
pa_mat_gather and the table accessor pa_mat_entry_info): declared, exported,
bound with the prototype's arity, and failing loudly on bad arguments, in the
words pa_vec_scatter / pa_vec_gather use (no compute calls: CPU only)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pa_hip.h")

ENTRIES = ["pa_mat_scatter", "pa_mat_gather", "pa_mat_entry_info"]
CONSTANTS = {"PA_IDS_LOCAL": 0, "PA_IDS_GLOBAL": 1, "PA_SCATTER_ADD": 0, "PA_SCATTER_SET": 1}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(pa_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.S)}


def test_header_declares_the_entries():
    protos = _prototypes()
    # (A, rows, cols, ids_kind, index_bytes, op | absent_zero, on_device, n, I, J, V | out)
    assert len(protos["pa_mat_scatter"]) == 11
    assert len(protos["pa_mat_gather"]) == 11
    assert len(protos["pa_mat_entry_info"]) == 3
    # I and J are inputs of both calls (never translated), V of the scatter
    assert protos["pa_mat_scatter"][-3:] == ["const void* I", "const void* J", "const void* V"]
    assert protos["pa_mat_gather"][-3:] == ["const void* I", "const void* J", "void* out"]
    assert protos["pa_mat_gather"][0] == "const pa_mat* A"
    # the deviation from the reference (no insertion into the pattern) is named
    doc = open(HEADER).read()
    assert "the device pattern is fixed" in doc


def test_library_exports_and_binding_matches(pamd):
    L = pamd._lib.lib()
    protos = _prototypes()
    for e in ENTRIES:
        assert hasattr(L, e), e
        assert e in pamd._lib.EXPORTED
        assert len(pamd._lib._SIGS[e]) == len(protos[e]), e
    for name, value in CONSTANTS.items():
        assert getattr(pamd._lib, name) == value, name
    for name in ("MatrixView", "local_view", "global_view", "add_coo_"):
        assert hasattr(pamd, name), name


def test_bad_arguments_are_errors_with_a_message(pamd):
    L = pamd._lib.lib()
    I = (ctypes.c_int64 * 2)(1, 2)
    J = (ctypes.c_int64 * 2)(2, 1)
    vals = (ctypes.c_double * 2)(1.0, 2.0)
    pi, pj, pv = (ctypes.cast(a, ctypes.c_void_p) for a in (I, J, vals))

    def err():
        return L.pa_last_error()

    # null A (every scalar argument valid)
    assert L.pa_mat_scatter(None, None, None, 0, 8, 0, 0, 2, pi, pj, pv) != 0 and b"null" in err()
    assert L.pa_mat_gather(None, None, None, 0, 8, 0, 0, 2, pi, pj, pv) != 0 and b"null" in err()
    assert L.pa_mat_entry_info(None, None, None) != 0 and b"null" in err()
    # bad op
    for op in (-1, 2):
        assert L.pa_mat_scatter(None, None, None, 0, 8, op, 0, 2, pi, pj, pv) != 0 and b"op" in err()
    # bad index_bytes
    for ib in (0, 2, 16):
        assert L.pa_mat_scatter(None, None, None, 0, ib, 0, 0, 2, pi, pj, pv) != 0 and b"index_bytes" in err()
        assert L.pa_mat_gather(None, None, None, 0, ib, 0, 0, 2, pi, pj, pv) != 0 and b"index_bytes" in err()
    # global ids are Int64
    assert L.pa_mat_scatter(None, None, None, 1, 4, 0, 0, 2, pi, pj, pv) != 0 and b"Int64" in err()
    assert L.pa_mat_gather(None, None, None, 1, 4, 0, 0, 2, pi, pj, pv) != 0 and b"Int64" in err()
    # bad ids kind, negative length
    assert L.pa_mat_scatter(None, None, None, 2, 8, 0, 0, 2, pi, pj, pv) != 0 and b"ids_kind" in err()
    assert L.pa_mat_gather(None, None, None, -1, 8, 0, 0, 2, pi, pj, pv) != 0 and b"ids_kind" in err()
    assert L.pa_mat_scatter(None, None, None, 0, 8, 0, 0, -1, pi, pj, pv) != 0 and b"negative" in err()
    assert L.pa_mat_gather(None, None, None, 0, 8, 0, 0, -1, pi, pj, pv) != 0 and b"negative" in err()
    # nothing was written to the inputs
    assert list(I) == [1, 2] and list(J) == [2, 1] and list(vals) == [1.0, 2.0]
