"""The findnz entries of the C-ABI (include/pa_hip.h: pa_mat_findnz and
pa_index_to_gids): declared, exported, bound with the prototype's arity, their
constants, and failing loudly on null and bad arguments before anything is
allocated (no compute calls: CPU only)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pa_hip.h")

ENTRIES = ["pa_mat_findnz", "pa_index_to_gids"]
CONSTANTS = {"PA_NZ_OWNED_ROWS": 0, "PA_NZ_ALL_ROWS": 1, "PA_IDS_LOCAL": 0, "PA_IDS_GLOBAL": 1}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(pa_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.S)}


def test_header_declares_the_entries():
    protos = _prototypes()
    assert protos["pa_mat_findnz"] == ["pa_mat* A", "pa_index* rows", "pa_index* cols", "int which_rows",
                                       "int ids_kind", "pa_coo** out"]
    # the mirror of pa_index_to_lids, parameter for parameter
    assert protos["pa_index_to_gids"] == protos["pa_index_to_lids"] == ["pa_index* idx", "int64_t n", "int64_t* ids"]
    src = open(HEADER).read()
    for name, value in CONSTANTS.items():
        assert re.search(rf"#define\s+{name}\s+{value}\b", src), name
    # the order contract and its one deviation are stated where the entry is declared
    doc = src[src.index("findnz(A) / nziterator(A)"):src.index("int pa_mat_findnz")]
    for words in ("ascending (col lid, row lid)", "ascending (row lid, col lid)", "Deviation", "exactly once"):
        assert words in doc, words


def test_library_exports_and_binding_matches(pamd):
    L = pamd._lib.lib()
    protos = _prototypes()
    for e in ENTRIES:
        assert hasattr(L, e), e
        assert e in pamd._lib.EXPORTED
        assert len(pamd._lib._SIGS[e]) == len(protos[e]), e
    for name, value in CONSTANTS.items():
        assert getattr(pamd._lib, name) == value, name
    for name in ("findnz", "to_gids_", "to_main", "gather", "scatter_", "solve", "lu", "lu_", "ldiv_", "zerox", "PLU"):
        assert hasattr(pamd, name), name
    # gather keeps its PData form
    parts = pamd.sequential.get_part_ids(3)
    assert pamd.gather(pamd.map_parts(lambda p: 10 * p, parts)).parts[0] == [10, 20, 30]


def test_julia_binding_reaches_the_entries():
    jl = open(os.path.join(ROOT, "julia", "HIPBackend.jl")).read()
    for e in ENTRIES:
        assert f"(:{e}, libpa)" in jl, e


def test_bad_arguments_are_errors_with_a_message(pamd):
    L = pamd._lib.lib()
    out = ctypes.c_void_p(0)
    ids = (ctypes.c_int64 * 3)(1, 2, 3)

    def err():
        return L.pa_last_error()

    # null handles (every scalar argument valid)
    for rows_kind in (0, 1):
        for ids_kind in (0, 1):
            assert L.pa_mat_findnz(None, None, None, rows_kind, ids_kind, ctypes.byref(out)) != 0 and b"null" in err()
    # a bad which_rows / ids_kind is named, whatever the handles
    for bad in (-1, 2, 7):
        assert L.pa_mat_findnz(None, None, None, bad, 0, ctypes.byref(out)) != 0 and b"which_rows" in err()
        assert L.pa_mat_findnz(None, None, None, 0, bad, ctypes.byref(out)) != 0 and b"ids_kind" in err()
    assert out.value in (None, 0)  # nothing was handed out
    assert L.pa_index_to_gids(None, 3, ids) != 0 and b"null" in err()
    assert list(ids) == [1, 2, 3]  # and nothing was written
