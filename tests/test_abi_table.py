"""The table entries of the C-ABI (include/pa_hip.h: pa_table_*): declared,
exported, bound with the prototype's arity in _lib.py and reached by the
Julia binding, and failing loudly on null and bad arguments before anything
is allocated (no compute calls: CPU only)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pa_hip.h")

PROTOS = {
    "pa_table_create": ["pa_ctx* ctx", "int dtype", "int64_t nrows", "const int32_t* ptrs", "int ptrs_on_device",
                        "pa_table** out"],
    "pa_table_destroy": ["pa_table* t"],
    "pa_table_data": ["pa_table* t", "pa_vec** data"],
    "pa_table_info": ["const pa_table* t", "int64_t* nrows", "int64_t* ndata"],
    "pa_table_ptrs": ["const pa_table* t", "int32_t* ptrs"],
    "pa_table_exchange_all": ["int n", "pa_table* const tables[]", "pa_xchg* const xg[]", "int op", "int reverse",
                              "int zero_sent"],
    "pa_table_exchange_all_async": ["int n", "pa_table* const tables[]", "pa_xchg* const xg[]", "int op",
                                    "int reverse", "int zero_sent", "pa_event* const after[]", "pa_event* done[]"],
}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [" ".join(p.split()) for p in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(pa_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.S)}


def test_header_declares_the_entries():
    protos = _prototypes()
    for name, params in PROTOS.items():
        assert protos[name] == params, name
    # the exchange entries take op / reverse / a zero flag and the events exactly as their vector and matrix twins
    assert protos["pa_table_exchange_all"][3:] == protos["pa_mat_exchange_all"][3:]
    assert protos["pa_table_exchange_all_async"][3:] == protos["pa_mat_exchange_all_async"][3:]
    src = open(HEADER).read()
    assert re.search(r"typedef\s+struct\s+pa_table\s+pa_table\s*;", src)
    doc = src[src.index("---- tables"):src.index("int pa_table_create")]
    for words in ("Interfaces.jl:", "must be 1", "not decrease", "on the device", "one offset per neighbour",
                  "per base exchanger", "zero_sent", "fit Int32", "both parts and both counts", "before any allocation",
                  "the caller's contract", "must not be destroyed"):
        assert words in doc, words


def test_library_exports_and_binding_matches(pamd):
    L = pamd._lib.lib()
    protos = _prototypes()
    for e in PROTOS:
        assert hasattr(L, e), e
        assert e in pamd._lib.EXPORTED
        assert len(pamd._lib._SIGS[e]) == len(protos[e]), e
    for name in ("DeviceTable", "exchange_table_", "async_exchange_table_"):
        assert hasattr(pamd, name), name
    for name in ("from_host", "to_host", "upload", "download", "ptrs"):
        assert hasattr(pamd.DeviceTable, name), name


def test_julia_binding_reaches_the_entries():
    jl = open(os.path.join(ROOT, "julia", "HIPBackend.jl")).read()
    for e in PROTOS:
        assert f"(:{e}, libpa)" in jl, e
    assert re.search(r"function async_exchange!\(\s*combine_op,\s*values::HIPData\{<:Table\b", jl)


def test_documents_list_the_entries():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for e in PROTOS:
        assert e in integ, e
    assert "4.10" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_bad_arguments_are_errors_with_a_message(pamd):
    L = pamd._lib.lib()
    out = ctypes.c_void_p(0)
    ptrs = (ctypes.c_int32 * 3)(1, 2, 4)
    fake = ctypes.c_void_p(64)  # never dereferenced: every check below fails before the handle is used
    err = L.pa_last_error

    # create: null context / ptrs / out, bad dtype, negative rows, bad flag
    assert L.pa_table_create(None, 1, 2, ptrs, 0, ctypes.byref(out)) != 0 and b"null" in err()
    assert L.pa_table_create(fake, 1, 2, None, 0, ctypes.byref(out)) != 0 and b"null" in err()
    assert L.pa_table_create(fake, 1, 2, ptrs, 0, None) != 0 and b"null" in err()
    for bad in (-1, 4, 17):
        assert L.pa_table_create(fake, bad, 2, ptrs, 0, ctypes.byref(out)) != 0 and b"dtype" in err()
    assert L.pa_table_create(fake, 1, -1, ptrs, 0, ctypes.byref(out)) != 0 and b"rows" in err()
    assert L.pa_table_create(fake, 1, 2, ptrs, 2, ctypes.byref(out)) != 0 and b"ptrs_on_device" in err()
    # host ptrs are checked before the context is touched
    assert L.pa_table_create(fake, 1, 2, (ctypes.c_int32 * 3)(0, 2, 4), 0, ctypes.byref(out)) != 0
    assert b"ptrs[1] must be 1" in err()
    assert L.pa_table_create(fake, 1, 2, (ctypes.c_int32 * 3)(1, 5, 4), 0, ctypes.byref(out)) != 0
    assert b"must not decrease" in err()
    assert out.value in (None, 0)  # nothing was handed out

    n, m = ctypes.c_int64(-7), ctypes.c_int64(-7)
    assert L.pa_table_info(None, ctypes.byref(n), ctypes.byref(m)) != 0 and b"null" in err()
    assert (n.value, m.value) == (-7, -7)
    assert L.pa_table_data(None, ctypes.byref(out)) != 0 and b"null" in err()
    assert L.pa_table_ptrs(None, ptrs) != 0 and b"null" in err()
    assert list(ptrs) == [1, 2, 4]
    assert L.pa_table_destroy(None) == 0  # as the other destroys

    # exchange: null arrays, null handles inside them, a bad op, no `done`
    one = (ctypes.c_void_p * 1)(None)
    done = (ctypes.c_void_p * 1)(None)
    assert L.pa_table_exchange_all(1, None, None, 0, 0, 0) != 0 and b"null" in err()
    assert L.pa_table_exchange_all(0, one, one, 0, 0, 0) != 0 and b"null" in err()
    assert L.pa_table_exchange_all(1, one, one, 0, 0, 0) != 0 and b"null handle" in err()
    assert L.pa_table_exchange_all(1, one, one, 5, 0, 0) != 0 and b"combine op" in err()
    assert L.pa_table_exchange_all_async(1, one, one, 0, 0, 0, None, None) != 0 and b"null done" in err()
    assert L.pa_table_exchange_all_async(1, one, one, 0, 0, 0, None, done) != 0 and b"null handle" in err()
    assert done[0] in (None, 0)  # a failed call leaves no handle
