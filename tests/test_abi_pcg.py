"""The Jacobi-PCG entries of the C-ABI (include/pa_hip.h: pa_mat_diag,
pa_pcg_apply_all, pa_pcg_update_all): declared as specified, exported, bound
with the prototype's arity in _lib.py, listed in INTEGRATION.md and reached by
the Julia binding, and failing loudly on null arguments and complex element
types before anything is touched (no compute calls: CPU only)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pa_hip.h")

PROTOS = {
    "pa_mat_diag": ["const pa_mat* A", "const pa_index* rows", "const pa_index* cols", "pa_vec* d"],
    "pa_pcg_apply_all": ["int n", "pa_vec* const c[]", "const pa_vec* const r[]", "const pa_vec* const d[]",
                         "const pa_index* const idx[]", "void* rho"],
    "pa_pcg_update_all": ["int n", "pa_vec* const x[]", "pa_vec* const r[]", "const pa_vec* const u[]",
                          "pa_vec* const c[]", "const pa_vec* const d[]", "const pa_index* const idx[]",
                          "const void* alpha", "double* rnorm", "void* rho"],
}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): [" ".join(p.split()) for p in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(pa_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.S)}


def test_header_declares_the_entries():
    protos = _prototypes()
    for name, params in PROTOS.items():
        assert protos[name] == params, name
    src = open(HEADER).read()
    doc = src[src.index("---- Jacobi-preconditioned CG"):src.index("int pa_mat_diag")]
    for words in ("Float32 and Float64 only", "zero(T)", "Stored ghost rows are skipped", "+0.0", "delta16",
                  "long rows' CSR", "oid_to_lid", "plain stores", "pa_mat_entry_info is unchanged",
                  "compute stream", "after assemble!(A)", "fails with a message", "one IEEE division",
                  "OF THE ELEMENT TYPE", "no FMA", "block order", "part order"):
        assert words in doc, words


def test_library_exports_and_binding_matches(pamd):
    L = pamd._lib.lib()
    protos = _prototypes()
    for e in PROTOS:
        assert hasattr(L, e), e
        assert e in pamd._lib.EXPORTED
        assert len(pamd._lib._SIGS[e]) == len(protos[e]), e
    for name in ("diag", "Jacobi", "ldiv_", "cg_", "pcg_apply_", "pcg_update_"):
        assert hasattr(pamd, name), name
    import inspect
    sig = inspect.signature(pamd.cg_)
    assert sig.parameters["Pl"].default is None


def test_julia_binding_reaches_the_entries():
    jl = open(os.path.join(ROOT, "julia", "HIPBackend.jl")).read()
    for e in PROTOS:
        assert f"(:{e}, libpa)" in jl, e
    assert re.search(r"struct HIPJacobi", jl)
    assert re.search(r"function LinearAlgebra\.ldiv!\(c::HIPVector\{T\}, P::HIPJacobi", jl)
    assert re.search(r"function LinearAlgebra\.diag\(A::HIPMatrix\{T\}\)", jl)


def test_documents_list_the_entries():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for e in PROTOS:
        assert e in integ, e
    assert "HIPJacobi" in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.11" in design and "pa_mat_diag" in design


class _Vec(ctypes.Structure):
    """the head of the library's pa_vec (pa_internal.h): enough for the
    element-type check, which runs before any other field is read"""
    _fields_ = [("ctx", ctypes.c_void_p), ("dtype", ctypes.c_int), ("n", ctypes.c_int64), ("d", ctypes.c_void_p),
                ("base", ctypes.c_void_p)]


class _Mat(ctypes.Structure):
    """the head of pa_mat: its context and element type"""
    _fields_ = [("ctx", ctypes.c_void_p), ("dtype", ctypes.c_int), ("pad", ctypes.c_char * 240)]


def test_bad_arguments_are_errors_with_a_message(pamd):
    L = pamd._lib.lib()
    err = L.pa_last_error
    fake = ctypes.c_void_p(64)  # never dereferenced: every check below fails before the handle is used
    P = ctypes.c_void_p
    one_null = (P * 1)(None)
    one_fake = (P * 1)(64)
    rho = ctypes.c_double(-7.0)
    rn = ctypes.c_double(-7.0)
    alpha = ctypes.c_double(0.5)
    br = ctypes.byref

    # null arguments
    assert L.pa_mat_diag(None, fake, fake, fake) != 0 and b"null" in err()
    assert L.pa_mat_diag(fake, None, fake, fake) != 0 and b"null" in err()
    assert L.pa_mat_diag(fake, fake, None, fake) != 0 and b"null" in err()
    assert L.pa_mat_diag(fake, fake, fake, None) != 0 and b"null" in err()
    # null arrays, n < 1, no result
    assert L.pa_pcg_apply_all(1, None, one_fake, one_fake, one_fake, br(rho)) != 0 and b"null" in err()
    assert L.pa_pcg_apply_all(1, one_fake, None, one_fake, one_fake, br(rho)) != 0 and b"null" in err()
    assert L.pa_pcg_apply_all(1, one_fake, one_fake, None, one_fake, br(rho)) != 0 and b"null" in err()
    assert L.pa_pcg_apply_all(1, one_fake, one_fake, one_fake, None, br(rho)) != 0 and b"null" in err()
    assert L.pa_pcg_apply_all(1, one_fake, one_fake, one_fake, one_fake, None) != 0 and b"null" in err()
    assert L.pa_pcg_apply_all(0, one_fake, one_fake, one_fake, one_fake, br(rho)) != 0 and b"null" in err()
    for k in range(6):
        arrs = [one_fake] * 6
        arrs[k] = None
        assert L.pa_pcg_update_all(1, *arrs, br(alpha), br(rn), br(rho)) != 0 and b"null" in err(), k
    full = [one_fake] * 6
    assert L.pa_pcg_update_all(1, *full, None, br(rn), br(rho)) != 0 and b"null" in err()
    assert L.pa_pcg_update_all(1, *full, br(alpha), None, br(rho)) != 0 and b"null" in err()
    assert L.pa_pcg_update_all(1, *full, br(alpha), br(rn), None) != 0 and b"null" in err()
    # null handles inside the arrays
    for k in range(4):
        arrs = [one_fake] * 4
        arrs[k] = one_null
        assert L.pa_pcg_apply_all(1, *arrs, br(rho)) != 0 and b"null handle" in err(), k
    for k in range(6):
        arrs = [one_fake] * 6
        arrs[k] = one_null
        assert L.pa_pcg_update_all(1, *arrs, br(alpha), br(rn), br(rho)) != 0 and b"null handle" in err(), k

    # complex element types: refused on the first handle's dtype, nothing else is read
    for code in (pamd._lib.PA_C64, pamd._lib.PA_C128):
        v = _Vec(None, code, 3, None, None)
        m = _Mat(None, code)
        one_v = (P * 1)(ctypes.addressof(v))
        assert L.pa_mat_diag(br(m), fake, fake, fake) != 0 and b"complex" in err()
        assert L.pa_pcg_apply_all(1, one_v, one_fake, one_fake, one_fake, br(rho)) != 0 and b"complex" in err()
        assert L.pa_pcg_update_all(1, one_v, one_fake, one_fake, one_fake, one_fake, one_fake, br(alpha), br(rn),
                                   br(rho)) != 0 and b"complex" in err()
    assert (rho.value, rn.value) == (-7.0, -7.0)  # no result was written
