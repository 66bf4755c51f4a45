"""The device-driven Jacobi-PCG entry of the C-ABI (include/pa_hip.h:
pa_pcg_solve_all): declared as specified, exported by the built library, bound
with the prototype's arity in _lib.py, reached by the Julia cg! method with
matching argument types, listed in the documents, and failing loudly on null
arguments, null handles, batch < 1 and complex element types before anything
is touched (no compute calls: CPU only)."""
import ctypes
import os
import re

from test_abi_pcg import HEADER, ROOT, _Mat, _prototypes
from test_julia_shim_types import _balanced, _split_top, _strip_comments, c_prototypes, mismatches

ENTRY = "pa_pcg_solve_all"
PARAMS = ["int n", "pa_mat* const A[]", "pa_vec* const x[]", "const pa_vec* const b[]", "const pa_vec* const d[]",
          "pa_vec* const u[]", "pa_vec* const r[]", "pa_vec* const c[]", "const pa_index* const idx[]",
          "pa_xchg* const xg[]", "double reltol", "double abstol", "int64_t maxiter", "int batch",
          "int64_t* iterations", "double* residual", "double* history"]


def test_header_declares_the_entry():
    protos = _prototypes()
    assert protos[ENTRY] == PARAMS
    # pa_cg_solve_all's arguments plus d, in fourth place
    assert [p for k, p in enumerate(PARAMS) if k != 4] == protos["pa_cg_solve_all"]
    src = open(HEADER).read()
    doc = src[src.index("IterativeSolvers.cg!(x, A, b; Pl = Diagonal(d)"):src.index("int " + ENTRY)]
    for words in ("Float32 and", "Float64 only", "bit for bit", "of the element", "batch < 1", "complex element type",
                  "not contiguous", "one part per process over RCCL", "its own sweep"):
        assert words in doc, words


def test_library_exports_and_binding_matches(pamd):
    L = pamd._lib.lib()
    assert hasattr(L, ENTRY)
    assert ENTRY in pamd._lib.EXPORTED
    assert len(pamd._lib._SIGS[ENTRY]) == len(PARAMS)
    # the binding's types: one count, nine handle arrays, the scalars as pa_cg_solve_all's
    assert pamd._lib._SIGS[ENTRY][:1] + pamd._lib._SIGS[ENTRY][2:] == pamd._lib._SIGS["pa_cg_solve_all"]
    import inspect
    sig = inspect.signature(pamd.cg_device_)
    assert list(sig.parameters) == ["x", "A", "b", "Pl", "reltol", "abstol", "maxiter", "history", "batch"]
    assert sig.parameters["Pl"].default is None and sig.parameters["batch"].default == 8
    assert sig.parameters["abstol"].default == 0.0
    for k in ("reltol", "maxiter", "history"):
        assert sig.parameters[k].default is None


def test_julia_cg_reaches_the_entry_with_matching_types():
    jl = open(os.path.join(ROOT, "julia", "HIPBackend.jl")).read()
    assert f"(:{ENTRY}, libpa)" in jl
    protos = c_prototypes()
    # the ccall of this entry alone, through the shim checker: argument count and types
    code = _strip_comments(jl)
    at = code.index(f"ccall((:{ENTRY}, libpa)")
    start = at + len("ccall")
    call = code[at:_balanced(code, start)]
    assert mismatches(call, protos) == ([], 1)
    types = _split_top(_split_top(call[len("ccall("):-1])[2][1:-1])
    assert len(types) == len(PARAMS)
    assert types[:10] == ["Cint"] + ["Ptr{Ptr{Cvoid}}"] * 9
    assert types[10:] == ["Float64", "Float64", "Int64", "Cint", "Ref{Int64}", "Ref{Float64}", "Ptr{Float64}"]
    # one argument short is a mismatch the checker reports
    short = call.replace("Ptr{Ptr{Cvoid}}, ", "", 1)
    bad, seen = mismatches(short, protos)
    assert seen == 1 and bad and bad[0][0] == ENTRY
    # the method sends only a HIPJacobi there, for real element types, without log or statevars
    body = jl[jl.index("function IterativeSolvers.cg!(x::HIPVector{T}"):]
    body = body[:body.index("\nend")]
    assert "Pl isa HIPJacobi" in body and "T <: PcgEltype" in body
    assert re.search(r"if log \|\| haskey\(kwargs, :statevars\) \|\| !\(Pl === nothing \|\| jacobi\)", body)
    assert body.index(ENTRY) < body.index("pa_cg_solve_all")


def test_documents_list_the_entry():
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert ENTRY in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for words in (ENTRY, "k_pcg_xu", "k_pcg_alpha", "k_pcg_step", "PCGState"):
        assert words in design, words
    assert "cg_device_" in open(os.path.join(ROOT, "README.md")).read()
    assert "pcg_bench.py" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_bad_arguments_are_errors_with_a_message(pamd):
    L = pamd._lib.lib()
    err = L.pa_last_error
    P = ctypes.c_void_p
    one_null = (P * 1)(None)
    one_fake = (P * 1)(64)  # never dereferenced: every check below fails before a handle is used
    its = ctypes.c_int64(-7)
    res = ctypes.c_double(-7.0)
    br = ctypes.byref

    def call(arrs, batch=8, its_p=br(its), res_p=br(res), n=1):
        return L.pa_pcg_solve_all(n, *arrs, ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int64(5), batch,
                                  its_p, res_p, None)

    full = [one_fake] * 9  # A, x, b, d, u, r, c, idx, xg
    # null arrays (xg may be null: no halo), n < 1, no place for the results
    for k in range(8):
        arrs = list(full)
        arrs[k] = None
        assert call(arrs) != 0 and b"null" in err(), k
    assert call(full, n=0) != 0 and b"null" in err()
    assert call(full, its_p=None) != 0 and b"null" in err()
    assert call(full, res_p=None) != 0 and b"null" in err()
    # batch < 1
    for batch in (0, -3):
        assert call(full, batch=batch) != 0 and b"batch must be >= 1" in err(), batch
    # null handles inside the arrays
    for k in range(8):
        arrs = list(full)
        arrs[k] = one_null
        assert call(arrs) != 0 and b"null handle" in err(), k
    # complex element types: refused on the matrix's dtype, nothing else is read
    for code in (pamd._lib.PA_C64, pamd._lib.PA_C128):
        m = _Mat(None, code)
        arrs = list(full)
        arrs[0] = (P * 1)(ctypes.addressof(m))
        assert call(arrs) != 0 and b"complex" in err() and b"pa_pcg_solve_all" in err()
    assert (its.value, res.value) == (-7, -7.0)  # no result was written
