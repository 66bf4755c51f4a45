"""Static type check of the Julia binding (no Julia on this image): every
argument type of every `ccall` in julia/HIPBackend.jl against the C parameter
type of the prototype in include/pa_hip.h.  A width or pointee mismatch fails:

    Cint                        int
    Int32 / Int64 / Cdouble     int32_t / int64_t / double
    Ptr{X} / Ref{X}             X* for X = Int32, Int64, Cint, Cfloat, Cdouble,
                                UInt8 (char), UInt64 — const or not, `X a[k]` too
    Ptr{Cvoid}                  an opaque handle `pa_x*`, a function pointer
    Ptr{Ptr{Cvoid}}             an array of handles (`pa_x* const a[]`)
    Ref{Ptr{Cvoid}}             a `T**` out parameter (handles, void**)
    Ref{T} / Ptr{T} / Ptr{...}  `void*` / `const void*` (values of the element type)
    Ref{PaExpr}                 `const pa_expr*`
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = open(os.path.join(ROOT, "julia", "HIPBackend.jl")).read()
HDR = open(os.path.join(ROOT, "include", "pa_hip.h")).read()

C_SCALARS = {"int": "int", "int32_t": "int32", "int64_t": "int64", "double": "double", "float": "float",
             "char": "uint8", "unsigned char": "uint8", "uint64_t": "uint64", "void": "void"}
JL_SCALARS = {"Cint": "int", "Int32": "int32", "Int64": "int64", "Cdouble": "double", "Float64": "double",
              "Cfloat": "float", "Float32": "float", "UInt8": "uint8", "Cchar": "uint8", "UInt64": "uint64",
              "Cvoid": "void"}
JL_STRUCTS = {"PaExpr": "pa_expr"}


def c_param_kind(param, fn_types):
    """A C parameter declaration -> 'int', ... for scalars; ('ptr', pointee);
    ('handle',) for `pa_x*`; ('handles',) for `pa_x**` / `pa_x* const a[]` /
    `void**`; ('fn',) for a function pointer type."""
    p = re.sub(r"\bconst\b", " ", param)
    arr = "[" in p
    p = re.sub(r"\[[^\]]*\]", " ", p)
    stars = p.count("*") + (1 if arr else 0)
    p = p.replace("*", " ")
    words = p.split()
    assert words, param
    # the base type: the longest known prefix; what follows is the parameter's name
    if words[0] == "unsigned":
        base, rest = " ".join(words[:2]), words[2:]
    else:
        base, rest = words[0], words[1:]
    assert len(rest) <= 1, param
    if base in fn_types:
        assert stars == 0, param
        return ("fn",)
    if base.startswith("pa_") and base not in ("pa_expr",):
        assert stars in (1, 2), param
        return ("handle",) if stars == 1 else ("handles",)
    if base == "pa_expr":
        assert stars == 1, param
        return ("ptr", "pa_expr")
    kind = C_SCALARS[base]
    if stars == 0:
        assert kind != "void", param
        return kind
    if stars == 2:
        assert kind == "void", param
        return ("handles",)
    return ("ptr", kind)


def c_prototypes():
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    fn_types = set(re.findall(r"typedef\s+\w+\s*\(\s*\*\s*(\w+)\s*\)", hdr))
    protos = {}
    for m in re.finditer(r"\b(?:int|const char\*)\s+(pa_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.S):
        params = m.group(2).strip()
        plist = [] if params in ("", "void") else [" ".join(q.split()) for q in params.split(",")]
        protos[m.group(1)] = [c_param_kind(q, fn_types) for q in plist]
    return protos


def jl_type_kind(t):
    """A ccall argument type -> the same kinds; a pointee that is a type
    variable (Ref{T}) is 'any'."""
    t = t.strip()
    if t in JL_SCALARS and t != "Cvoid":
        return JL_SCALARS[t]
    if t == "Cstring":
        return ("ptr", "uint8")
    m = re.fullmatch(r"(Ptr|Ref)\{(.*)\}", t)
    assert m, f"unknown ccall type {t}"
    inner = m.group(2).strip()
    if inner == "Ptr{Cvoid}":
        return ("handles",)
    if inner == "Cvoid":
        return ("ptr", "void")
    if inner in JL_SCALARS:
        return ("ptr", JL_SCALARS[inner])
    if inner in JL_STRUCTS:
        return ("ptr", JL_STRUCTS[inner])
    assert re.fullmatch(r"[A-Z]\w*", inner), f"unknown pointee {inner}"
    return ("ptr", "any")


def compatible(jl, c):
    if isinstance(c, str) or isinstance(jl, str):
        return jl == c  # scalars: the same width and kind
    if c == ("handle",) or c == ("fn",):
        return jl == ("ptr", "void")
    if c == ("handles",):
        return jl == ("handles",)
    if c == ("ptr", "void"):  # values of the element type, index arrays of a width passed alongside
        return jl[0] == "ptr"
    return jl == c  # a typed pointer: the same pointee


def _strip_comments(src):
    return "\n".join(line if "#" not in line else line[:line.find("#")] for line in src.splitlines())


def _balanced(s, i):
    depth = 0
    for j in range(i, len(s)):
        depth += s[j] == "("
        depth -= s[j] == ")"
        if depth == 0:
            return j + 1
    raise ValueError("unbalanced")


def _split_top(s):
    parts, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur)
    return [p.strip() for p in parts]


def mismatches(julia_source, protos):
    """[(entry, argument number, Julia type, C kind)] over the ccalls of the source"""
    code = _strip_comments(julia_source)
    bad, seen = [], 0
    for m in re.finditer(r"ccall\(", code):
        start = m.end() - 1
        args = _split_top(code[start + 1:_balanced(code, start) - 1])
        name = re.match(r"\(:(\w+),\s*libpa\)", args[0]).group(1)
        ret, types = args[1], _split_top(args[2][1:-1])
        seen += 1
        if name == "pa_last_error":
            if ret != "Cstring":
                bad.append((name, 0, ret, "const char*"))
            continue
        if ret != "Cint":
            bad.append((name, 0, ret, "int"))
        cs = protos[name]
        if len(cs) != len(types):
            bad.append((name, -1, f"{len(types)} types", f"{len(cs)} parameters"))
            continue
        for k, (t, c) in enumerate(zip(types, cs), 1):
            if not compatible(jl_type_kind(t), c):
                bad.append((name, k, t, c))
    return bad, seen


def test_header_parameter_kinds():
    P = c_prototypes()
    assert P["pa_ctx_create"] == ["int", "int", "int", ("handles",)]
    assert P["pa_vec_device_ptr"] == [("handle",), ("handles",)]
    assert P["pa_xchg_create"][:5] == [("handle",), "int32", ("ptr", "int32"), ("ptr", "int32"), ("ptr", "int32")]
    assert P["pa_exchange_all_async"] == ["int", ("handles",), ("handles",), ("handles",), "int", "int", "int",
                                          ("handles",), ("handles",)]
    assert P["pa_event_query"] == [("handle",), ("ptr", "int")]
    assert P["pa_comm_unique_id"] == [("ptr", "uint8")]
    assert P["pa_cg_solve_all"][9:12] == ["double", "double", "int64"]
    assert P["pa_cg_fuse_agree"] == ["int", ("fn",), ("ptr", "void"), ("ptr", "int")]


def test_every_ccall_argument_type_matches_its_c_parameter():
    bad, seen = mismatches(JL, c_prototypes())
    assert seen >= 25
    assert not bad, "\n".join(f"{n}: argument {k}: Julia {t}, C {c}" for n, k, t, c in bad)


def test_the_checker_rejects_wrong_types():
    P = c_prototypes()
    ok = "check(ccall((:pa_event_query, libpa), Cint, (Ptr{Cvoid}, Ref{Cint}), ev.h, d))"
    assert mismatches(ok, P) == ([], 1)
    wrong = {
        # a 64-bit out value for `int* done`
        "check(ccall((:pa_event_query, libpa), Cint, (Ptr{Cvoid}, Ref{Int64}), ev.h, d))":
            ("pa_event_query", 2, "Ref{Int64}"),
        # a 64-bit count for `int n`
        "ccall((:pa_exchange_all, libpa), Cint, (Int64, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, "
        "Cint, Cint), n, v, x, i, 0, 0, 0)": ("pa_exchange_all", 1, "Int64"),
        # one handle where the array of handles goes
        "ccall((:pa_exchange_all, libpa), Cint, (Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Cint, "
        "Cint, Cint), n, v, x, i, 0, 0, 0)": ("pa_exchange_all", 2, "Ptr{Cvoid}"),
        # Int32 ptrs into `const int64_t* k_rcv`
        "ccall((:pa_mat_xchg_create, libpa), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, "
        "Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ref{Ptr{Cvoid}}), A, 1, a, b, c, 1, d, e, f, out)":
            ("pa_mat_xchg_create", 5, "Ptr{Int32}"),
        # a double for `int64_t n`
        "ccall((:pa_vec_create, libpa), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ref{Ptr{Cvoid}}), c, 1, n, out)":
            ("pa_vec_create", 3, "Cdouble"),
    }
    for line, (name, k, t) in wrong.items():
        bad, seen = mismatches(line, P)
        assert seen == 1 and [(b[0], b[1], b[2]) for b in bad] == [(name, k, t)], (line, bad)
