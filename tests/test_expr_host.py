"""Broadcast expressions, host side (no device): the encoder's postfix
programs (order, stack depth, scalar kinds, T/W tags), the rejections of the
Python layer and of pa_expr_check, and PVector's hashing left alone."""
import ctypes as C
import types

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L(pamd):
    return pamd._lib


def _vec(pamd, rows, dtype):
    """a PVector over `rows` without device values: the encoder only looks at
    the element type, the rows and the object's identity"""
    p = rows.partition
    stub = [types.SimpleNamespace(dtype=np.dtype(dtype)) for _ in p.parts]
    return pamd.PVector(pamd.PData(p.backend, p.part_ids, stub, p.shape), rows)


@pytest.fixture(scope="module")
def rows(pamd):
    return pamd.prange_linear(pamd.sequential.get_part_ids(2), 10)


def _check(pamd, P):
    """pa_expr_check on an encoded program → (depth, result flags)"""
    e, ns, _, kinds = P.c_args()
    depth, flags = C.c_int(-1), C.c_int(-1)
    pamd._lib.call("pa_expr_check", C.byref(e), pamd._lib.DTYPES[P.dtype], len(P.vecs), ns, kinds,
                   C.byref(depth), C.byref(flags))
    return depth.value, flags.value


def test_left_assoc_order_and_depth(pamd, L, rows):
    v, w, u = (_vec(pamd, rows, np.float64) for _ in range(3))
    P = pamd.encode_expr(v + w - u)
    assert [x is y for x, y in zip(P.vecs, (v, w, u))] == [True] * 3
    assert P.ops == [(L.OP_VEC, 0, 0), (L.OP_VEC, 1, 0), (L.OP_ADD, 0, L.EXPR_SS),
                     (L.OP_VEC, 2, 0), (L.OP_SUB, 0, L.EXPR_SS)]
    assert P.depth == 2
    assert _check(pamd, P) == (2, 0)


def test_deeper_subtree_first(pamd, L, rows):
    """a - (b - (c - (d - (e - f)))): operands in source order would need six
    slots; the deeper sibling first (reversed mode keeps left - right) needs two"""
    a, b, c, d, e, f = (_vec(pamd, rows, np.float32) for _ in range(6))
    P = pamd.encode_expr(a - (b - (c - (d - (e - f)))))
    assert P.depth == 2 <= L.EXPR_MAX_DEPTH
    assert [x is y for x, y in zip(P.vecs, (e, f, d, c, b, a))] == [True] * 6
    assert P.ops[:3] == [(L.OP_VEC, 0, 0), (L.OP_VEC, 1, 0), (L.OP_SUB, 0, L.EXPR_SS)]
    assert P.ops[3:] == [(L.OP_VEC, k, 0) if i % 2 == 0 else (L.OP_SUB, 0, L.EXPR_RS)
                         for k in range(2, 6) for i in range(2)]
    assert _check(pamd, P)[0] == 2
    # a balanced tree over 8 leaves needs all four slots and still fits
    vs = [_vec(pamd, rows, np.float32) for _ in range(8)]
    P = pamd.encode_expr(((vs[0] + vs[1]) * (vs[2] + vs[3])) - ((vs[4] + vs[5]) * (vs[6] + vs[7])))
    assert P.depth == 4 and _check(pamd, P)[0] == 4


@pytest.mark.parametrize("dtype,kinds", [(np.float32, (0, 1, 1)), (np.complex64, (3, 1, 2))])
def test_scalar_kinds(pamd, L, rows, dtype, kinds):
    """2 is of the element type next to real vectors and of its real type next
    to complex ones (kind 3: Julia's Real * Complex), 2.0 a Float64, 2.0 + 0j a
    Float64 into a real vector (no imaginary part) and a ComplexF64 into a
    complex one"""
    v = _vec(pamd, rows, dtype)
    for s, kind in zip((2, 2.0, 2.0 + 0j), kinds):
        P = pamd.encode_expr(s * v)
        assert [k for _, k in P.scalars] == [kind]
        wide = L.EXPR_WIDE if kind in (1, 2) else 0
        lreal = L.EXPR_LREAL if (kind in (1, 3) and np.dtype(dtype).kind == "c") else 0
        assert P.ops == [(L.OP_VEC, 0, 0), (L.OP_MUL, 0, L.EXPR_CS | wide | lreal)]
        real = np.zeros(1, dtype).real.dtype
        assert P.scalars[0][0].dtype == (np.dtype(dtype), np.float64, np.complex128, real)[kind]
        assert _check(pamd, P) == (1, wide)
    e, ns, buf, ck = pamd.encode_expr(2.0 * v - 3).c_args()
    assert ns == 2 and list(ck) == [1, kinds[0]]
    raw = bytes(buf)
    assert np.frombuffer(raw[:8], np.float64)[0] == 2.0
    assert np.frombuffer(raw[16:16 + real.itemsize], real)[0] == 3  # a Float32 in both cases
    # a complex scalar of the element type stays kind 0
    assert pamd.encode_expr(v + np.dtype(dtype).type(3)).scalars[0][1] == 0


def test_type_tags(pamd, L, rows):
    """(v + u) * 2.0 over Float32: the sum is a Float32 node, the product a
    Float64 node; with np.float32(2) both are Float32"""
    v, u = _vec(pamd, rows, np.float32), _vec(pamd, rows, np.float32)
    P = pamd.encode_expr((v + u) * 2.0)
    assert P.ops == [(L.OP_VEC, 0, 0), (L.OP_VEC, 1, 0), (L.OP_ADD, 0, L.EXPR_SS),
                     (L.OP_MUL, 0, L.EXPR_SC | L.EXPR_WIDE)]
    assert P.wide and _check(pamd, P) == (2, L.EXPR_WIDE)
    P = pamd.encode_expr((v + u) * np.float32(2))
    assert P.ops[-1] == (L.OP_MUL, 0, L.EXPR_SC) and not P.wide
    # a comparison's 1 / 0 is a Float32 node even against a Float64 scalar (Julia's Bool): the sum stays Float32
    P = pamd.encode_expr((v <= 0.25) + u)
    assert P.ops == [(L.OP_VEC, 0, 0), (L.OP_LE, 0, L.EXPR_SC | L.EXPR_WIDE), (L.OP_VEC, 1, 0), (L.OP_ADD, 0, L.EXPR_SS)]
    assert not P.wide and _check(pamd, P) == (2, 0)
    # complex vectors: abs2 is a real node, Float64 * complex is Real * Complex
    z = _vec(pamd, rows, np.complex64)
    P = pamd.encode_expr(pamd.abs2(z) * z - 0.5 * z)
    assert P.ops == [(L.OP_VEC, 0, 0), (L.OP_ABS2, 0, 0), (L.OP_VEC, 0, 0), (L.OP_MUL, 0, L.EXPR_SS | L.EXPR_LREAL),
                     (L.OP_VEC, 0, 0), (L.OP_MUL, 0, L.EXPR_CS | L.EXPR_WIDE | L.EXPR_LREAL),
                     (L.OP_SUB, 0, L.EXPR_SS | L.EXPR_WIDE)]
    assert _check(pamd, P) == (2, L.EXPR_WIDE)
    assert pamd.abs2(z).real and (pamd.eq(z, z)).real and not (z * z).real


def _alive(pamd):
    assert pamd._lib.lib().pa_version() == 1


def test_python_rejections(pamd, rows):
    v, u = _vec(pamd, rows, np.float32), _vec(pamd, rows, np.float32)
    with pytest.raises(TypeError, match="mixed element types"):
        v + _vec(pamd, rows, np.float64)
    with pytest.raises(TypeError, match="InexactError"):
        v * (1 + 2j)
    z = _vec(pamd, rows, np.complex128)
    with pytest.raises(TypeError, match="div of complex"):
        z / z
    with pytest.raises(TypeError, match="abs of complex"):
        abs(z)
    with pytest.raises(TypeError, match="ordered comparison"):
        z < 1.0
    with pytest.raises(TypeError):
        v + "x"
    e = v
    for _ in range(16):
        e = e + u  # 1 + 2 * 16 = 33 ops
    with pytest.raises(TypeError, match="more than 32"):
        pamd.encode_expr(e)
    t = v + u
    for _ in range(4):  # a full tree of the same leaves: needs 5 slots
        t = t * t
    with pytest.raises(TypeError, match="(stack slots|more than 32)"):
        pamd.encode_expr(t)
    d5 = (((v + u) * (v - u)) - ((u + v) * (u - v))) / (((v * u) + (v - u)) * ((u * v) - (u + v)))
    with pytest.raises(TypeError, match="stack slots"):
        pamd.encode_expr(d5)
    with pytest.raises(TypeError, match="comparison"):
        pamd.any_(v + u)
    _alive(pamd)


def _prog(pamd, ops):
    e = pamd._lib.Expr()
    e.nops = len(ops)
    for i, (c, a, f) in enumerate(ops[:pamd._lib.EXPR_MAX_OPS]):
        e.ops[i] = pamd._lib.ExprOp(c, a, f, 0)
    return e


def _c_check(pamd, ops, dtype, nvec=2, kinds=()):
    e = _prog(pamd, ops)
    ck = (C.c_int * max(1, len(kinds)))(*kinds)
    pamd._lib.call("pa_expr_check", C.byref(e), pamd._lib.DTYPES[np.dtype(dtype)], nvec, len(kinds), ck, None, None)


def test_library_rejections(pamd, L):
    """pa_expr_check (what pa_vec_eval / pa_reduce_expr_all run before any
    launch) refuses with a message and the library stays usable"""
    V0, V1 = (L.OP_VEC, 0, 0), (L.OP_VEC, 1, 0)
    _c_check(pamd, [V0, V1, (L.OP_ADD, 0, 0)], np.float64)  # a valid program passes
    bad = [
        ("32", [V0] + [(L.OP_NEG, 0, 0)] * 32, np.float64, ()),                      # 33 ops
        ("PA_EXPR_MAX_DEPTH", [V0, V1, V0, V1, V0], np.float64, ()),                 # five pushes
        ("underflow", [V0, (L.OP_ADD, 0, 0)], np.float64, ()),
        ("one value", [V0, V1], np.float64, ()),
        ("op code", [V0, (16, 0, 0)], np.float64, ()),
        ("out of range", [(L.OP_VEC, 2, 0)], np.float64, ()),
        ("out of range", [V0, (L.OP_MUL, 1, L.EXPR_SC)], np.float64, (0,)),
        ("complex division", [V0, V1, (L.OP_DIV, 0, 0)], np.complex128, ()),
        ("abs of a complex", [V0, (L.OP_ABS, 0, 0)], np.complex64, ()),
        ("ordered comparison", [V0, V1, (L.OP_LT, 0, 0)], np.complex64, ()),
        ("InexactError", [V0, (L.OP_MUL, 0, L.EXPR_SC | L.EXPR_WIDE)], np.float32, (2,)),
        ("type tags", [V0, (L.OP_MUL, 0, L.EXPR_SC)], np.float32, (1,)),             # a Float64 scalar needs WIDE
        ("type tags", [V0, V1, (L.OP_ADD, 0, L.EXPR_WIDE)], np.float32, ()),
        ("type tags", [V0, (L.OP_MUL, 0, L.EXPR_SC)], np.complex64, (3,)),           # a real(T) scalar needs RREAL
        ("scalar kind", [V0, (L.OP_MUL, 0, L.EXPR_SC)], np.float32, (4,)),
        ("empty", [], np.float64, ()),
    ]
    for msg, ops, dtype, kinds in bad:
        with pytest.raises(pamd.PAError, match=msg):
            _c_check(pamd, ops, dtype, kinds=kinds)
        _alive(pamd)
    with pytest.raises(pamd.PAError, match="null"):
        pamd._lib.call("pa_expr_check", None, 1, 0, 0, None, None, None)
    with pytest.raises(pamd.PAError, match="null"):
        pamd._lib.call("pa_vec_eval", None, None, None, 0, None, None, 0, None, None, 1)
    with pytest.raises(pamd.PAError, match="null"):
        pamd._lib.call("pa_reduce_expr_all", 1, 0, None, 1, None, None, 0, None, None, None)
    _alive(pamd)


def test_pvector_stays_hashable(pamd, rows):
    v, w = _vec(pamd, rows, np.float64), _vec(pamd, rows, np.float64)
    assert hash(v) == hash(v) and len({v, w}) == 2 and {v: 1}[v] == 1
    assert (v == w) is False and (v == v) is True and (v != w) is True  # identity, not a broadcast
    e = v + w
    assert isinstance(e, pamd.Broadcasted) and hash(e) == hash(e) and isinstance(v < w, pamd.Broadcasted)
    assert "__eq__" not in pamd.PVector.__dict__ and "__ne__" not in pamd.PVector.__dict__
    assert callable(pamd.isequal)
    assert isinstance(np.float32(2) * v, pamd.Broadcasted) and isinstance(2.0 - v, pamd.Broadcasted)
