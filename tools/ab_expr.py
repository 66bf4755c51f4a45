"""Interleaved A/B of the one-pass broadcast expressions (pa_vec_eval,
pa_reduce_expr_all) against the shortest chains of named entry points, in
one process, at the C-ABI (programs encoded and argument arrays built before
the timed loops, so the Python mirror's per-call work is not in the numbers):

    a  x .+= α.*u               pa_vec_eval          vs  pa_vec_axpby mode 1
    b  w .= v .+ α.*u .- β.*z   pa_vec_eval          vs  pa_vec_copy + axpby 1 + axpby 2
    c  sqeuclidean(a, b)        pa_reduce_expr_all   vs  pa_vec_copy + axpby 3 + pa_norm2_all

A repetition times one side on the device (pa_ctx_span events around
`--inner` back-to-back calls of that side, each on the next operand set, so
launch latency overlaps the previous kernel); the sides alternate, and the
operand sets rotate over enough copies that every call streams from HBM, not
the Infinity Cache.  Reports per case and side the median ms per call, the
spread (min, max, quartiles) and GB/s of the bytes that side actually
streams, next to the same run's pa_hbm_probe rates, and checks the sides
against each other: the same bits for a, and for b in Float64 (in Float32 the
chain rounds after every call, the one pass once: 1e-6), the reduction
tolerance for c.

    python tools/ab_expr.py --n 256 --dtype f64 --reps 30
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pamd  # noqa: E402
from pamd import _lib  # noqa: E402

DT = {"f64": np.float64, "f32": np.float32, "c128": np.complex128, "c64": np.complex64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256, help="owned values: n^3")
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--reps", type=int, default=30, help="repetitions per side (>= 20)")
    ap.add_argument("--inner", type=int, default=4, help="back-to-back calls per timed span")
    ap.add_argument("--rotate-bytes", type=float, default=1.5e9, help="bytes the rotating operand sets span")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    dtype = DT[a.dtype]
    S = np.dtype(dtype).itemsize
    N = a.n ** 3
    be = pamd.HIPBackend(devices=[0])
    parts = be.get_part_ids(1)
    rows = pamd.prange_linear(parts, N)
    ctx = be.context(1)
    rng = np.random.default_rng(7)
    nsets = max(a.inner, int(math.ceil(a.rotate_bytes / (5 * N * S))))

    def vec():
        h = rng.uniform(0.5, 1.5, N).astype(dtype)
        return pamd.PVector.from_host(pamd.map_parts(lambda s: h, rows.partition), rows, dtype)

    sets = [tuple(vec() for _ in range(5)) for _ in range(nsets)]  # (x, u, z, w, t) per set
    alpha, beta = 0.625, 0.375  # Float64 scalars, as IterativeSolvers' are
    wide = np.dtype(dtype) in (np.float32, np.complex64)
    idx = pamd.pvector._idx(sets[0][0])[0]
    h = lambda v: v.values.parts[0].h
    keep = []  # the ctypes buffers of the prebuilt calls

    def eval_call(y, expr):
        P = pamd.encode_expr(expr)
        e, ns, sbuf, kinds = P.c_args()
        vh, ih = _lib.ptr_array([h(v) for v in P.vecs]), _lib.ptr_array([idx] * len(P.vecs))
        keep.append((P, e, sbuf, kinds, vh, ih))
        return lambda: _lib.call("pa_vec_eval", h(y), idx, C.byref(e), len(P.vecs), vh, ih, ns, sbuf, kinds, 1)

    def axpby_call(y, x, s, mode):
        buf, bp = _lib.scalar_buf(s, np.float64 if mode < 3 else dtype)
        keep.append(buf)
        m = mode | (_lib.PA_BCAST_F64 if mode < 3 else 0)
        return lambda: _lib.call("pa_vec_axpby", h(y), h(x), idx, bp, m, 1)

    def copy_call(dst, src):
        return lambda: _lib.call("pa_vec_copy", h(dst), idx, h(src), idx, 1)

    def seq(*calls):
        def f():
            for c in calls:
                r = c()
            return r
        return f

    out64 = np.zeros(1, np.float64)
    outT = np.zeros(1, dtype)

    def reduce_call(expr):
        P = pamd.encode_expr(expr)
        e, ns, sbuf, kinds = P.c_args()
        vh, ih = _lib.ptr_array([h(v) for v in P.vecs]), _lib.ptr_array([idx] * len(P.vecs))
        keep.append((P, e, sbuf, kinds, vh, ih))

        def f():
            _lib.call("pa_reduce_expr_all", 1, _lib.REDUCE_SUM, C.byref(e), len(P.vecs), vh, ih, ns, sbuf, kinds,
                      outT.ctypes.data_as(C.c_void_p))
            return float(outT[0].real)
        return f

    def norm2_call(t):
        vh, ih = _lib.ptr_array([h(t)]), _lib.ptr_array([idx])
        keep.append((vh, ih))

        def f():
            _lib.call("pa_norm2_all", 1, vh, ih, out64.ctypes.data_as(C.c_void_p))
            return float(out64[0]) ** 2
        return f

    res = {}

    def run(case, nbytes, sides, same):
        """sides: {name: [one prebuilt call per operand set]}"""
        ms = {k: [] for k in sides}
        for k, calls in sides.items():  # warm-up: code objects, first touches
            for c in calls:
                c()
        ctx.sync()
        pos = 0
        for rep in range(a.reps):
            for k, calls in sides.items():
                ctx.span_start()
                for j in range(a.inner):
                    calls[(pos + j) % nsets]()
                ctx.span_stop()
                ms[k].append(ctx.span_ms() / a.inner)
            pos += a.inner
        res[case] = {"same": bool(same()), "sides": {}}
        for k in sides:
            m = np.sort(np.array(ms[k]))
            med = float(np.median(m))
            res[case]["sides"][k] = {
                "ms_median": round(med, 5), "ms_min": round(float(m[0]), 5), "ms_max": round(float(m[-1]), 5),
                "ms_q1": round(float(np.percentile(m, 25)), 5), "ms_q3": round(float(np.percentile(m, 75)), 5),
                "bytes": nbytes[k], "gbs": round(nbytes[k] / (med * 1e-3) / 1e9, 1)}

    def equal(p, q, exact):
        hp, hq = p.to_host().parts, q.to_host().parts
        if exact:
            return all(np.array_equal(s, t) for s, t in zip(hp, hq))
        return all(np.allclose(s, t, rtol=1e-6, atol=0) for s, t in zip(hp, hq))

    # a: x .+= α.*u
    def same_a():
        x, u, z, w, t = sets[0]
        copy_call(w, z)()
        copy_call(t, z)()
        eval_call(w, w + alpha * u)()
        axpby_call(t, u, alpha, 1)()
        return equal(w, t, True)

    run("a: x .+= alpha.*u", {"eval": 3 * N * S, "axpby": 3 * N * S},
        {"eval": [eval_call(x, x + alpha * u) for x, u, z, w, t in sets],
         "axpby": [axpby_call(x, u, alpha, 1) for x, u, z, w, t in sets]}, same_a)

    # b: w .= v .+ α.*u .- β.*z (v = the set's x)
    b_eval = [eval_call(w, x + alpha * u - beta * z) for x, u, z, w, t in sets]
    b_chain = [seq(copy_call(t, x), axpby_call(t, u, alpha, 1), axpby_call(t, z, beta, 2)) for x, u, z, w, t in sets]

    def same_b():
        b_eval[0]()
        b_chain[0]()
        return equal(sets[0][3], sets[0][4], not wide)

    run("b: w .= v .+ alpha.*u .- beta.*z", {"eval": 4 * N * S, "chain": 8 * N * S},
        {"eval": b_eval, "chain": b_chain}, same_b)

    # c: sqeuclidean(a, b) (a, b = the set's u, z)
    c_eval = [reduce_call(pamd.abs2(u - z)) for x, u, z, w, t in sets]
    c_chain = [seq(copy_call(t, u), axpby_call(t, z, 0, 3), norm2_call(t)) for x, u, z, w, t in sets]
    tol = 1e-12 if not wide else 1e-6

    def same_c():
        p, q = c_eval[0](), c_chain[0]()
        return abs(p - q) <= tol * abs(q)

    run("c: sqeuclidean(a, b)", {"eval": 2 * N * S, "chain": 6 * N * S}, {"eval": c_eval, "chain": c_chain}, same_c)

    read_gbs, copy_gbs = _lib.hbm_probe(0, 2 << 30, 10)
    print(json.dumps({"tool": "ab_expr", "label": a.label, "n": a.n, "owned": N, "dtype": a.dtype, "reps": a.reps,
                      "inner": a.inner, "operand_sets": nsets, "hbm_probe_read_gbs": round(read_gbs, 1),
                      "hbm_probe_copy_gbs": round(copy_gbs, 1), "cases": res}))


if __name__ == "__main__":
    main()
