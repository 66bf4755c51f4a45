"""Jacobi-preconditioned CG per iteration, host-driven against device-driven
(DESIGN.md 4.11): whole solves with reltol = 0 and a fixed maxiter, timed by
the host clock around work that ends in a device synchronise, so the figure
holds what a solve pays: the host's per-call cost, every read-back, the set-up
SpMV and norms.

Loops, all from the same x0 = 0 on the same operator, right-hand side and
Jacobi(A):
  host_pcg      cg_(…, Pl=P, fused=True): xpby_, mul_dot_, pa_pcg_update_all,
                two read-backs per iteration
  dev_pcg_b8    cg_device_(…, Pl=P, batch=8)   (pa_pcg_solve_all)
  dev_pcg_b16   cg_device_(…, Pl=P, batch=16)
  dev_cg_b16    cg_device_(…, batch=16) without Pl (pa_cg_solve_all)

Cases: FE27 at 128^3 on one part in Float64 and Float32 (4.11's case), and
FE27 at 64^3 on (2,2,2) parts of the one GPU in Float64, where the host's
issue cost sets the iteration time.

Protocol: 10 warm-up iterations per loop, then --rounds (at least 9) rounds
alternating the loops, --iters iterations per solve; per loop the median
[min, max] over the rounds of ms per iteration.  The device loops' x and
history are compared with the host loop's bit for bit before anything is
timed.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pamd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--n1", type=int, default=128, help="grid edge of the one-part cases")
ap.add_argument("--n8", type=int, default=64, help="grid edge of the (2,2,2) case")
a = ap.parse_args()
if a.rounds < 9:
    ap.error("--rounds: at least 9")
if pamd.device_count() == 0:
    sys.exit("pcg_bench: no HIP device visible (this is a GPU measurement; nothing is timed without one)")

be = pamd.HIPBackend(devices=[0])
CASES = [("fe27_%d3_1part_f64" % a.n1, (1, 1, 1), a.n1, np.float64),
         ("fe27_%d3_1part_f32" % a.n1, (1, 1, 1), a.n1, np.float32),
         ("fe27_%d3_8parts_f64" % a.n8, (2, 2, 2), a.n8, np.float64)]


def sync(parts):
    for p in parts.part_ids:
        be.context(p).sync()


def run_case(shape, n, dtype):
    parts = be.get_part_ids(shape)
    A = pamd.drivers.stencil_operator(parts, (n,) * 3, 27, dtype)

    def rnd(s):
        return np.random.default_rng(31 + s.part).uniform(-1, 1, s.num_lids).astype(dtype)
    b = pamd.PVector.from_host(pamd.map_parts(rnd, A.cols.partition), A.cols)
    P = pamd.Jacobi(A)
    x0 = pamd.PVector.undef(A.cols, dtype).fill_(0)
    loops = {
        "host_pcg": lambda x, k, h: pamd.cg_(x, A, b, reltol=0.0, maxiter=k, history=h, fused=True, Pl=P),
        "dev_pcg_b8": lambda x, k, h: pamd.cg_device_(x, A, b, Pl=P, reltol=0.0, maxiter=k, history=h, batch=8),
        "dev_pcg_b16": lambda x, k, h: pamd.cg_device_(x, A, b, Pl=P, reltol=0.0, maxiter=k, history=h, batch=16),
        "dev_cg_b16": lambda x, k, h: pamd.cg_device_(x, A, b, reltol=0.0, maxiter=k, history=h, batch=16),
    }
    # warm-up: 10 iterations per loop; the preconditioned loops must agree bit for bit
    got = {}
    for name, f in loops.items():
        x, h = x0.copy(), []
        f(x, 10, h)
        sync(parts)
        got[name] = (h, x.to_host())
    for name in ("dev_pcg_b8", "dev_pcg_b16"):
        same = got[name][0] == got["host_pcg"][0] and all(
            np.array_equal(got[name][1].local(p), got["host_pcg"][1].local(p)) for p in parts.part_ids)
        if not same:
            sys.exit(f"pcg_bench: {name} differs from the host-driven loop: not timed")
    ms = {name: [] for name in loops}
    for _ in range(a.rounds):
        for name, f in loops.items():
            x = x0.copy()
            sync(parts)
            t0 = time.perf_counter()
            f(x, a.iters, None)
            sync(parts)
            ms[name].append(1e3 * (time.perf_counter() - t0) / a.iters)
    out = {"rows": len(A.rows), "parts": len(parts.part_ids), "dtype": np.dtype(dtype).name}
    for name, t in ms.items():
        out[name] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    host = out["host_pcg"]["median_ms"]
    for name in ("dev_pcg_b8", "dev_pcg_b16"):
        out[name]["over_host_pcg"] = round(out[name]["median_ms"] / host, 3)
    return out


res = {"tool": "pcg_bench", "rounds": a.rounds, "iterations_per_solve": a.iters, "warmup_iterations": 10,
       "figure": "ms per iteration, host clock over whole solves (reltol 0), median/min/max over the rounds",
       "cases": {}}
for name, shape, n, dtype in CASES:
    res["cases"][name] = run_case(shape, n, dtype)
print(json.dumps(res), flush=True)
