"""Fixed-pattern re-assembly on one part: the Q1-hex element
triplets of an n^3-node grid (FE27 pattern, 64 triplets per cell, global ids)
written into an existing matrix.

--mode feature: fillstored_(A, 0) + add_coo_(A, I, J, V) on the device, from
  host arrays and from device-resident arrays; the one-time cost and the size
  of the entry table; one mul_ for scale; fillstored_ alone (fill + refresh)
  and a pa_vec_scatter of as many entries over as many values (sort + fold
  alone), to see where the time goes.
--mode baseline: the two routes that need no entry views — (a) building the
  matrix again with PSparseMatrix.from_coo, (b) get_values, the in-order fold
  on the host (np.add.at over nz positions computed beforehand, not timed),
  set_values.  PA_HIP_LIB selects the library (e.g. the parent commit's).

Host clocks around work that ends in a device synchronise; medians.  Every
route's nonzeros are compared bit for bit with those of the matrix built from
the same triplets.  One JSON line."""
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
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--mode", choices=("feature", "baseline"), default="feature")
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

n = a.n
be = pamd.HIPBackend(devices=[0])
parts = be.get_part_ids(1)
ctx = be.context(1)
rows = pamd.prange_linear(parts, n ** 3)
mk = lambda t: pamd.PData(parts.backend, [1], [t], parts.shape)

# element triplets: cell c's 8 nodes x 8 nodes, values Ke (the same for every cell)
c = np.arange((n - 1) ** 3, dtype=np.int64)
base = 1 + c % (n - 1) + n * (c // (n - 1) % (n - 1) + n * (c // (n - 1) ** 2))
off = np.array([dx + n * (dy + n * dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], dtype=np.int64)
nodes = base[:, None] + off[None, :]
I = np.repeat(nodes, 8, axis=1).ravel()
J = np.tile(nodes, (1, 8)).ravel()
V = np.tile(pamd.drivers.q1_hex_ke(2.0 / (n - 1)).ravel(), len(c))
del c, base, nodes
nt = len(I)


def timed(f, reps):
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ts)), 3), [round(t, 3) for t in ts]


def build():
    return pamd.PSparseMatrix.from_coo(mk(I), mk(J), mk(V), rows, rows, ids="global")


t0 = time.perf_counter()
A = build()
ctx.sync()
M = A.values.local(1)
built = M.get_values()
out = {"mode": a.mode, "workload": f"Q1-hex element triplets, {n}^3 nodes, one part, Float64, global ids",
       "library": os.environ.get("PA_HIP_LIB", "in-tree"), "triplets": nt, "stored_entries": len(built),
       "first_build_ms": round(1e3 * (time.perf_counter() - t0), 1)}
same = lambda v: bool(np.array_equal(v.view(np.uint64), built.view(np.uint64)))

if a.mode == "baseline":
    out["rebuild_from_coo_ms"], out["rebuild_all"] = timed(build, min(a.reps, 3))
    # nz position of each triplet in CSC order (sorted by column, then row): setup, not timed
    _, p = np.unique((J - 1) * n ** 3 + (I - 1), return_inverse=True)

    def host_route():
        nz = M.get_values()
        nz[:] = 0
        np.add.at(nz, p, V)
        M.set_values(nz)
    out["host_get_fold_set_ms"], out["host_all"] = timed(host_route, min(a.reps, 3))
    out["host_route_bits_equal"] = same(M.get_values())
else:
    x = pamd.PVector.full(1.0, rows)
    y = pamd.PVector.undef(rows)
    for _ in range(3):
        pamd.mul_(y, A, x)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(20):
        pamd.mul_(y, A, x)
    ctx.sync()
    out["mul_ms"] = round(1e3 * (time.perf_counter() - t0) / 20, 4)
    view = pamd.global_view(A, rows, rows).parts[0]
    assert M.entry_table() == (0, 0)
    out["table_build_ms"], _ = timed(lambda: view.get([1], [1]), 1)  # the first view call builds the table
    out["lookup_of_one_entry_ms"], _ = timed(lambda: view.get([1], [1]), 3)
    entries, nbytes = M.entry_table()
    out.update(table_entries=entries, table_bytes=nbytes, table_bytes_per_stored_entry=nbytes / max(entries, 1))

    def reassemble_host():
        pamd.fillstored_(A, 0)
        pamd.add_coo_(A, mk(I), mk(J), mk(V), ids="global")
    reassemble_host()  # warm-up
    out["reassemble_host_arrays_ms"], out["reassemble_host_all"] = timed(reassemble_host, a.reps)
    out["reassemble_host_arrays_bits_equal"] = same(M.get_values())

    def resident(v, dtype):
        d = pamd.device.DeviceVector(ctx, np.float64, len(v))
        d.upload(v.view(np.float64))
        return d.as_array(dtype)
    dI, dJ, dV = resident(I, np.int64), resident(J, np.int64), resident(V, np.float64)
    ridx = pamd.device.device_index_gids(ctx, rows.partition.local(1))

    def reassemble_device():
        pamd.fillstored_(A, 0)
        M.scatter(ridx, ridx, dI, dJ, dV, ids_global=True)
    reassemble_device()
    out["reassemble_device_arrays_ms"], out["reassemble_device_all"] = timed(reassemble_device, a.reps)
    out["reassemble_device_arrays_bits_equal"] = same(M.get_values())
    out["fillstored_alone_ms"], _ = timed(lambda: pamd.fillstored_(A, 0), a.reps)
    # sort + fold alone: as many entries over a vector of as many values, a like spread of duplicates
    nv = M.info()["slots"]
    w = pamd.device.DeviceVector(ctx, np.float64, nv)
    w.fill(0.0)
    widx = pamd.device.DeviceIndex(ctx, pamd.index_range(1, nv, 1))
    dP = resident(1 + ((I - 1) * 27 + J % 27) % nv, np.int64)
    w.scatter(widx, dP, dV)
    out["vec_scatter_same_size_ms"], _ = timed(lambda: w.scatter(widx, dP, dV), a.reps)
print(json.dumps(out), flush=True)
