"""Reading a matrix's stored entries back as (I, J, V) on one part (DESIGN.md
4.9): the matrix 4.8 measured, the Q1-hex element triplets of an n^3-node grid
(FE27 pattern, global ids, Float64), about 56 M stored entries at n = 128.

--mode feature: (1) findnz(A, "owned", "global") alone, the COO staying on the
  device; (2) findnz + PSparseMatrix.from_coo of its result, the round trip,
  with the nonzeros of the rebuilt matrix compared bit for bit first; the
  bytes findnz allocates per stored entry; and, for scale, one A \\ b of the
  216-unknown FDM problem on 4 parts.
--mode baseline: the only route without findnz — get_values() and the host
  copy of the CSC pattern (kept from the build, not timed) expanded to (I, J)
  with numpy.  PA_HIP_LIB selects the library (e.g. the parent commit's).

Host clocks around work that ends in a device synchronise; medians after a
warm-up.  One JSON line."""
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
s = rows.partition.local(1)
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


def timed(f, reps):
    ts = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        f()
        ctx.sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ts)), 3), [round(t, 3) for t in ts]


out = {"mode": a.mode, "workload": f"Q1-hex element triplets, {n}^3 nodes, one part, Float64, global ids",
       "library": os.environ.get("PA_HIP_LIB", "in-tree"), "triplets": len(I)}

if a.mode == "baseline":
    idx = pamd.device.device_index_gids(ctx, s)
    M, colptr, rowval = pamd.DeviceMatrix.from_coo(ctx, I, J, V, idx, idx, s.num_lids, s.num_lids, ids_global=True,
                                                   pattern=True)
    del I, J, V
    out["stored_entries"] = len(rowval)

    def host_route():
        nz = M.get_values()
        gi = s.lid_to_gid[rowval - 1]
        gj = s.lid_to_gid[np.repeat(np.arange(s.num_lids), np.diff(colptr))]
        return gi, gj, nz
    host_route()  # warm-up
    out["get_values_and_host_pattern_ms"], out["host_all"] = timed(host_route, min(a.reps, 5))
    gi, gj, nz = host_route()
    out["entries_returned"] = len(nz)
else:
    A = pamd.PSparseMatrix.from_coo(mk(I), mk(J), mk(V), rows, rows, ids="global")
    del I, J, V
    ctx.sync()
    M = A.values.local(1)
    built = M.get_values()
    info = M.info()
    out.update(stored_entries=len(built), value_slots=info["slots"])
    keep = []

    def read_back():
        keep[:] = [pamd.findnz(A, "owned", "global")]
    out["first_findnz_ms"], _ = timed(read_back, 1)  # (no table is kept: the first call is a call like the others)
    out["findnz_ms"], out["findnz_all"] = timed(read_back, a.reps)
    assert M.entry_table() == (0, 0)
    ne = len(keep[0].values.local(1))
    out["entries_returned"] = ne
    # what one call allocates: key, flag and rank per value slot, then the compacted pairs and the
    # sort's second pair buffer per entry (plus rocprim's temporary storage), and the COO it returns
    out["bytes_per_entry"] = {"returned_coo": 24, "pairs_and_sort_buffers": 32,
                              "emit_pass": round(24 * info["slots"] / max(ne, 1), 2)}
    B = pamd.PSparseMatrix.from_coo(keep[0], None, None, rows, rows, ids="global")
    out["round_trip_bits_equal"] = bool(np.array_equal(B.values.local(1).get_values().view(np.uint64),
                                                       built.view(np.uint64)))
    del B

    def round_trip():
        keep[:] = [pamd.findnz(A, "owned", "global")]
        keep.append(pamd.PSparseMatrix.from_coo(keep[0], None, None, rows, rows, ids="global"))
    out["findnz_and_from_coo_ms"], out["round_trip_all"] = timed(round_trip, min(a.reps, 5))
    keep.clear()
    # for scale only: the direct solve is a debugging aid
    p4 = be.get_part_ids(4)
    F, b, _, _ = pamd.drivers.fdm_problem(p4, 6)
    pamd.solve(F, b)
    t0 = time.perf_counter()
    pamd.solve(F, b)
    out["solve_fdm_216_unknowns_4_parts_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
print(json.dumps(out), flush=True)
