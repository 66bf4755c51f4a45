"""The built matrix layout, pinned: every count DeviceMatrix.info() returns,
the traffic under spmv_format 0 and the SHA-256 of nonzeros(A), per part,
for the smallest inputs at which each structure of pa_mat exists, against
tests/golden/layout_fingerprint.json.

The fixture is written by this file:

    PA_HIP_LIB=<libpa_hip.so of the commit to pin> python tests/test_gpu_layout.py <that commit's hash>

and its header names the commit whose library produced it.  A change of the
build path (pa_api.cpp) that is meant to keep the layout must leave this test
green without regenerating the fixture."""
import gc
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest

from matrix_cases import SEED, long_row_coo, tridiag, unsorted_csr, with_ghost_coo

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_fingerprint.json")
DTYPES = {"f64": np.float64, "f32": np.float32, "c128": np.complex128, "c64": np.complex64}
N_STENCIL = (12, 10, 9)
# One node more in y than the FD7 cases above: their first z-plane (120 rows)
# does not fill a 128-row slice, so every Float64 slice has 7 entries per row
# and the uniform layout (K = 7) streams what the pattern slices would.
# Here slice 0 holds Dirichlet rows only (1 entry per row against K = 7).
N_UNIFORM = (12, 11, 9)
N_VORONOI, P_VORONOI = (24, 22, 20), 8      # test_gpu_irregular.py's smallest
N_LONG = (20, 18, 16)                       # test_gpu_coo.py's test_long_rows_bitexact
# every structure the fixture must show in at least one case (else it pins nothing)
MUST_EXIST = ("pattern_slices", "side_rows", "delta16_slices", "triple_sell_slices", "tri_slices", "pair_slices",
              "long_rows")


def _pdata(pamd, parts, d):
    return pamd.PData(parts.backend, parts.part_ids, [d[p] for p in parts.part_ids], parts.shape)


def _stencil(pamd, be, kind, shape, dtype, N=N_STENCIL):
    return pamd.drivers.stencil_operator(be.get_part_ids(shape), N, kind, dtype)


def _fd7_triplets(pamd, be):
    parts = be.get_part_ids((2, 2, 1))
    rows, cols = pamd.drivers.stencil_partition(parts, N_STENCIL, 7)
    I, J, V = {}, {}, {}
    for p in parts.part_ids:
        s = rows.partition.local(p)
        own = s.lid_to_gid[s.oid_to_lid - 1]
        i, J[p], V[p] = pamd.drivers.stencil_entries(7, N_STENCIL, own)
        I[p] = own[i]
    return parts, rows, cols, I, J, V


def _fd7_via(pamd, be, how):
    parts, rows, cols, I, J, V = _fd7_triplets(pamd, be)
    if how == "csc":
        csc = {p: pamd.compresscoo(rows.partition.local(p).to_lids(I[p]), cols.partition.local(p).to_lids(J[p]), V[p],
                                   rows.partition.local(p).num_lids, cols.partition.local(p).num_lids)
               for p in parts.part_ids}
        return pamd.PSparseMatrix.from_csc(_pdata(pamd, parts, csc), rows, cols)
    if how == "dcoo":
        coo = pamd.COO.from_host(_pdata(pamd, parts, I), _pdata(pamd, parts, J), _pdata(pamd, parts, V), rows)
        return pamd.PSparseMatrix.from_coo(coo, None, None, rows, cols, ids="global")
    return pamd.PSparseMatrix.from_coo(_pdata(pamd, parts, I), _pdata(pamd, parts, J), _pdata(pamd, parts, V), rows,
                                       cols, ids="global")


def _voronoi(pamd, be, dtype):
    return pamd.drivers.irregular_problem(be.get_part_ids(P_VORONOI), N_VORONOI, 27, dtype)


def _long_rows(pamd, be, build):
    parts = be.get_part_ids((2, 2, 1))
    _, part = pamd.drivers.stencil_partition(parts, N_LONG, 27)
    rng = np.random.default_rng(23)
    coo = {p: long_row_coo(rng, part, p, np.float64, [600, 1000, 4000, 70]) for p in parts.part_ids}
    mk = lambda k: _pdata(pamd, parts, {p: coo[p][k] for p in parts.part_ids})
    if build == "coo":
        return pamd.PSparseMatrix.from_coo(mk(0), mk(1), mk(2), part, part, ids="local")
    csc = pamd.map_parts(lambda i, j, v, s: pamd.compresscoo(i, j, v, s.num_lids, s.num_lids), mk(0), mk(1), mk(2),
                         part.partition)
    return pamd.PSparseMatrix.from_csc(csc, part, part)


def _unsorted(pamd, be):
    n = 390
    rowptr, colval, V, _, _, _ = unsorted_csr(n, (-1, 0, 1), 0, "diag_first", np.float64)
    parts = be.get_part_ids(1)
    rows = pamd.prange_linear(parts, n)
    return pamd.PSparseMatrix.from_csr(_pdata(pamd, parts, {1: pamd.CSR(0, n, n, rowptr, colval, V)}), rows, rows)


def _with_ghost(pamd, be):
    shape, ngids, periodic = (2, 2, 1), (16, 14, 6), (True, False, True)
    parts = be.get_part_ids(shape)
    rows = pamd.prange_cartesian(parts, ngids, with_ghost=True, isperiodic=periodic)
    I, J, V = with_ghost_coo(rows, parts, ngids, periodic, np.random.default_rng(SEED))
    return pamd.PSparseMatrix.from_coo(_pdata(pamd, parts, I), _pdata(pamd, parts, J), _pdata(pamd, parts, V), rows,
                                       rows, ids="global")


def _tiny_parts(pamd, be):
    """3 rows over 4 parts: three 1-row parts and an empty one"""
    n, parts = 3, be.get_part_ids(4)
    rows = pamd.prange_linear(parts, n)
    coo = {p: tridiag(n, rows.partition.local(p).lid_to_gid[rows.partition.local(p).oid_to_lid - 1])
           for p in parts.part_ids}
    mk = lambda k: _pdata(pamd, parts, {p: coo[p][k] for p in parts.part_ids})
    cols = pamd.add_gids(rows, mk(1))
    return pamd.PSparseMatrix.from_coo(mk(0), mk(1), mk(2), rows, cols, ids="global")


CASES = {}
for _k, _name in ((7, "fd7"), (27, "fe27")):
    for _shape in ((1, 1, 1), (2, 2, 1)):
        for _d, _dt in DTYPES.items():
            CASES[f"stencil-{_name}-{'x'.join(map(str, _shape))}-{_d}"] = (
                lambda pamd, be, k=_k, shape=_shape, dt=_dt: _stencil(pamd, be, k, shape, dt))
CASES["stencil-fd7-1x1x1-f64-uniform"] = lambda pamd, be: _stencil(pamd, be, 7, (1, 1, 1), np.float64, N_UNIFORM)
for _how in ("csc", "coo", "dcoo"):
    CASES[f"fd7-from-{_how}"] = lambda pamd, be, how=_how: _fd7_via(pamd, be, how)
for _d, _dt in DTYPES.items():
    CASES[f"voronoi-{_d}"] = lambda pamd, be, dt=_dt: _voronoi(pamd, be, dt)
for _b in ("coo", "csc"):
    CASES[f"long-rows-{_b}"] = lambda pamd, be, b=_b: _long_rows(pamd, be, b)
CASES["unsorted-csr"] = _unsorted
CASES["with-ghost-periodic"] = _with_ghost
CASES["tiny-parts"] = _tiny_parts


def fingerprint(pamd, A):
    """per part: info(), the traffic under spmv_format 0, sha256 of nonzeros(A)"""
    out = []
    for M in A.values.parts:
        f = {"info": M.info()}
        prev = pamd._lib.tune("spmv_format", 0)
        try:
            f["traffic_format0"] = M.traffic()
        finally:
            pamd._lib.tune("spmv_format", prev)
        has_nz = getattr(M, "csc_nnz", None) is not None  # (the stencil generator keeps no nz map)
        f["values_sha256"] = hashlib.sha256(M.get_values().tobytes()).hexdigest() if has_nz else None
        out.append(f)
    return out


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_fingerprint(be, pamd, golden, case):
    got = fingerprint(pamd, CASES[case](pamd, be))
    want = golden["cases"][case]
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case} part {p + 1}: " + str(
            {k: (g["info"].get(k), w["info"].get(k)) for k in set(g["info"]) | set(w["info"])
             if g["info"].get(k) != w["info"].get(k)})
    if case == "voronoi-f32":  # the f32_rows auto rebuild: 128-row slices (2 rows per lane)
        for g in got:
            assert g["info"]["nslices"] == math.ceil(g["info"]["nrows"] / 128)


def test_builders_agree(be, pamd):
    """the same FD7 matrix through from_csc, from_coo and from_dcoo: one layout"""
    a, b, c = (fingerprint(pamd, _fd7_via(pamd, be, how)) for how in ("csc", "coo", "dcoo"))
    assert a == b == c


def test_fixture_not_vacuous(be, pamd, golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    for key in MUST_EXIST:
        assert any(f["info"][key] > 0 for parts in golden["cases"].values() for f in parts), key
    vb = {}
    for u in (1, 0):
        prev = pamd._lib.tune("spmv_uniform", u)
        try:
            A = _stencil(pamd, be, 7, (1, 1, 1), np.float64, N_UNIFORM)
            vb[u] = A.values.local(1).traffic()["value_bytes"]
        finally:
            pamd._lib.tune("spmv_uniform", prev)
    assert vb[1] != vb[0], vb


def test_build_destroy_returns_device_memory(be, pamd):
    """200 builds and destroys of one FD7 matrix leave the device's free
    memory where the first build/destroy left it, to within one 2 MiB
    granule (the size the HIP runtime's device allocator hands out and takes
    back memory in): pa_mat owns every array it allocates."""
    import torch
    granule = 2 << 20

    def cycle():
        A = _stencil(pamd, be, 7, (1, 1, 1), np.float64)
        for M in A.values.parts:
            assert M.info()["pattern_slices"] > 0
        del A, M

    def free_bytes():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    cycle()
    first = free_bytes()
    for _ in range(200):
        cycle()
    last = free_bytes()
    assert abs(last - first) <= granule, (first, last)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import pamd as _pamd
    _be = _pamd.HIPBackend(devices=[0])
    doc = {"header": {"generated_by": "python tests/test_gpu_layout.py <commit>",
                      "library_commit": sys.argv[1],
                      "library": "PA_HIP_LIB" if os.environ.get("PA_HIP_LIB") else "in-tree"},
           "cases": {k: fingerprint(_pamd, CASES[k](_pamd, _be)) for k in sorted(CASES)}}
    missing = [k for k in MUST_EXIST
               if not any(f["info"][k] > 0 for parts in doc["cases"].values() for f in parts)]
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(doc['cases'])} cases; structures missing: {missing or 'none'}")
