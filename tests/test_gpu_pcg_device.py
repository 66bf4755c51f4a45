"""cg_device_(…, Pl=Jacobi) / pa_pcg_solve_all: the Jacobi-preconditioned CG
with its scalar recurrence on the device against the host-driven fused loop
cg_(…, Pl=P, fused=True) — x, the residual history and the iteration count
bit for bit.  That loop is pinned to the reference by test_gpu_pcg.py and
pcg_ref.py, so no tolerance appears here besides the reference's own 1e-5 on
the solution."""
import numpy as np
import pytest

import pcg_ref
from matrix_cases import SEED, with_ghost_coo
from pcg_ref import ERR_TOL
from test_gpu_drivers import _stencil_rhs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(pamd):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0])


def _host(pamd, A, b, x0, P, **kw):
    x, h = x0.copy(), []
    assert pamd.cg_(x, A, b, history=h, fused=True, Pl=P, **kw) is x
    return x, h


def _device(pamd, A, b, x0, P, batch, **kw):
    x, h = x0.copy(), []
    assert pamd.cg_device_(x, A, b, Pl=P, history=h, batch=batch, **kw) is x
    return x, h


def _same(parts, run1, run2):
    (x1, h1), (x2, h2) = run1, run2
    assert h1 == h2, (len(h1), len(h2), [(k, a, b) for k, (a, b) in enumerate(zip(h1, h2)) if a != b][:3])
    a, b = x1.to_host(), x2.to_host()
    for p in parts.part_ids:
        assert np.array_equal(a.local(p), b.local(p)), f"part {p}: x differs"


def _error(x, xh):
    return pcg_ref.owned_error(x.rows.partition.parts, x.to_host(), xh.to_host())


def _skewed_jacobi(pamd, A):
    """Jacobi of diag(A) times a factor running from 1 to 2 over the gids, the
    same on a ghost lid as on its owner: Pl \\ r is no uniform scaling of r"""
    n = len(A.cols)
    d = pamd.diag(A)
    vals = pamd.map_parts(lambda v, s: (v * (1.0 + (np.asarray(s.lid_to_gid, np.float64) - 1.0) / (n - 1.0)))
                          .astype(v.dtype), d.to_host(), A.cols.partition)
    return pamd.Jacobi(pamd.PVector.from_host(vals, A.cols))


# ---------------------------------------------------------------------------
# 1. bit for bit over exactly maxiter iterations

@pytest.mark.parametrize("shape,N,dtype,batch,maxiter", [
    ((2, 2, 1), (12, 10, 9), np.float64, 8, 40),    # 4 local parts: the gather kernel
    ((1, 1, 1), (9, 8, 7), np.float64, 3, 25),      # one part (no gather), batch not dividing maxiter
    ((2, 1, 1), (9, 9, 9), np.float32, 4, 20),      # Float32: the T-typed ρ, β and α
    ((2, 2, 2), (8, 8, 8), np.float32, 7, 20),
])
def test_device_pcg_equals_host_pcg(be, pamd, shape, N, dtype, batch, maxiter):
    parts = be.get_part_ids(shape)
    A = pamd.drivers.stencil_operator(parts, N, 27, dtype)
    b = _stencil_rhs(pamd, A, dtype, 31)
    P = _skewed_jacobi(pamd, A)
    x0 = pamd.PVector.undef(A.cols, dtype).fill_(0)
    kw = dict(reltol=0.0, maxiter=maxiter)
    host = _host(pamd, A, b, x0, P, **kw)
    dev = _device(pamd, A, b, x0, P, batch, **kw)
    print(f"{shape} {np.dtype(dtype).name}: residuals {host[1][0]:.6e} … {host[1][-1]:.6e}")
    assert len(host[1]) == len(dev[1]) == maxiter
    assert all(np.isfinite(host[1]))
    _same(parts, host, dev)


# ---------------------------------------------------------------------------
# 2. convergence in the middle of a batch (test_fdm.jl, default tolerances)

@pytest.fixture(scope="module")
def fdm10(be, pamd):
    """test_fdm.jl at nx = 10 per part shape: the problem and the host-driven
    fused loop's result, computed once.  Every call makes `shape` the
    backend's current partition again (its contexts are created once per
    number of parts), so a test may build further problems on `parts`."""
    cache = {}

    def get(shape):
        parts = be.get_part_ids(shape)
        if shape not in cache:
            A, b, x0, xh = pamd.drivers.fdm_problem(parts, 10)
            P = pamd.Jacobi(A)
            cache[shape] = (A, b, x0, xh, P, _host(pamd, A, b, x0, P))
        return (parts,) + cache[shape]
    return get


@pytest.mark.parametrize("shape,batch", [((2, 2, 2), 1), ((2, 2, 2), 4), ((2, 2, 2), 64), ((1, 1, 1), 5)])
def test_device_pcg_converges_like_the_host_loop(be, pamd, fdm10, shape, batch):
    parts, A, b, x0, xh, P, host = fdm10(shape)
    dev = _device(pamd, A, b, x0, P, batch)
    print(f"{shape} batch {batch}: {len(dev[1])} iterations")
    assert 0 < len(dev[1]) < 1000
    _same(parts, host, dev)
    assert _error(dev[0], xh) < ERR_TOL


# ---------------------------------------------------------------------------
# 3. the badly scaled system of test_gpu_pcg.py::test_pcg_scaled_system

def test_device_pcg_scaled_system(be, pamd):
    """b lies on A.rows, x on A.cols: b is copied onto x's range.  The host
    loop stops after the reference's 30 iterations (test_pcg_scaled_system)."""
    parts = be.get_part_ids((2, 2, 2))
    A, b, x0, xh = pcg_ref.scaled_device_fdm(pamd, parts, 10)
    P = pamd.Jacobi(A)
    host = _host(pamd, A, b, x0, P)
    dev = _device(pamd, A, b, x0, P, 8)
    assert len(dev[1]) == len(host[1]) == 30
    _same(parts, host, dev)
    assert _error(dev[0], xh) < ERR_TOL
    xc, hc = x0.copy(), []
    pamd.cg_device_(xc, A, b, history=hc)
    print(f"scaled fdm: device PCG {len(dev[1])} iterations, device CG {len(hc)}")
    assert len(dev[1]) < len(hc)


# ---------------------------------------------------------------------------
# 4. stored ghost rows (test_fem_sa.jl)

def test_device_pcg_fem_sa(be, pamd):
    parts = be.get_part_ids(4)
    A, b, x0, xh = pamd.drivers.fem_sa_problem(parts, 10)
    if not all(s.num_oids == 0 or (s.oid_to_lid[0] == 1 and s.oid_to_lid[-1] == s.num_oids)
               for s in A.cols.partition.parts):
        pytest.skip("fem_sa_problem's owned lids are not contiguous: the device recurrence refuses the range")
    P = pamd.Jacobi(A)
    host = _host(pamd, A, b, x0, P)
    dev = _device(pamd, A, b, x0, P, 8)
    assert len(dev[1]) > 0
    _same(parts, host, dev)
    assert _error(dev[0], xh) < ERR_TOL


# ---------------------------------------------------------------------------
# 5. the diagonal on another PRange

def test_device_pcg_diagonal_on_another_prange(be, pamd, fdm10):
    parts, A, b, x0, xh, P, host = fdm10((2, 2, 2))
    A2, _, _, _ = pamd.drivers.fdm_problem(parts, 10)
    P2 = pamd.Jacobi(A2)
    assert P2.d.rows is not x0.rows
    _same(parts, host, _device(pamd, A, b, x0, P2, 8))


# ---------------------------------------------------------------------------
# 6., 7. RCCL halos, and one part per process

def test_rccl_device_pcg_equals_device_reads(be, pamd):
    """every halo over RCCL (the parts of the device share one rank) == the
    device-read transport"""
    prev = pamd._lib.tune("halo_transport", 0)
    try:
        res = []
        for bk in (pamd.HIPBackend(devices=[0], rccl=True), be):
            parts = bk.get_part_ids((2, 2, 2))
            A, rhs, x0, _ = pamd.drivers.fdm_problem(parts, 12)
            res.append((parts, _device(pamd, A, rhs, x0, pamd.Jacobi(A), 8, reltol=0.0, maxiter=12)))
    finally:
        pamd._lib.tune("halo_transport", prev)
    (parts, r1), (_, r2) = res
    assert len(r1[1]) == 12
    _same(parts, r1, r2)


def test_one_part_per_process_device_pcg(be, pamd):
    """HIPDistributedBackend in a one-process world: the part values travel
    through ncclAllGather, and the result equals HIPBackend's direct read"""
    import socket
    import torch.distributed as dist
    own = not dist.is_initialized()
    if own:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        res = []
        for bk in (pamd.HIPDistributedBackend(device=0), be):
            parts = bk.get_part_ids(1)
            A, rhs, x0, _ = pamd.drivers.fdm_problem(parts, 14)
            P = pamd.Jacobi(A)
            kw = dict(reltol=0.0, maxiter=10)
            dev = _device(pamd, A, rhs, x0, P, 4, **kw)
            _same(parts, _host(pamd, A, rhs, x0, P, **kw), dev)
            res.append((parts, dev))
        (parts, r1), (_, r2) = res
        assert len(r1[1]) == 10
        _same(parts, r1, r2)
    finally:
        if own:
            dist.destroy_process_group()


# ---------------------------------------------------------------------------
# 8. degenerate solves

def test_no_iterations_leave_x_alone(be, pamd, fdm10):
    parts, A, b, x0, xh, P, host = fdm10((2, 2, 2))
    before = x0.to_host()
    for kw in (dict(maxiter=0), dict(reltol=0.0, abstol=1e300)):  # nothing allowed; x0 already within the tolerance
        x, h = _device(pamd, A, b, x0, P, 8, **kw)
        assert h == []
        for p in parts.part_ids:
            assert np.array_equal(x.to_host().local(p), before.local(p))


def test_empty_parts_device_pcg(be, pamd, O):
    """test_gpu_edges.py::test_empty_parts_cg's partition: 6 rows on 8 parts"""
    from test_gpu_edges import _build
    n, nparts = 6, 8
    parts = be.get_part_ids(nparts)
    A, _ = _build(pamd, O, parts, n, nparts)
    assert any(s.num_oids == 0 for s in A.rows.partition.parts)
    bh = {p: np.ones(A.cols.partition.local(p).num_lids) for p in parts.part_ids}
    b = pamd.PVector.from_host(pamd.map_parts(lambda s: bh[s.part], A.cols.partition), A.cols)
    x0 = pamd.PVector.undef(A.cols).fill_(0)
    P = pamd.Jacobi(A)
    host = _host(pamd, A, b, x0, P)
    dev = _device(pamd, A, b, x0, P, 2)
    assert len(dev[1]) > 0
    _same(parts, host, dev)


# ---------------------------------------------------------------------------
# 9. guards

def test_guards(be, pamd, fdm10):
    parts, A, b, x0, xh, P, host = fdm10((2, 2, 2))
    # cg_ keeps refusing device=True with a preconditioner, and names the new function
    with pytest.raises(NotImplementedError, match="cg_device_"):
        pamd.cg_(x0.copy(), A, b, Pl=P, device=True)
    # complex vectors
    Ac, bc, xc, _ = pamd.drivers.fdm_problem(parts, 10, np.complex128)
    with pytest.raises(NotImplementedError):
        pamd.cg_device_(xc.copy(), Ac, bc, Pl=P)
    # a Pl that is no Jacobi, or of another element type
    with pytest.raises(TypeError):
        pamd.cg_device_(x0.copy(), A, b, Pl=pamd.diag(A))
    A32, b32, x32, _ = pamd.drivers.fdm_problem(parts, 10, np.float32)
    with pytest.raises(TypeError):
        pamd.cg_device_(x32.copy(), A32, b32, Pl=P)
    # the entry itself refuses batch < 1 with a message
    with pytest.raises(pamd.PAError, match="batch must be >= 1"):
        pamd.cg_device_(x0.copy(), A, b, Pl=P, batch=0)
    # Pl=None is cg_(…, device=True), bit for bit
    x1, h1, x2, h2 = x0.copy(), [], x0.copy(), []
    pamd.cg_(x1, A, b, history=h1, device=True, batch=4)
    pamd.cg_device_(x2, A, b, history=h2, batch=4)
    assert len(h1) > 0
    _same(parts, (x1, h1), (x2, h2))


def test_interleaved_lids_are_refused(be, pamd):
    """PRange with ghosts and periodic dimensions (test_gpu_pcg.py::
    test_diag_interleaved_lids): owned and ghost lids interleave"""
    shape, ngids, periodic = (2, 2, 1), (16, 14, 6), (True, False, True)
    parts = be.get_part_ids(shape)
    rows = pamd.prange_cartesian(parts, ngids, with_ghost=True, isperiodic=periodic)
    assert any(s.oid_to_lid[-1] != s.num_oids for s in rows.partition.parts)
    I, J, V = with_ghost_coo(rows, parts, ngids, periodic, np.random.default_rng(SEED + 32))
    mk = lambda d: pamd.PData(parts.backend, parts.part_ids, [d[p].copy() for p in parts.part_ids], parts.shape)
    A = pamd.PSparseMatrix.from_coo(mk(I), mk(J), mk(V), rows, rows, ids="global")
    x = pamd.PVector.undef(rows).fill_(0)
    b = pamd.PVector.undef(rows).fill_(1)
    P = pamd.Jacobi(A)
    with pytest.raises(ValueError, match="contiguous"):
        pamd.cg_device_(x, A, b, Pl=P, maxiter=3)
    with pytest.raises(ValueError, match="contiguous"):
        pamd.cg_device_(x, A, b, maxiter=3)
    # the entry refuses the layout itself
    L, hs, ix = pamd._lib, pamd.pvector._hs, pamd.pvector._idx
    import ctypes as C
    w = [x.similar() for _ in range(3)]
    with pytest.raises(pamd.PAError, match="contiguous"):
        L.call("pa_pcg_solve_all", len(parts.part_ids), hs(A.values.parts), hs(x.values.parts), hs(b.values.parts),
               hs(P.d.values.parts), *[hs(v.values.parts) for v in w], L.ptr_array(ix(x)), None, 0.0, 0.0, 3, 8,
               C.byref(C.c_int64(0)), C.byref(C.c_double(0.0)), None)
