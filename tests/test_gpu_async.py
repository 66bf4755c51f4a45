"""async_exchange_ / async_assemble_ on the device (pa_exchange_all_async,
pa_mat_exchange_all_async, pa_event): each call's work runs on its part's
comm stream and completes on its own.

No test blocks without a bound: _poll asks Task.done() against a deadline and
fails the test when it passes; the blocking Task.wait() is only called on
tasks that are already done."""
import math
import time

import numpy as np
import pytest

from matrix_cases import with_ghost_coo

pytestmark = pytest.mark.gpu

SEED = 20250114
DEADLINE = 30.0  # seconds


def _backend(pamd, **kw):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    return pamd.HIPBackend(devices=[0], **kw)


@pytest.fixture(scope="module")
def be(pamd):
    return _backend(pamd)


@pytest.fixture(scope="module")
def be_own(pamd):
    return _backend(pamd, share_streams=False)


@pytest.fixture(scope="module")
def be_rccl(pamd):
    return _backend(pamd, rccl=True)


@pytest.fixture
def backends(be, be_own, be_rccl):
    return {"shared": be, "own": be_own, "rccl": be_rccl}


def _poll(tasks, what="the tasks"):
    end = time.monotonic() + DEADLINE
    for t in tasks.parts:
        while not t.done():
            if time.monotonic() > end:
                pytest.fail(f"{what} did not complete within {DEADLINE:.0f} s")
    return tasks


def _finish(pamd, tasks, what="the tasks"):
    """poll until done, then the blocking wait (on finished tasks only)"""
    _poll(tasks, what)
    pamd.wait_all(tasks)
    assert all(t.done() for t in tasks.parts)


def _rand(rng, n, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(dtype)
    return rng.uniform(-1, 1, n).astype(dtype)


def _ox(O, a):
    return O.Cx(a.real.copy(), a.imag.copy()) if np.iscomplexobj(a) else a.copy()


def _eq(O, got, ref):
    if isinstance(ref, O.Cx):
        return np.array_equal(got.real, ref.re) and np.array_equal(got.imag, ref.im)
    return np.array_equal(got, ref)


def _tuned(pamd, **knobs):
    prev = {k: pamd._lib.tune(k, v) for k, v in knobs.items()}
    return lambda: [pamd._lib.tune(k, v) for k, v in prev.items()]


# ---- 1. parity ---------------------------------------------------------------
# name: (part shape or count, what builds the ranges)
CASES = {
    "cart222": ((2, 2, 2), ("stencil", (9, 8, 10))),
    "cart311": ((3, 1, 1), ("stencil", (40, 5, 4))),
    "single": ((1, 1, 1), ("stencil", (7, 6, 5))),                 # no neighbour
    "voronoi": (8, ("voronoi", (24, 22, 20))),                     # several senders combine into one lid
    "periodic": ((2, 2, 1), ("with_ghost", (16, 14, 6), (True, False, True))),  # interleaved lids
}
_ORANGE, _REF = {}, {}


def _range(pamd, parts, case):
    spec = CASES[case][1]
    if spec[0] == "stencil":
        return pamd.drivers.stencil_partition(parts, spec[1], 27)[1]
    if spec[0] == "voronoi":
        return pamd.drivers.irregular_partition(parts, spec[1], 27)[1]
    return pamd.prange_cartesian(parts, spec[1], with_ghost=True, isperiodic=spec[2])


def _oracle_range(O, case):
    if case not in _ORANGE:
        shape, spec = CASES[case]
        oparts = O.get_part_ids(shape)
        if spec[0] == "stencil":
            _ORANGE[case] = O.stencil_problem(oparts, spec[1], 27).cols
        elif spec[0] == "voronoi":
            _ORANGE[case] = O.irregular_problem(oparts, spec[1], 27).cols
        else:
            _ORANGE[case] = O.prange_cartesian(oparts, spec[1], with_ghost=True, isperiodic=spec[2])
    return _ORANGE[case]


def _reference(O, case, dtype):
    """the inputs (per part) and the oracle's exchange! / assemble! of them,
    computed once per case and element type"""
    key = (case, np.dtype(dtype).name)
    if key not in _REF:
        orng = _oracle_range(O, case)
        rng = np.random.default_rng(SEED + 7)
        vs = {s.part: _rand(rng, s.num_lids, dtype) for s in orng.partition.parts}
        ov = O.PVector(O.map_parts(lambda s: _ox(O, vs[s.part]), orng.partition), orng)
        ow = O.PVector(O.map_parts(lambda s: _ox(O, vs[s.part]), orng.partition), orng)
        O.exchange_pvector_(ov)
        O.assemble_(ow)
        _REF[key] = (vs, ov.values, ow.values)
    return _REF[key]


CONFIGS = [  # backend, halo_pull, halo_direct, dtype
    ("shared", 1, 1, np.float64), ("shared", 1, 1, np.float32), ("shared", 1, 1, np.complex64),
    ("shared", 1, 1, np.complex128), ("shared", 0, 1, np.float64), ("shared", 1, 0, np.float64),
    ("shared", 0, 0, np.float64), ("rccl", 1, 1, np.float64), ("own", 1, 1, np.float64), ("own", 0, 1, np.float64),
]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("backend,pull,direct,dtype", CONFIGS,
                         ids=[f"{b}-pull{p}-direct{d}-{np.dtype(t).name}" for b, p, d, t in CONFIGS])
def test_async_exchange_assemble_bitexact(backends, pamd, O, case, backend, pull, direct, dtype):
    restore = _tuned(pamd, halo_pull=pull, halo_direct=direct)
    try:
        parts = backends[backend].get_part_ids(CASES[case][0])
        rows = _range(pamd, parts, case)
        vs, ref_x, ref_a = _reference(O, case, dtype)
        v = pamd.PVector.from_host(pamd.map_parts(lambda s: vs[s.part], rows.partition), rows)
        w = pamd.PVector.from_host(pamd.map_parts(lambda s: vs[s.part], rows.partition), rows)
        tv = pamd.async_exchange_(v)
        tw = pamd.async_assemble_(w)
        assert len(tv.parts) == len(tw.parts) == len(parts.part_ids)
        _finish(pamd, tv, "async_exchange_")
        _finish(pamd, tw, "async_assemble_")
        gv, gw = v.to_host(), w.to_host()
        for p in parts.part_ids:
            assert _eq(O, gv.local(p), ref_x[p]), f"part {p}: async_exchange_ differs from exchange!"
            assert _eq(O, gw.local(p), ref_a[p]), f"part {p}: async_assemble_ differs from assemble!"
    finally:
        restore()


@pytest.mark.parametrize("nparts", [4, (2, 2)])
def test_async_matrix_exchange_assemble_bitexact(be, pamd, O, nparts):
    """async_assemble_(A) / async_exchange_(A) over nonzeros(A) on
    test_fem_sa's matrix, as test_fem_sa_matrix_exchange_assemble runs the
    blocking forms: bit-exact after each, and mul! with the assembled values
    (the side copies were refreshed by the async call)."""
    parts = be.get_part_ids(nparts)
    A, _, _, _ = pamd.drivers.fem_sa_problem(parts, 10)
    OA, _, _, _ = O.fem_sa_problem(O.get_part_ids(nparts), 10)
    rng = np.random.default_rng(11)
    for M, OM in zip(A.values.parts, OA.values.parts):  # ghost rows get values: both directions move data
        v = rng.uniform(-1, 1, len(OM.nzval))
        M.set_values(v)
        OM.nzval[:] = v
    _finish(pamd, pamd.async_assemble_(A), "async_assemble_(A)")
    O.assemble_matrix_(OA)
    for M, OM in zip(A.values.parts, OA.values.parts):
        assert np.array_equal(M.get_values(), OM.nzval)
    x = pamd.PVector.from_host(pamd.map_parts(lambda s: rng.uniform(-1, 1, s.num_lids), A.cols.partition), A.cols)
    ox = O.PVector(O.PData([a.copy() for a in x.to_host().parts], OA.cols.partition.shape), OA.cols)
    y, oy = pamd.PVector.undef(A.rows), O.pvector_undef(OA.rows)
    pamd.mul_(y, A, x)
    O.mul_(oy, OA, ox)
    for p in parts.part_ids:
        own = A.rows.partition.local(p).oid_to_lid - 1
        assert np.array_equal(y.to_host().local(p)[own], oy.values[p][own])
    _finish(pamd, pamd.async_exchange_(A), "async_exchange_(A)")
    O.exchange_matrix_(OA)
    for M, OM in zip(A.values.parts, OA.values.parts):
        assert np.array_equal(M.get_values(), OM.nzval)


# ---- 2. the call sees the writer before it --------------------------------------
def test_async_exchange_waits_for_the_compute_stream(be, pamd):
    """32 passes of v .= v .+ 1 over 2^22 owned values per part, then
    async_exchange_(v) at once: every ghost holds its owner's final value.  A
    pack that is not ordered behind the compute stream reads an earlier one."""
    parts = be.get_part_ids((2, 1, 1))
    N = (2048, 64, 64)
    rows = pamd.drivers.stencil_partition(parts, N, 7)[1]
    for s in rows.partition.parts:
        assert s.num_oids == 1 << 22 and s.num_hids > 0
    init = lambda s: np.where(s.lid_to_part == s.part, (s.lid_to_gid % 1024).astype(np.float64), -5.0)
    v = pamd.PVector.from_host(pamd.map_parts(init, rows.partition), rows)
    for _ in range(32):
        pamd.assign_(v, v + 1)
    t = pamd.async_exchange_(v)
    _finish(pamd, t, "async_exchange_")
    got = v.to_host()
    for p in parts.part_ids:
        s = rows.partition.local(p)
        assert np.array_equal(got.local(p), (s.lid_to_gid % 1024).astype(np.float64) + 32.0), f"part {p}"


# ---- 3. the call completes on its own ---------------------------------------------
W_PER_PART = 1 << 26  # Float32 values of w per part (raise it on a box that misses the precondition below)


def test_async_exchange_completes_before_queued_compute(be, pamd):
    """The exchange of a small v finishes while the compute stream still has K
    passes over a large unrelated w in its queue: its tasks are done when the
    event recorded behind the passes is not.  Tasks that drain the part's
    streams, or an exchange on the compute stream, fail the first assertion."""
    parts = be.get_part_ids((2, 1, 1))
    ctxs = [be.context(p) for p in parts.part_ids]
    sync = lambda: [c.sync() for c in ctxs]
    rows = pamd.drivers.stencil_partition(parts, (12, 10, 9), 27)[1]
    init = lambda s: np.where(s.lid_to_part == s.part, s.lid_to_gid.astype(np.float64), -1.0)
    v = pamd.PVector.from_host(pamd.map_parts(init, rows.partition), rows)
    w = pamd.PVector.full(np.float32(0), pamd.prange_linear(parts, 2 * W_PER_PART), np.float32)
    for s in w.rows.partition.parts:
        assert s.num_lids == W_PER_PART
    passes = 0
    # warm-up: pull tables, first launches; and 32 untimed passes, because for
    # some tens of ms after the 2^27-id range of w was built the host needs
    # ~1 ms to enqueue a pass (measured; 40 us afterwards)
    pamd.exchange_(v)
    for _ in range(32):
        pamd.assign_(w, w + 1)
    passes += 32
    sync()
    # te: a blocking exchange and the wait for it
    tes = []
    for _ in range(5):
        t0 = time.perf_counter()
        pamd.exchange_(v)
        sync()
        tes.append(time.perf_counter() - t0)
    te = sorted(tes)[2]
    # tp: device time of one pass over w (both parts; they share the stream pair); th: host time to enqueue one
    ctxs[0].span_start()
    t0 = time.perf_counter()
    for _ in range(32):
        pamd.assign_(w, w + 1)
    th = (time.perf_counter() - t0) / 32
    ctxs[0].span_stop()
    tp = ctxs[0].span_ms() * 1e-3 / 32
    passes += 32
    sync()
    K = max(64, math.ceil(100 * te / tp))
    print(f"\nte = {te * 1e6:.1f} us  tp = {tp * 1e6:.1f} us  th = {th * 1e6:.1f} us  K = {K}")
    assert tp >= 4 * th, "the host enqueues too slowly for the queue to build: raise W_PER_PART"
    # ghosts away again, so that the exchange below is seen to have happened
    for dv, s in zip(v.values.parts, rows.partition.parts):
        dv.upload(init(s))
    t = pamd.async_exchange_(v)
    for _ in range(K):
        pamd.assign_(w, w + 1)
    passes += K
    e = pamd.record(w)
    _poll(t, "async_exchange_")
    still_running = [not x.done() for x in e.parts]
    assert all(still_running), f"the exchange's tasks completed only with the queued passes: {still_running}"
    _finish(pamd, e, "the passes over w")
    pamd.wait_all(t)
    gv, gw = v.to_host(), w.to_host()
    for p in parts.part_ids:
        s = rows.partition.local(p)
        assert np.array_equal(gv.local(p), s.lid_to_gid.astype(np.float64)), f"part {p}: ghosts of v"
        a = gw.local(p)
        assert a.min() == a.max() == np.float32(passes), f"part {p}: w"


# ---- 4. chaining without the host ------------------------------------------------
@pytest.mark.parametrize("backend", ["shared", "own"])
def test_assemble_then_exchange_chained_by_t0(backends, pamd, O, backend):
    """t1 = async_assemble_(v); t2 = async_exchange_(v, t0=t1); wait(t2)
    (test_interfaces.jl:286-287) equals assemble! then exchange!."""
    case = "cart222"
    parts = backends[backend].get_part_ids(CASES[case][0])
    rows = _range(pamd, parts, case)
    vs, _, ref_a = _reference(O, case, np.float64)
    key = ("chain", case)
    if key not in _REF:
        orng = _oracle_range(O, case)
        ov = O.PVector(O.map_parts(lambda a: a.copy(), ref_a), orng)
        O.exchange_pvector_(ov)
        _REF[key] = ov.values
    v = pamd.PVector.from_host(pamd.map_parts(lambda s: vs[s.part], rows.partition), rows)
    t1 = pamd.async_assemble_(v)
    t2 = pamd.async_exchange_(v, t0=t1)
    _finish(pamd, t2, "async_exchange_(v, t0)")
    assert all(t.done() for t in t1.parts)  # t2 ran behind t1
    got = v.to_host()
    for p in parts.part_ids:
        assert np.array_equal(got.local(p), _REF[key][p]), f"part {p}"


def test_mul_then_exchange_chained_by_record(be, pamd, O):
    """record(y) after mul_(y, A, x) as the t0 of async_exchange_(y) equals
    mul! then exchange!(y) (rows with a ghost layer: y has ghosts)."""
    shape, ngids, periodic = (2, 2, 2), (12, 10, 9), None
    parts, oparts = be.get_part_ids(shape), O.get_part_ids(shape)
    rows = pamd.prange_cartesian(parts, ngids, with_ghost=True, isperiodic=periodic)
    orows = O.prange_cartesian(oparts, ngids, with_ghost=True, isperiodic=periodic)
    rng = np.random.default_rng(SEED)
    I, J, V = with_ghost_coo(rows, parts, ngids, periodic, rng)
    mk = lambda d: pamd.PData(parts.backend, parts.part_ids, [d[p] for p in parts.part_ids], parts.shape)
    A = pamd.PSparseMatrix.from_coo(mk(I), mk(J), mk(V), rows, rows, ids="global")
    omk = lambda d, f: O.PData([f(d[p]) for p in parts.part_ids], oparts.shape)
    OA = O.psparse_from_coo(omk(I, lambda a: [int(v) for v in a]), omk(J, lambda a: [int(v) for v in a]),
                            omk(V, lambda a: a.copy()), orows, orows, ids="global")
    xs = {p: rng.uniform(-1, 1, rows.partition.local(p).num_lids) for p in parts.part_ids}
    x = pamd.PVector.from_host(pamd.map_parts(lambda s: xs[s.part], rows.partition), rows)
    y = pamd.PVector.from_host(pamd.map_parts(lambda s: np.full(s.num_lids, 7.0), rows.partition), rows)
    ox = O.PVector(O.map_parts(lambda s: xs[s.part].copy(), orows.partition), orows)
    oy = O.PVector(O.map_parts(lambda s: np.full(s.num_lids, 7.0), orows.partition), orows)
    pamd.mul_(y, A, x)
    t = pamd.async_exchange_(y, t0=pamd.record(y))
    O.mul_(oy, OA, ox)
    O.exchange_pvector_(oy)
    _finish(pamd, t, "async_exchange_(y, t0=record(y))")
    got = y.to_host()
    for p in parts.part_ids:
        assert np.array_equal(got.local(p), oy.values[p]), f"part {p}"


# ---- 5. device-side join -----------------------------------------------------------
@pytest.mark.parametrize("backend", ["shared", "own"])
def test_join_orders_the_compute_stream_without_a_host_wait(backends, pamd, O, backend):
    case = "cart222"
    parts = backends[backend].get_part_ids(CASES[case][0])
    rows = _range(pamd, parts, case)
    vs, ref_x, _ = _reference(O, case, np.float64)
    v = pamd.PVector.from_host(pamd.map_parts(lambda s: vs[s.part], rows.partition), rows)
    w = pamd.PVector.undef(rows)
    t = pamd.async_exchange_(v)
    for x in t.parts:
        x.join()
    pamd.assign_(w, v + 0)  # all lids: w shares v's rows
    got = w.to_host()       # the download is in compute-stream order: no wait on t before it
    for p in parts.part_ids:
        assert np.array_equal(got.local(p), ref_x[p]), f"part {p}"
    _finish(pamd, t)


# ---- 6. one exchanger, several calls -------------------------------------------------
@pytest.mark.parametrize("barrier", [1, 0])
@pytest.mark.parametrize("backend", ["shared", "own"])
def test_calls_on_one_exchanger_back_to_back(backends, pamd, O, backend, barrier):
    """async_exchange_(a), async_exchange_(b) and a blocking mul_(y, A, x), all
    over A.cols' exchanger (its send and receive buffers), with no wait in
    between."""
    restore = _tuned(pamd, halo_barrier=barrier)
    try:
        shape, N = (2, 2, 1), (12, 10, 9)
        parts = backends[backend].get_part_ids(shape)
        A = pamd.drivers.stencil_operator(parts, N, 27)
        key = ("stencil", shape, N)
        if key not in _REF:
            OA = O.stencil_problem(O.get_part_ids(shape), N, 27)
            rng = np.random.default_rng(SEED + 9)
            ins = [{s.part: rng.uniform(-1, 1, s.num_lids) for s in OA.cols.partition.parts} for _ in range(3)]
            outs = []
            for d in ins:
                ov = O.PVector(O.map_parts(lambda s: d[s.part].copy(), OA.cols.partition), OA.cols)
                O.exchange_pvector_(ov)
                outs.append(ov.values)
            oy = O.pvector_undef(OA.rows)
            ox = O.PVector(O.map_parts(lambda s: ins[2][s.part].copy(), OA.cols.partition), OA.cols)
            O.mul_(oy, OA, ox)
            _REF[key] = (ins, outs, oy.values)
        ins, outs, ref_y = _REF[key]
        a, b, x = [pamd.PVector.from_host(pamd.map_parts(lambda s: d[s.part], A.cols.partition), A.cols) for d in ins]
        y = pamd.PVector.undef(A.rows)
        pamd.mul_(y, A, x)  # the exchanger's tables and, with halo_barrier, its chain exist before the async calls
        y.fill_(0.0)
        for dv, s in zip(x.values.parts, A.cols.partition.parts):
            dv.upload(ins[2][s.part])
        ta = pamd.async_exchange_(a)
        tb = pamd.async_exchange_(b)
        pamd.mul_(y, A, x)
        _finish(pamd, ta)
        _finish(pamd, tb)
        for got, ref in ((a.to_host(), outs[0]), (b.to_host(), outs[1]), (x.to_host(), outs[2]), (y.to_host(), ref_y)):
            for p in parts.part_ids:
                assert np.array_equal(got.local(p), ref[p]), f"part {p}"
    finally:
        restore()


# ---- 7. handles --------------------------------------------------------------------------
def test_task_handles(be_own, pamd, O):
    case = "cart222"
    parts = be_own.get_part_ids(CASES[case][0])
    rows = _range(pamd, parts, case)
    vs, ref_x, _ = _reference(O, case, np.float64)
    mk = lambda: pamd.PVector.from_host(pamd.map_parts(lambda s: vs[s.part], rows.partition), rows)
    v = mk()
    t = pamd.async_exchange_(v)
    assert all(isinstance(x, pamd.Task) for x in t.parts)
    _poll(t)
    for x in t.parts:
        x.wait()
        assert x.done()
        x.wait()  # waiting twice is fine
        assert x.done()
    # a task dropped before its work has finished: the next blocking exchange on the vector is exact
    u = mk()
    t = pamd.async_exchange_(u)
    del t
    pamd.exchange_(u)
    # a join across two contexts of one GPU: part 2's compute stream waits for part 1's task
    z = mk()
    t = pamd.async_exchange_(z)
    c2 = be_own.context(parts.part_ids[1])
    t.parts[0].join(c2)
    e = pamd.record(pamd.get_part_ids(parts))
    _finish(pamd, e, "the joined contexts")
    assert t.parts[0].done()  # part 2's compute stream ran behind it
    _finish(pamd, t)
    for w in (v, u, z):
        got = w.to_host()
        for p in parts.part_ids:
            assert np.array_equal(got.local(p), ref_x[p]), f"part {p}"


def test_coo_forms_return_finished_tasks(be, pamd):
    """async_assemble_ of a COO runs the blocking call (its outputs are sized
    on the host): the tasks it returns are done."""
    parts = be.get_part_ids((2, 2))
    rows, cols, I, J, V, _, _ = pamd.drivers.fem_sa_cells(parts, 4)
    coo = pamd.COO.from_host(I, J, V, rows)
    t = pamd.async_assemble_(coo, rows=rows)
    assert len(t.parts) == 4 and all(x.done() for x in t.parts)
    pamd.wait_all(t)
