"""pa_exchange_all, its async and matrix twins and the halo of mul! against
tests/exchange_ref.py, by bytes over every lid of every part: all eight
(op, reverse, zero_ghosts) combinations, the four element types, exchangers
that no PRange would build, and more slots than one grid-stride round covers.

The partition (tests/exchange_cases.py): three parts on device 0 with 41, 300
and 17 lids, the ghosts scattered among the owned lids, every ghost's gid
owned by the part lid_to_part names.  Parts 1 and 3 hold a third of their
lids as ghosts; part 2 holds all 38 gids the other two own (there are no more
to ghost).  The exchanger cases:

  ghost    exchanger_from_ids of the partition; its tables are read out for
           the reference;
  dup      edges 1→2 (70 slots), 2→1 (50), 2→3 (40), 1→3 (9) and a zero-length
           3→2 that both sides list, no 3→1; send lids drawn with replacement
           from all lids, receive lids with replacement from half the lids:
           duplicates across and inside segments, owned targets, ghost senders;
  forward  the same edges with unique receive lids (so with fewer slots: 50
           unique lids do not fit into part 1's 41 nor 49 into part 3's 17:
           70, 18, 5, 3, 0); every non-empty send segment names lids of the
           part's own receive list, owned ones among them;
  lonely   part 3 without lids and without neighbours, parts 1 and 2 as in dup;
  wide     two parts, one edge of 1,048,576 + 300 slots without repeats;
  wide_dup about 1.2 M slots onto 1,048,576 + 4096 distinct targets.

Values are ±u·2^k (u in [1, 2), k in -8..8) so that the order of a fold shows
in the bits: test_values_make_fold_order_visible asserts it per case and type
on the reference.  The edges above cap one exchange of dup at 84 targets with
several contributions (169 slots), so the 100 targets are counted over the
case's eight runs, each with its own values; the share that a descending fold
changes is taken over the ADD runs."""
import ctypes as C

import numpy as np
import pytest

import exchange_cases as X
import exchange_ref as R

pytestmark = pytest.mark.gpu

F64, C64 = np.float64, np.complex64
_DT = lambda d: np.dtype(d).name


def _differences(got, want, what):
    """compare by bytes; on a mismatch name the lids"""
    for p, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: part {p + 1} has another type or length"
        if g.tobytes() != w.tobytes():
            k = g.dtype.itemsize
            bad = np.flatnonzero((g.view(np.uint8).reshape(-1, k) != w.view(np.uint8).reshape(-1, k)).any(axis=1))
            show = ", ".join(f"lid {l + 1}: {g[l]!r} != {w[l]!r}" for l in bad[:4])
            pytest.fail(f"{what}: part {p + 1}: {len(bad)} of {len(g)} lids differ ({show})")


class World:
    """One backend's contexts with the cases' ranges, exchangers and vectors
    on them, each built once."""

    def __init__(self, pamd, backend, cases):
        self.pamd, self.backend, self.cases = pamd, backend, cases
        self._rows, self._vec, self._xg = {}, {}, {}

    def rows(self, name, exchanger="case"):
        """PRange(ngids, partition, Exchanger(case)); cases over one partition share its index sets"""
        pamd, c = self.pamd, self.cases[name]
        key = (id(c.lid_to_gid), exchanger if exchanger != "case" else name)
        if key not in self._rows:
            pk = ("partition", id(c.lid_to_gid))
            if pk not in self._rows:
                parts = self.backend.get_part_ids(c.nparts)
                sets = [pamd.IndexSet(p + 1, c.lid_to_gid[p], c.lid_to_part[p]) for p in range(c.nparts)]
                self._rows[pk] = pamd.PData(parts.backend, parts.part_ids, sets, parts.shape)
            part = self._rows[pk]
            mk = lambda xs: pamd.PData(part.backend, part.part_ids, list(xs), part.shape)
            if exchanger == "empty":
                ex = pamd.empty_exchanger(part)
            elif name == "ghost":
                ex = pamd.exchanger_from_ids(part)
            else:
                tab = lambda ts: mk([pamd.Table(d, p) for d, p in ts])
                ex = pamd.Exchanger(mk(c.parts_rcv), mk(c.parts_snd), tab(c.lids_rcv), tab(c.lids_snd))
            self._rows[key] = pamd.PRange(c.ngids, part, ex)
        return self._rows[key]

    def vector(self, name, dtype, exchanger="case", slot=0):
        key = (name, _DT(dtype), exchanger, slot)
        if key not in self._vec:
            self._vec[key] = self.pamd.PVector.undef(self.rows(name, exchanger), dtype)
        return self._vec[key]

    def exchangers(self, name):
        if name not in self._xg:
            rows = self.rows(name)
            ctxs = self.pamd.device.contexts(rows.partition)
            self._xg[name] = [self.pamd.device.device_exchanger(c, rows.exchanger, p)
                              for c, p in zip(ctxs, rows.partition.part_ids)]
        return self._xg[name]


@pytest.fixture(scope="module")
def cases():
    return X.small_cases()


@pytest.fixture(scope="module")
def worlds(pamd, cases):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    wide = {"wide": X.wide_case(False), "wide_dup": X.wide_case(True)}
    W = {"shared": World(pamd, pamd.HIPBackend(devices=[0], share_streams=True), {**cases, **wide}),
         "own": World(pamd, pamd.HIPBackend(devices=[0], share_streams=False), cases),
         "rccl": World(pamd, pamd.HIPBackend(devices=[0], rccl=True), cases)}
    # ghost: the exchanger the package derives from the index sets, read out for the reference
    ex = W["shared"].rows("ghost").exchanger
    c = cases["ghost"]
    tabs = lambda t: [(np.asarray(x.data, np.int32), np.asarray(x.ptrs, np.int32)) for x in t.parts]
    c.set_tables([np.asarray(p, np.int32) for p in ex.parts_rcv.parts], tabs(ex.lids_rcv),
                 [np.asarray(p, np.int32) for p in ex.parts_snd.parts], tabs(ex.lids_snd))
    for p in range(c.nparts):  # what a PRange builds: every ghost received once, owned lids sent
        assert sorted(c.lids_rcv[p][0].tolist()) == c.hids[p].tolist()
        assert not np.isin(c.lids_snd[p][0], c.hids[p]).any()
    return W


_REF = {}


def _reference(case, dtype, mode):
    """(start, expected) of a run, computed once and never written to"""
    key = (case.name, _DT(dtype), mode)
    if key not in _REF:
        start = X.start_values(case, dtype, mode)
        want = X.expected(case, start, mode)
        for a in start + want:
            a.setflags(write=False)
        _REF[key] = (start, want)
    return _REF[key]


def _tuned(pamd, **knobs):
    prev = {k: pamd._lib.tune(k, v) for k, v in knobs.items()}
    return lambda: [pamd._lib.tune(k, v) for k, v in prev.items()]


def _call_exchange(pamd, v, xg, mode, entry="pa_exchange_all"):
    op, reverse, zero = mode
    hs = pamd._lib.ptr_array
    n = len(xg)
    args = (n, hs([d.h for d in v.values.parts]), hs([x.h for x in xg]), hs(pamd.pvector._idx(v)),
            pamd._lib.PA_ADD if op == R.ADD else pamd._lib.PA_REPLACE, int(reverse), int(zero))
    if entry == "pa_exchange_all":
        pamd._lib.call(entry, *args)
        return
    done = (C.c_void_p * n)()
    pamd._lib.call(entry, *args, None, done)
    ctxs = pamd.device.contexts(v.values)
    for t in [pamd.Task(c, C.c_void_p(h)) for c, h in zip(ctxs, done)]:
        t.wait()


def _run(world, name, dtype, mode, entry="pa_exchange_all"):
    pamd, case = world.pamd, world.cases[name]
    start, want = _reference(case, dtype, mode)
    v = world.vector(name, dtype)
    for dv, a in zip(v.values.parts, start):
        dv.upload(a)
    _call_exchange(pamd, v, world.exchangers(name), mode, entry)
    got = v.to_host().parts
    _differences(got, want, f"{name} {_DT(dtype)} {X.MODE_IDS[X.MODES.index(mode)]}")
    if mode[2]:  # the ghosts are all-zero bytes, whatever they held
        for g, h in zip(got, case.hids):
            assert not g[h - 1].view(np.uint8).any()


# ---- the reference side: the values make the order of a fold visible -----------

FOLD_CASES = ([(n, d) for n in ("dup", "lonely") for d in X.DTYPES] +
              [("wide_dup", np.float64), ("wide_dup", np.complex128)])  # every case with repeated targets, in its types


@pytest.mark.parametrize("name,dtype", FOLD_CASES, ids=[f"{n}-{_DT(d)}" for n, d in FOLD_CASES])
def test_values_make_fold_order_visible(cases, name, dtype):
    """At least 100 targets with two or more contributions, and folding them
    in descending slot order changes the bits of at least 10 % of the ADD
    runs' ones: an unpack in another order cannot pass."""
    wide = name == "wide_dup"
    case = X.wide_case(True) if wide else cases[name]
    multi, multi_add, changed = X.fold_order_stats(case, dtype, [m for m in X.MODES if not (wide and m[2])])
    print(f"{name} {_DT(dtype)}: {multi} targets with several contributions over the runs, {multi_add} in ADD "
          f"runs, descending order changes {changed} of them ({100.0 * changed / multi_add:.1f} %)")
    assert multi >= 100
    assert changed >= 0.10 * multi_add


# ---- pa_exchange_all ---------------------------------------------------------------

@pytest.mark.parametrize("halo_pull", [1, 0], ids=["pull", "copies"])
@pytest.mark.parametrize("backend", ["shared", "own"])
@pytest.mark.parametrize("dtype", X.DTYPES, ids=_DT)
@pytest.mark.parametrize("mode", X.MODES, ids=X.MODE_IDS)
@pytest.mark.parametrize("name", ["ghost", "dup", "forward", "lonely"])
def test_exchange_all(pamd, worlds, name, mode, dtype, backend, halo_pull):
    restore = _tuned(pamd, halo_pull=halo_pull)
    try:
        _run(worlds[backend], name, dtype, mode)
    finally:
        restore()


@pytest.mark.parametrize("dtype", [F64, C64], ids=_DT)
@pytest.mark.parametrize("mode", X.MODES, ids=X.MODE_IDS)
@pytest.mark.parametrize("name", ["ghost", "dup"])
def test_exchange_all_rccl(worlds, name, mode, dtype):
    """the segments through grouped ncclSend/ncclRecv, then the unpack kernels"""
    _run(worlds["rccl"], name, dtype, mode)


@pytest.mark.parametrize("mode", X.MODES, ids=X.MODE_IDS)
@pytest.mark.parametrize("name", ["dup", "forward"])
def test_exchange_all_async(worlds, name, mode):
    _run(worlds["shared"], name, F64, mode, entry="pa_exchange_all_async")


@pytest.mark.parametrize("halo_pull", [1, 0], ids=["pull", "copies"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128], ids=_DT)
@pytest.mark.parametrize("mode", [m for m in X.MODES if not m[2]], ids=[i for i, m in zip(X.MODE_IDS, X.MODES) if not m[2]])
@pytest.mark.parametrize("name", ["wide", "wide_dup"])
def test_exchange_all_wide(pamd, worlds, name, mode, dtype, halo_pull):
    """more slots (wide) and more targets (wide_dup) than 4096 blocks of 256
    threads: every grid-stride loop of the pack, pull and unpack kernels goes
    round twice"""
    case = worlds["shared"].cases[name]
    assert len(case.lids_rcv[1][0]) > 1_048_576 and len(np.unique(case.into(mode[1])[1 - mode[1]][0])) > 1_048_576
    restore = _tuned(pamd, halo_pull=halo_pull)
    try:
        _run(worlds["shared"], name, dtype, mode)
    finally:
        restore()


# ---- mul! with caller-supplied exchangers ---------------------------------------------

_MAT = {}


def _matrix(world, backend, dtype):
    """a from_coo matrix (local ids) on the main partition: 3 to 9 entries per
    owned row over owned and ghost columns"""
    key = (backend, _DT(dtype))
    if key not in _MAT:
        pamd, case = world.pamd, world.cases["ghost"]
        rows = world.rows("ghost")
        rng = np.random.default_rng(X.SEED + 5)
        I, J, V = [], [], []
        for p, n in enumerate(case.sizes):
            own = np.flatnonzero(case.lid_to_part[p] == p + 1) + 1
            k = rng.integers(3, 10, len(own))
            I.append(np.repeat(own, k))
            J.append(np.concatenate([rng.choice(n, kk, replace=False) + 1 for kk in k]))
            V.append(X.family(rng, int(k.sum()), dtype))
            assert np.isin(J[-1], case.hids[p]).any() and not np.isin(J[-1], case.hids[p]).all()
        part = rows.partition
        mk = lambda xs: pamd.PData(part.backend, part.part_ids, xs, part.shape)
        _MAT[key] = pamd.PSparseMatrix.from_coo(mk(I), mk(J), mk(V), rows, rows, ids="local")
    return _MAT[key]


MUL_PATHS = ([("shared", dict(spmv_group=g, halo_direct=d)) for g in (1, 0) for d in (1, 0)] +
             [("own", dict(issue_threads=t, halo_barrier=b, halo_pull=q)) for t in (0, 2) for b in (1, 0) for q in (1, 0)])


@pytest.mark.parametrize("backend,knobs", MUL_PATHS,
                         ids=[b + "-" + "-".join(f"{k}{v}" for k, v in kn.items()) for b, kn in MUL_PATHS])
@pytest.mark.parametrize("dtype", [F64, C64], ids=_DT)
@pytest.mark.parametrize("name", ["ghost", "dup", "forward"])
def test_mul_halo(pamd, worlds, name, dtype, backend, knobs):
    """mul!(y, A, b) with b on PRange(ngids, partition, Exchanger(case)): b
    ends as the reference's REPLACE forward exchange of it, and y as mul! of
    the same matrix with a vector that needs no halo (empty exchanger) and
    holds those values — the SpMV kernels have their own parity tests, this
    isolates the halo.  Twice on fresh values: the barrier issue alternates
    its send buffers.  A lid that is sent and received (forward) travels with
    its old value, as in the reference, where every part packs before any
    unpacks."""
    world = worlds[backend]
    case = world.cases[name]
    A = _matrix(world, backend, dtype)
    b = world.vector(name, dtype)
    y = world.vector("ghost", dtype, slot=1)
    b2 = world.vector("ghost", dtype, "empty")
    y2 = world.vector("ghost", dtype, slot=2)
    restore = _tuned(pamd, **knobs)
    try:
        for rnd in range(2):
            rng = np.random.default_rng([X.SEED, 77, rnd, sum(map(ord, name))])
            start = [X.family(rng, n, dtype) for n in case.sizes]
            want = [a.copy() for a in start]
            R.exchange(want, *case.tables, R.REPLACE, False)
            for dv, a in zip(b.values.parts, start):
                dv.upload(a)
            for dv, a in zip(b2.values.parts, want):
                dv.upload(a)
            for v in (y, y2):
                v.fill_(0)
            pamd.mul_(y, A, b)
            pamd.mul_(y2, A, b2)
            _differences(b.to_host().parts, want, f"b after mul! ({name}, round {rnd})")
            _differences(b2.to_host().parts, want, "the halo-free vector after mul!")
            got = y.to_host().parts
            _differences(got, y2.to_host().parts, f"y of mul! ({name}, round {rnd})")
            assert all(np.count_nonzero(g) >= n for g, n in zip(got, X.NOWN))  # y was computed
    finally:
        restore()


# ---- matrix entries -------------------------------------------------------------------

MAT_MODES = [(op, rev, z) for op, rev, z in X.MODES if (op, rev, z) not in ((R.REPLACE, 0, 0), (R.ADD, 1, 1))]


@pytest.fixture(scope="module")
def kat(pamd, worlds):
    """the diagonal matrix of test_interfaces_matrix_exchange_kat (the
    reference's irregular four-part partition), per element type, and a twin
    that only ever gets set_values"""
    import json
    import os
    k = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "interfaces_kats.json")))["exchanger"]
    parts = worlds["shared"].backend.get_part_ids(4)
    sets = [pamd.IndexSet(p + 1, k["lid_to_gid"][p], k["lid_to_part"][p]) for p in range(4)]
    ids = pamd.prange_from_partition(10, pamd.PData(parts.backend, parts.part_ids, sets, parts.shape))
    out = {"ids": ids, "sets": sets}
    for dtype in (F64, C64):
        csc = pamd.map_parts(lambda s: pamd.compresscoo(np.arange(1, s.num_lids + 1), np.arange(1, s.num_lids + 1),
                                                        np.full(s.num_lids, 2.0).astype(dtype), s.num_lids, s.num_lids),
                             ids.partition)
        out[_DT(dtype)] = (pamd.PSparseMatrix.from_csc(csc, ids, ids), pamd.PSparseMatrix.from_csc(csc, ids, ids))
    return out


@pytest.mark.parametrize("dtype", [F64, C64], ids=_DT)
@pytest.mark.parametrize("mode", MAT_MODES, ids=[X.MODE_IDS[X.MODES.index(m)] for m in MAT_MODES])
def test_mat_exchange_all(pamd, kat, mode, dtype):
    """pa_mat_exchange_all with the six (op, reverse, zero_sent) triples that
    exchange!(A) and assemble!(A) do not use: nonzeros(A) equal the reference
    applied to the nz positions, the lids the transfer left from zeroed when
    asked, and a following mul! sees them (the side copies were refreshed)."""
    op, reverse, zero_sent = mode
    A, B = kat[_DT(dtype)]
    ex = A.exchanger
    tabs = lambda t: [(np.asarray(x.data, np.int64), np.asarray(x.ptrs, np.int64)) for x in t.parts]
    tables = ([list(p) for p in ex.parts_rcv.parts], tabs(ex.lids_rcv), [list(p) for p in ex.parts_snd.parts],
              tabs(ex.lids_snd))
    assert sum(len(t[0]) for t in tables[1]) >= 8  # the ghost rows' entries travel
    rng = np.random.default_rng([X.SEED, 99, X.MODES.index(mode), np.dtype(dtype).num])
    start = [X.family(rng, s.num_lids, dtype) for s in kat["sets"]]
    want = [a.copy() for a in start]
    R.exchange(want, *tables, op, bool(reverse))
    if zero_sent:
        R.zero(want, [t[0] for t in (tables[1] if reverse else tables[3])])
    for M, a in zip(A.values.parts, start):
        M.set_values(a)
    xg = pamd.pvector._mat_dev_xchg(A)
    hs = pamd._lib.ptr_array
    pamd._lib.call("pa_mat_exchange_all", len(xg), hs([M.h for M in A.values.parts]), hs([x.h for x in xg]),
                   pamd._lib.PA_ADD if op == R.ADD else pamd._lib.PA_REPLACE, int(reverse), int(zero_sent))
    _differences([M.get_values() for M in A.values.parts], want, "nonzeros(A)")
    assert any(w.tobytes() != s.tobytes() for w, s in zip(want, start))
    for M, a in zip(B.values.parts, want):
        M.set_values(a)
    ids = kat["ids"]
    x = pamd.PVector.from_host(pamd.map_parts(lambda s: X.family(rng, s.num_lids, dtype), ids.partition), ids)
    ya, yb = pamd.PVector.undef(ids, dtype), pamd.PVector.undef(ids, dtype)
    pamd.mul_(ya, A, x)
    pamd.mul_(yb, B, x)
    _differences(ya.to_host().parts, yb.to_host().parts, "mul! after the matrix exchange")
    assert any(np.count_nonzero(g) for g in ya.to_host().parts)
