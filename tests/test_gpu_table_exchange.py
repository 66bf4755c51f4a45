"""pa_table_exchange_all and its async twin — exchange!(combine_op,
values::AbstractPData{<:Table}, exchanger) with rows of any length per lid —
against tests/table_exchange_ref.py, by bytes over every data entry of every
part: all eight (op, reverse, zero_sent) combinations, the four element
types, three parts on device 0 sharing a stream pair, with their own stream
pairs, and over RCCL.

Cases (tests/table_exchange_cases.py): ghost (exchanger_from_ids of the
partition, read out for the reference), forward and lonely of the vector
exchange tests, and tdup (41 classes built class-first: several source rows
per target row, two slots of one segment naming one target).  Row lengths are
drawn per class from {0, 1, 2, 3, 65, 300}; test_table_exchange_ref_host.py
asserts the class, length and fold-order conditions on the reference side.

The new kernels (pa_table.hip) run no grid-stride loop under a capped grid:
every launch covers its items (one thread per slot or target for the
lengths, one wave per slot or target for the fills).  test_wide still runs
1,048,876 slots, more than the 4096 blocks of 256 threads that cap the pack
and unpack kernels the values move through, and 262,219 blocks of the fill."""
import json
import os
import re

import numpy as np
import pytest

import exchange_cases as X
import exchange_ref as R
import table_exchange_cases as TC
import table_exchange_ref as T

pytestmark = pytest.mark.gpu

F64, C64 = np.float64, np.complex64
_DT = lambda d: np.dtype(d).name
_ID = lambda mode: X.MODE_IDS[X.MODES.index(mode)]


def _differences(got, want, what):
    """compare by bytes; on a mismatch name the entries"""
    for p, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: part {p + 1} has another type or length"
        if g.tobytes() != w.tobytes():
            k = g.dtype.itemsize
            bad = np.flatnonzero((g.view(np.uint8).reshape(-1, k) != w.view(np.uint8).reshape(-1, k)).any(axis=1))
            show = ", ".join(f"entry {l + 1}: {g[l]!r} != {w[l]!r}" for l in bad[:4])
            pytest.fail(f"{what}: part {p + 1}: {len(bad)} of {len(g)} data entries differ ({show})")


class World:
    """One backend's contexts with the cases' partitions, exchangers and
    tables on them, each built once."""

    def __init__(self, pamd, backend, cases):
        self.pamd, self.backend, self.cases = pamd, backend, cases
        self._part, self._ex, self._tab = {}, {}, {}

    def partition(self, name):
        c = self.cases[name]
        key = id(c.lid_to_gid)
        if key not in self._part:
            parts = self.backend.get_part_ids(c.nparts)
            sets = [self.pamd.IndexSet(p + 1, c.lid_to_gid[p], c.lid_to_part[p]) for p in range(c.nparts)]
            self._part[key] = self.pamd.PData(parts.backend, parts.part_ids, sets, parts.shape)
        return self._part[key]

    def pdata(self, name, xs):
        part = self.partition(name)
        return self.pamd.PData(part.backend, part.part_ids, list(xs), part.shape)

    def exchanger(self, name):
        if name not in self._ex:
            pamd, c = self.pamd, self.cases[name]
            if name == "ghost":
                self._ex[name] = pamd.exchanger_from_ids(self.partition(name))
            else:
                tab = lambda ts: self.pdata(name, [pamd.Table(d, p) for d, p in ts])
                self._ex[name] = pamd.Exchanger(self.pdata(name, c.parts_rcv), self.pdata(name, c.parts_snd),
                                                tab(c.lids_rcv), tab(c.lids_snd))
        return self._ex[name]

    def new_tables(self, name, dtype, tptrs, device_ptrs=False):
        """a PData of DeviceTable with the given row pointers (data: zero)"""
        pamd = self.pamd
        ctxs = pamd.device.contexts(self.partition(name))
        tabs = []
        for c, p in zip(ctxs, tptrs):
            if device_ptrs:  # the ptrs as an Int32 array on the part's device
                holder = pamd.device.DeviceVector(c, np.float32, len(p))
                holder.upload(np.asarray(p, np.int32).view(np.float32))
                p = holder.as_array(np.int32)
            tabs.append(pamd.DeviceTable(c, dtype, p))
        return self.pdata(name, tabs)

    def tables(self, name, dtype, variant=0):
        key = (name, _DT(dtype), variant)
        if key not in self._tab:
            self._tab[key] = self.new_tables(name, dtype, TC.table_ptrs(self.cases[name], variant))
        return self._tab[key]


@pytest.fixture(scope="module")
def cases():
    return TC.small_cases()


@pytest.fixture(scope="module")
def worlds(pamd, cases):
    if pamd.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests need the MI355X")
    W = {"shared": World(pamd, pamd.HIPBackend(devices=[0], share_streams=True), cases),
         "own": World(pamd, pamd.HIPBackend(devices=[0], share_streams=False), cases),
         "rccl": World(pamd, pamd.HIPBackend(devices=[0], rccl=True), cases)}
    # ghost: the exchanger the package derives from the index sets, read out for the reference
    ex = W["shared"].exchanger("ghost")
    c = cases["ghost"]
    tabs = lambda t: [(np.asarray(x.data, np.int32), np.asarray(x.ptrs, np.int32)) for x in t.parts]
    c.set_tables([np.asarray(p, np.int32) for p in ex.parts_rcv.parts], tabs(ex.lids_rcv),
                 [np.asarray(p, np.int32) for p in ex.parts_snd.parts], tabs(ex.lids_snd))
    for name in TC.CASES:  # the conditions the host test asserts hold for what the device gets
        T.check_lengths(cases[name].sizes, cases[name].tables, TC.table_ptrs(cases[name]))
    return W


_REF = {}


def _reference(case, dtype, mode, variant=0, salt=0):
    """(ptrs, start, expected) of a run, computed once and never written to"""
    key = (case.name, _DT(dtype), mode, variant, salt)
    if key not in _REF:
        tptrs = TC.table_ptrs(case, variant)
        start = TC.start_data(case, tptrs, dtype, mode, salt)
        want = TC.expected(case, tptrs, start, mode)
        for a in start + want:
            a.setflags(write=False)
        _REF[key] = (tptrs, start, want)
    return _REF[key]


def _exchange(pamd, tabs, ex, mode, use_async=False):
    op, reverse, zero = mode
    kw = dict(combine="+" if op == R.ADD else None, reverse=bool(reverse), zero_sent=bool(zero))
    if not use_async:
        assert pamd.exchange_table_(tabs, ex, **kw) is tabs
        return
    tasks = pamd.async_exchange_table_(tabs, ex, **kw)
    assert all(isinstance(t, pamd.Task) and t.h for t in tasks.parts)
    pamd.wait_all(tasks)
    assert all(t.done() for t in tasks.parts)


def _run(world, name, dtype, mode, use_async=False, variant=0, salt=0, tabs=None):
    pamd, case = world.pamd, world.cases[name]
    tptrs, start, want = _reference(case, dtype, mode, variant, salt)
    if tabs is None:
        tabs = world.tables(name, dtype, variant)
    for t, a in zip(tabs.parts, start):
        t.upload(a)
    _exchange(pamd, tabs, world.exchanger(name), mode, use_async)
    got = [t.download() for t in tabs.parts]
    _differences(got, want, f"{name} {_DT(dtype)} {_ID(mode)}")
    if mode[2]:  # the rows the transfer left from are all-zero bytes, whatever they held
        for g, l, p in zip(got, case.frm(mode[1]), tptrs):
            assert not g[T.expand(l, p)[0] - 1].view(np.uint8).any()
    assert any(w.tobytes() != s.tobytes() for w, s in zip(want, start))  # the run moved something


# ---- parity ------------------------------------------------------------------------

@pytest.mark.parametrize("backend", ["shared", "own"])
@pytest.mark.parametrize("dtype", X.DTYPES, ids=_DT)
@pytest.mark.parametrize("mode", X.MODES, ids=X.MODE_IDS)
@pytest.mark.parametrize("name", TC.CASES)
def test_table_exchange(worlds, name, mode, dtype, backend):
    _run(worlds[backend], name, dtype, mode)


@pytest.mark.parametrize("dtype", [F64, C64], ids=_DT)
@pytest.mark.parametrize("mode", X.MODES, ids=X.MODE_IDS)
@pytest.mark.parametrize("name", TC.CASES)
def test_table_exchange_rccl(worlds, name, mode, dtype):
    """the expanded segments through grouped ncclSend/ncclRecv, then the unpack kernels"""
    _run(worlds["rccl"], name, dtype, mode)


@pytest.mark.parametrize("mode", X.MODES, ids=X.MODE_IDS)
@pytest.mark.parametrize("name", ["forward", "tdup"])
def test_table_exchange_async(worlds, name, mode):
    _run(worlds["shared"], name, F64, mode, use_async=True)


@pytest.mark.parametrize("backend", ["shared", "own", "rccl"])
def test_repeated_exchange_and_a_second_table(worlds, backend):
    """The same table again with fresh values (its cached derived exchanger),
    then a table with other row lengths on the same exchanger (its own), then
    the first once more."""
    world = worlds[backend]
    mode = (R.ADD, 0, 1)
    for variant, salt in ((0, 1), (0, 2), (1, 3), (0, 4)):
        _run(world, "tdup", F64, mode, variant=variant, salt=salt)
        _run(world, "forward", F64, (R.REPLACE, 1, 0), variant=variant, salt=salt)


def test_host_ptrs_and_device_ptrs_agree(worlds):
    world = worlds["shared"]
    case = world.cases["tdup"]
    for mode in ((R.REPLACE, 0, 0), (R.ADD, 1, 1)):
        tptrs, start, want = _reference(case, C64, mode)
        out = []
        for device_ptrs in (False, True):
            tabs = world.new_tables("tdup", C64, tptrs, device_ptrs)
            assert [t.ptrs().tolist() for t in tabs.parts] == [p.tolist() for p in tptrs]
            _run(world, "tdup", C64, mode, tabs=tabs)
            out.append([t.download() for t in tabs.parts])
        _differences(out[1], out[0], "device ptrs against host ptrs")


def test_bad_device_ptrs_are_rejected(pamd, worlds):
    world = worlds["shared"]
    for bad, words in (([2, 3, 4], "must be 1"), ([1, 5, 4], "not decrease")):
        with pytest.raises(pamd.PAError, match=words):
            world.new_tables("tdup", F64, [np.array(bad, np.int32)] * 3, device_ptrs=True)


# ---- integer payloads ---------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=_DT)
def test_integer_kat(pamd, worlds, dtype):
    """test_interfaces.jl:255-264 as test_exchange_table_kat checks it: owned
    rows [100*owner + 10*gid + i], ghost rows zero; afterwards every lid holds
    its owner's row"""
    k = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "interfaces_kats.json")))["exchanger"]
    parts = worlds["shared"].backend.get_part_ids(4)
    sets = [pamd.IndexSet(p + 1, k["lid_to_gid"][p], k["lid_to_part"][p]) for p in range(4)]
    part = pamd.PData(parts.backend, parts.part_ids, sets, parts.shape)
    ex = pamd.exchanger_from_ids(part)
    tabs = []
    for c, s in zip(pamd.device.contexts(part), sets):
        rows = [[100 * s.part + 10 * g + i for i in (1, 2, 3)] if o == s.part else [0, 0, 0]
                for g, o in zip(s.lid_to_gid, s.lid_to_part)]
        tabs.append(pamd.DeviceTable.from_host(c, pamd.Table.from_lists(rows, dtype=dtype)))
    tabs = pamd.PData(part.backend, part.part_ids, tabs, part.shape)
    pamd.exchange_table_(tabs, ex)
    for s, t in zip(sets, tabs.parts):
        host = t.to_host()
        assert host.data.dtype == dtype and len(host) == s.num_lids
        for lid in range(1, s.num_lids + 1):
            g, o = s.lid_to_gid[lid - 1], s.lid_to_part[lid - 1]
            assert host[lid].tolist() == [100 * o + 10 * g + i for i in (1, 2, 3)]


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=_DT)
@pytest.mark.parametrize("reverse", [0, 1])
def test_integer_bit_patterns(pamd, worlds, dtype, reverse):
    """payloads that read as a signalling NaN, a denormal and all ones in the
    float type of their width come back bit for bit (replace)"""
    world = worlds["own"]
    case = world.cases["tdup"]
    tptrs = TC.table_ptrs(case)
    u = np.uint32 if dtype == np.int32 else np.uint64
    pats = (np.array([0x7FA00001, 0x00000001, 0xFFFFFFFF, 0xFF800001], u) if dtype == np.int32 else
            np.array([0x7FF4000000000001, 0x0000000000000001, 0xFFFFFFFFFFFFFFFF, 0xFFF0000000000001], u))
    rng = np.random.default_rng([X.SEED, 41, reverse])
    start = [pats[rng.integers(0, len(pats), int(p[-1]) - 1)].view(dtype) +
             (np.arange(int(p[-1]) - 1) % 7 == 3).astype(dtype) * 2 for p in tptrs]
    want = [a.copy() for a in start]
    T.exchange(want, tptrs, *case.tables, R.REPLACE, bool(reverse))
    tabs = world.new_tables("tdup", dtype, tptrs)
    for t, a in zip(tabs.parts, start):
        t.upload(a)
    pamd.exchange_table_(tabs, world.exchanger("tdup"), reverse=bool(reverse))
    _differences([t.download() for t in tabs.parts], want, f"{_DT(dtype)} payloads")
    assert any(w.tobytes() != s.tobytes() for w, s in zip(want, start))
    with pytest.raises(TypeError, match="cannot be added"):
        pamd.exchange_table_(tabs, world.exchanger("tdup"), combine="+")
    with pytest.raises(TypeError, match="cannot be added"):
        pamd.async_exchange_table_(tabs, world.exchanger("tdup"), combine="+")


# ---- degenerate tables ----------------------------------------------------------------

@pytest.mark.parametrize("backend", ["shared", "rccl"])
def test_all_empty_table_is_a_no_op(pamd, worlds, backend):
    world = worlds[backend]
    case = world.cases["forward"]
    tabs = world.new_tables("forward", F64, [np.ones(n + 1, np.int32) for n in case.sizes])
    for mode in X.MODES:
        _exchange(pamd, tabs, world.exchanger("forward"), mode)
        _exchange(pamd, tabs, world.exchanger("forward"), mode, use_async=True)
    for t, n in zip(tabs.parts, case.sizes):
        host = t.to_host()
        assert (t.nrows, t.ndata) == (n, 0) and host.ptrs.tolist() == [1] * (n + 1) and len(host.data) == 0


def test_to_host_round_trips(pamd, worlds):
    """ptrs and data of every part, the part without lids (lonely's third) included"""
    world = worlds["shared"]
    case = world.cases["lonely"]
    assert case.sizes[2] == 0
    tptrs, start, _ = _reference(case, C64, (R.REPLACE, 0, 0))
    ctxs = pamd.device.contexts(world.partition("lonely"))
    for c, p, a in zip(ctxs, tptrs, start):
        t = pamd.DeviceTable.from_host(c, pamd.Table(a, p))
        host = t.to_host()
        assert host.ptrs.dtype == np.int32 and host.ptrs.tolist() == p.tolist()
        assert host.data.dtype == a.dtype and host.data.tobytes() == a.tobytes()
        assert t.data.n == len(a) and t.data.download().tobytes() == a.tobytes()  # the data as a DeviceVector


# ---- mismatch ---------------------------------------------------------------------------

@pytest.mark.parametrize("backend", ["shared", "rccl"])
@pytest.mark.parametrize("use_async", [False, True], ids=["blocking", "async"])
def test_row_length_mismatch_is_an_error(pamd, worlds, backend, use_async):
    """one ghost row one entry longer than its owner's row: an error naming
    the two parts and the two counts, raised before any value moves"""
    world = worlds[backend]
    case = world.cases["ghost"]
    tptrs = [p.copy() for p in TC.table_ptrs(case)]
    q = 0  # the receiver: part 1; its first ghost lid of the first segment
    data, ptrs = case.lids_rcv[q]
    sender = int(case.parts_rcv[q][0])
    assert ptrs[1] > ptrs[0]
    lid = int(data[ptrs[0] - 1])
    xr, xs = T.table_exchanger(tptrs, case.lids_rcv, case.lids_snd)  # the expanded segments as they match
    m = list(case.parts_snd[sender - 1]).index(q + 1)
    have = int(xs[sender - 1][1][m + 1] - xs[sender - 1][1][m])
    want = int(xr[q][1][1] - xr[q][1][0]) + 1
    assert want == have + 1
    tptrs[q][lid:] += 1  # row `lid` of part 1 one entry longer
    tabs = world.new_tables("ghost", F64, tptrs)
    rng = np.random.default_rng(X.SEED + 43)
    start = [X.family(rng, int(p[-1]) - 1, F64) for p in tptrs]
    for t, a in zip(tabs.parts, start):
        t.upload(a)
    call = pamd.async_exchange_table_ if use_async else pamd.exchange_table_
    with pytest.raises(pamd.PAError) as e:
        call(tabs, world.exchanger("ghost"))
    m = re.search(r"part (\d+) sends (\d+) entries to part (\d+), whose rows for them hold (\d+)", str(e.value))
    assert m, str(e.value)
    assert [int(x) for x in m.groups()] == [sender, have, q + 1, want]
    _differences([t.download() for t in tabs.parts], start, "the tables after the refused call")
    # the reverse direction sees the same pair of rows from the other side
    with pytest.raises(pamd.PAError, match=rf"part {q + 1} sends {want} entries to part {sender}, whose rows for them hold {have}"):
        call(tabs, world.exchanger("ghost"), reverse=True)
    _differences([t.download() for t in tabs.parts], start, "the tables after the refused reverse call")


def test_wrong_tables_are_refused(pamd, worlds):
    """fewer rows than the exchanger's largest lid; a table of another context"""
    world = worlds["shared"]
    case = world.cases["forward"]
    tptrs = TC.table_ptrs(case)
    short = [p[:max(1, len(p) // 4)] for p in tptrs]
    with pytest.raises(pamd.PAError, match="fewer rows"):
        pamd.exchange_table_(world.new_tables("forward", F64, short), world.exchanger("forward"))
    other = worlds["own"].new_tables("forward", F64, tptrs)
    mixed = world.pdata("forward", other.parts)
    with pytest.raises(pamd.PAError, match="different contexts"):
        pamd.exchange_table_(mixed, world.exchanger("forward"))


# ---- more slots than the capped grids of the pack / unpack kernels cover ------------------

@pytest.fixture(scope="module")
def wide(pamd, worlds):
    case = X.wide_case(False)
    nslots = len(case.lids_snd[0][0])
    assert nslots == 1_048_876 > 4096 * 256
    rng = np.random.default_rng(X.SEED + 47)
    per_slot = rng.integers(0, 4, nslots)  # one class per slot pair: both lists are without repeats
    n = [rng.integers(0, 4, s) for s in case.sizes]
    n[0][case.lids_snd[0][0] - 1] = per_slot
    n[1][case.lids_rcv[1][0] - 1] = per_slot
    tptrs = [np.concatenate([[1], 1 + np.cumsum(x)]).astype(np.int32) for x in n]
    world = World(pamd, worlds["shared"].backend, {"wide": case})
    return world, case, tptrs, world.new_tables("wide", F64, tptrs)


@pytest.mark.parametrize("op", [R.REPLACE, R.ADD])
def test_wide(wide, op):
    world, case, tptrs, tabs = wide
    mode = (op, 0, 0)
    rng = np.random.default_rng([X.SEED, 53, X.MODES.index(mode)])
    start = [X.family(rng, int(p[-1]) - 1, F64) for p in tptrs]
    want = [a.copy() for a in start]
    T.exchange(want, tptrs, *case.tables, op, False)
    for t, a in zip(tabs.parts, start):
        t.upload(a)
    _exchange(world.pamd, tabs, world.exchanger("wide"), mode)
    _differences([t.download() for t in tabs.parts], want, f"wide {op}")
    assert np.count_nonzero(want[1] != start[1]) > 1_000_000
