"""bench.py --gpus N without torchrun around it starts the N one-part ranks
itself (launch_ranks) before anything touches the GPU: the command it runs
is the driver's torchrun command with this script's arguments, on the
loopback, with dmabuf IPC (no CPU-side GPU work needed to check this)."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_n_self_launches_torchrun(monkeypatch):
    bench = _load_bench()
    seen = {}

    class Done:
        returncode = 7

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return Done()

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "9", "--warmup", "2"])
    assert bench.main() == 7  # the ranks' exit status is passed on
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    i = cmd.index("--nproc-per-node")
    assert cmd[i + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--nnodes") + 1] == "1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "9", "--warmup", "2"]
    assert os.path.samefile(cmd[-7], os.path.join(ROOT, "bench.py"))
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_torchrun_rank_does_not_relaunch(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(bench, "launch_ranks", lambda n: (_ for _ in ()).throw(AssertionError("relaunched")))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "1"])
    monkeypatch.setenv("WORLD_SIZE", "2")  # already a torchrun rank: no second launch
    # the rank path then needs a GPU: stop it at its first step (fd 1 to stderr)
    class OsProxy:
        def __getattr__(self, name):
            return getattr(os, name)

        @staticmethod
        def dup(fd):
            raise RuntimeError("rank path reached")

    monkeypatch.setattr(bench, "os", OsProxy())
    try:
        bench.main()
        raise AssertionError("the rank path did not start")
    except RuntimeError as e:
        assert "rank path reached" in str(e)


def test_one_process_leg_runs_a_bounded_child_and_reports_failure(monkeypatch):
    """The one-process leg of an N-rank run (bench.one_process_leg): rank 0
    starts `bench.py --child-oneproc` with the run's problem and without the
    torchrun rank variables, bounded by a timeout; a child that fails (here:
    no GPU in this container) becomes a note in the line, not an exception."""
    import argparse
    bench = _load_bench()
    seen = {}
    real_run = bench.subprocess.run

    def spy(cmd, env=None, **kw):
        seen["cmd"], seen["env"], seen["kw"] = cmd, env, kw
        return real_run(cmd, env=env, **kw)

    monkeypatch.setattr(bench.subprocess, "run", spy)
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "8")
    a = argparse.Namespace(gpus=8, n=32, kind=27, dtype="f64", steps=3, warmup=1, tune="", oneproc_devices="")
    out = bench.one_process_leg(a)
    cmd = seen["cmd"]
    assert "--child-oneproc" in cmd and cmd[cmd.index("--gpus") + 1] == "8" and cmd[cmd.index("--n") + 1] == "32"
    assert "RANK" not in seen["env"] and "WORLD_SIZE" not in seen["env"]
    assert seen["kw"].get("timeout")
    assert "note" in out and "failed" in out["note"], out


def test_dump_outputs_writes_owned_y_as_real_arrays(monkeypatch, tmp_path):
    """--dump-outputs (bench.dump_outputs): one y_part<p>.npy per part with the
    owned values, complex as (n, 2) re/im pairs; a part above its share of
    DUMP_BYTES is a fixed sorted sample, the same in every run."""
    import types

    import numpy as np
    bench = _load_bench()

    class Parts:
        def __init__(self, d):
            self.d, self.part_ids = d, list(d)

        def local(self, p):
            return self.d[p]

    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 40 * 8)  # 40 float64 values per part
    vals = {1: np.arange(105, dtype=np.float64), 2: (np.arange(30) * (1 + 2j)).astype(np.complex64)}
    sets = {1: types.SimpleNamespace(oid_to_lid=np.arange(1, 101)), 2: types.SimpleNamespace(oid_to_lid=np.arange(11, 31))}
    y = types.SimpleNamespace(to_host=lambda: Parts(vals))
    rows = types.SimpleNamespace(partition=Parts(sets))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), Parts(vals), rows, y, 2)
    a1, a2 = np.load(tmp_path / "a" / "y_part1.npy"), np.load(tmp_path / "a" / "y_part2.npy")
    assert a1.dtype == np.float64 and a1.shape == (40,)
    assert np.all(np.diff(a1) > 0) and a1.max() < 100  # a sorted sample without repeats of the owned values
    assert a2.dtype == np.float32 and np.array_equal(a2, np.stack([np.arange(10, 30), 2 * np.arange(10, 30)], 1))
    assert np.array_equal(a1, np.load(tmp_path / "b" / "y_part1.npy"))


def test_rccl_run_info_proves_ranks_and_devices():
    """config.rccl_halo of an N > 1 line: the
    communicator size of every rank (ncclCommCount), the distinct devices
    and the resolved librccl; a run whose ranks folded onto fewer GPUs, or
    whose communicator is smaller than the world, fails instead of
    reporting."""
    import pytest
    bench = _load_bench()
    lib = "/opt/rocm/lib/librccl.so.1"
    mk = lambda r, pci, n=2: {"ranks": n, "rank": r, "device": r, "pci": pci, "rccl_version": 22700, "librccl": lib}
    out = bench.rccl_run_info([mk(0, "0000:05:00.0"), mk(1, "0000:15:00.0")], 2)
    assert out["rccl_ranks"] == {"min": 2, "max": 2} and out["distinct_devices"] == 2
    assert out["devices"] == ["0000:05:00.0", "0000:15:00.0"] and out["librccl"] == [lib]
    with pytest.raises(SystemExit, match="distinct devices"):
        bench.rccl_run_info([mk(0, "0000:05:00.0"), mk(1, "0000:05:00.0")], 2)
    with pytest.raises(SystemExit, match="communicator sizes"):
        bench.rccl_run_info([mk(0, "0000:05:00.0", 1), mk(1, "0000:15:00.0", 1)], 2)


def _stand_in_pamd(fail_copy_at=None):
    """A CPU stand-in for `pamd` with what bench.main() touches: one part of
    1000 rows whose format bytes are those of a 2 GB operator (one copy is
    enough to stay out of the cache), mul! as y = 2x.  `fail_copy_at`: the
    stencil_operator call (0-based) that fails like a full device."""
    import types

    import numpy as np
    n = 1000

    class PD:
        def __init__(self, d):
            self.d, self.part_ids, self.parts = d, list(d), list(d.values())

        def local(self, p):
            return self.d[p]

    class Ctx:
        device = 0
        sync = span_start = span_stop = lambda self: None
        set_timing = lambda self, on: None
        tune = lambda self, k, v: None
        span_ms = lambda self: 1.0
        kernel_times = lambda self: {"interior_ms": 0.1, "halo_wait_ms": 0.0, "boundary_ms": 0.0, "calls": 5}

    class HIPBackend:
        share_streams = True

        def __init__(self, devices, **kw):
            self.ctx = Ctx()

        def get_part_ids(self, shape):
            return PD({p: p for p in range(1, int(np.prod(shape)) + 1)})

        def context(self, p):
            return self.ctx

    class Mat:
        def info(self):
            return dict(nrows=n, nnz=27 * n, value_bytes=2_000_000_000, index_bytes=100, meta_bytes=10,
                        pattern_slices=1, nslices=2, regular_rows=n, side_rows=0)

        def traffic(self):
            return dict(value_bytes=8 * 27 * n, index_bytes=4 * 27 * n, meta_bytes=10)

    class PVector:
        def __init__(self, vals):
            self.vals = vals

        from_host = staticmethod(lambda pd, cols: PVector(pd))
        undef = staticmethod(lambda rows, dtype=np.float64: PVector(
            PD({p: np.zeros(n, dtype) for p in rows.partition.part_ids})))

        def to_host(self):
            return self.vals

    class PAError(RuntimeError):
        pass

    m = types.ModuleType("pamd")
    m.built, m.mul_calls = [], []

    def mul_(y, A, x):
        m.mul_calls.append(A)
        for p in y.vals.part_ids:
            y.vals.d[p][:] = 2 * x.vals.d[p][:n]

    def stencil_partition(parts, N, kind):
        sets = PD({p: types.SimpleNamespace(part=p, num_lids=n, num_hids=0, oid_to_lid=np.arange(1, n + 1))
                   for p in parts.part_ids})
        empty = PD({p: types.SimpleNamespace(data=[]) for p in parts.part_ids})
        r = types.SimpleNamespace(partition=sets, exchanger=types.SimpleNamespace(lids_snd=empty, lids_rcv=empty))
        return r, r

    def stencil_operator(parts, N, kind, dtype=np.float64, partition=None):
        if fail_copy_at is not None and len(m.built) == fail_copy_at:
            raise PAError("out of memory")
        rows, cols = partition
        A = types.SimpleNamespace(rows=rows, cols=cols, dtype=dtype, values=PD({p: Mat() for p in parts.part_ids}))
        m.built.append(A)
        return A

    m.HIPBackend, m.PVector, m.PAError, m.mul_ = HIPBackend, PVector, PAError, mul_
    m.map_parts = lambda f, pd: PD({p: f(v) for p, v in pd.d.items()})
    m.drivers = types.SimpleNamespace(stencil_partition=stencil_partition, stencil_operator=stencil_operator)
    m._lib = types.SimpleNamespace(tune=lambda k, v: 0, PAError=PAError, hbm_probe_launch=lambda *a: 5000.0)
    return m


def _run_main(monkeypatch, capfd, argv, pamd):
    """bench.main() on the stand-in with the legs that take runs of their own
    replaced by recorders: the printed line and the legs that ran."""
    import json
    bench = _load_bench()
    ran = []

    def leg(name, out):
        def f(*a, **kw):
            ran.append(name)
            return out
        return f

    monkeypatch.setitem(sys.modules, "pamd", pamd)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench, "halo_1gpu", leg("halo_1gpu", {"value": 1.0, "frac": 0.1, "kernel_ms": 1.0,
                                                              "bytes_per_step": 1}))
    monkeypatch.setattr(bench, "pmc_traffic", leg("pmc_traffic", (None, "stand-in")))
    monkeypatch.setattr(bench, "cpu_baseline", leg("cpu_baseline", {"value": 1.0}))
    monkeypatch.setattr(bench, "cpu_baseline_mpi", leg("cpu_baseline_mpi", {"value": 1.0}))
    monkeypatch.setattr(bench, "box_hbm_gbs", leg("box_hbm_gbs", (6000.0, 5000.0)))
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    fd1 = os.dup(1)  # main() points fd 1 at stderr for good: put it back for the next run
    try:
        bench.main()
    finally:
        os.dup2(fd1, 1)
        os.close(fd1)
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # stdout carries exactly the result line
    return json.loads(lines[0]), ran


def test_plain_run_times_the_steps_and_leaves_the_full_legs_out(monkeypatch, capfd):
    pamd = _stand_in_pamd()
    line, ran = _run_main(monkeypatch, capfd, ["--gpus", "1", "--steps", "7", "--warmup", "2"], pamd)
    assert ran == []
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 7 and line["ms_per_step"] > 0
    assert "halo_1gpu" not in line and "cpu_baseline" not in line and "one_process" not in line
    assert line["config"]["per_part_ms"] is None and line["roofline"]["traffic"] is None
    assert line["roofline"]["box_read_gbs"] is None and "int32_columns_kernel_ms" not in line["roofline"]
    # one copy per timed step (7 < 32): each extra copy once when built, 2 warm-up and 7 timed steps, each copy once
    assert line["config"]["operator_copies_rotated"] == 7 and len(pamd.built) == 7
    assert len(pamd.mul_calls) == 6 + 2 + 7
    assert {id(a) for a in pamd.mul_calls[-7:]} == {id(a) for a in pamd.built}


def test_rotation_is_capped_and_survives_a_full_device(monkeypatch, capfd):
    pamd = _stand_in_pamd()
    line, _ = _run_main(monkeypatch, capfd, ["--gpus", "1", "--steps", "70", "--warmup", "2"], pamd)
    assert line["config"]["operator_copies_rotated"] == 32
    pamd = _stand_in_pamd(fail_copy_at=5)  # the sixth operator does not fit: the last built is released too
    line, _ = _run_main(monkeypatch, capfd, ["--gpus", "1", "--steps", "70", "--warmup", "2"], pamd)
    assert line["config"]["operator_copies_rotated"] == 4 and line["steps"] == 70


def test_full_run_keeps_every_leg_on_the_first_copy(monkeypatch, capfd):
    pamd = _stand_in_pamd()
    line, ran = _run_main(monkeypatch, capfd, ["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"], pamd)
    assert ran == ["box_hbm_gbs", "halo_1gpu", "pmc_traffic", "pmc_traffic", "cpu_baseline", "cpu_baseline_mpi"]
    assert "halo_1gpu" in line and "cpu_baseline" in line and "cpu_baseline" in line["halo_1gpu"]
    assert line["config"]["per_part_ms"]["1"]["calls"] == 5
    assert line["roofline"]["box_read_gbs"] == 6000.0 and line["roofline"]["int32_columns_kernel_ms"] == round(1 / 7, 4)
    # attribution and int32-column loops (7 steps: 7 calls each) run the first operator, as one copy did
    assert all(a is pamd.built[0] for a in pamd.mul_calls[6 + 2 + 7:]) and len(pamd.mul_calls) == 6 + 2 + 7 + 14
    line, ran = _run_main(monkeypatch, capfd, ["--steps", "3", "--full", "--no-pmc", "--no-halo-leg",
                                               "--no-cpu-baseline"], _stand_in_pamd())
    assert ran == ["box_hbm_gbs"] and "halo_1gpu" not in line and "cpu_baseline" not in line


def test_dump_outputs_from_the_command_line_and_not_with_cg(monkeypatch, capfd, tmp_path):
    import numpy as np
    import pytest
    out = tmp_path / "dump"
    _run_main(monkeypatch, capfd, ["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)], _stand_in_pamd())
    y = np.load(out / "y_part1.npy")
    assert y.dtype == np.float64 and y.shape == (1000,)
    x = np.random.default_rng(20250114 + 1).uniform(-1, 1, 1000)
    assert np.array_equal(y, 2 * x)  # the timed path's y on the seeded x
    monkeypatch.setattr(sys, "argv", ["bench.py", "--cg", "5", "--dump-outputs", str(out)])
    with pytest.raises(SystemExit):
        _load_bench().main()


def test_dump_outputs_stays_under_64_mb_at_the_headline_size(tmp_path):
    """256^3 Float64 rows of one part (134 MB of y): the sample written is
    DUMP_BYTES of values, under the 64 MB a dump may take."""
    import types

    import numpy as np
    bench = _load_bench()
    n = 256 ** 3

    class Parts:
        def __init__(self, d):
            self.d, self.part_ids = d, list(d)

        def local(self, p):
            return self.d[p]

    vals = {1: np.arange(n, dtype=np.float64)}
    rows = types.SimpleNamespace(partition=Parts({1: types.SimpleNamespace(oid_to_lid=np.arange(1, n + 1))}))
    bench.dump_outputs(str(tmp_path), Parts(vals), rows, types.SimpleNamespace(to_host=lambda: Parts(vals)), 1)
    size = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert bench.DUMP_BYTES <= size <= 64 << 20
