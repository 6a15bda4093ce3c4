"""bench.py host logic that needs no GPU: what rides along with which invocation (a plain run times
its steps and nothing else, --full adds the rest), profiler detection, the loud failure when there is
no device, and what --dump-outputs writes; gpu-marked tests run a plain line and --dump-outputs end
to end."""
import argparse
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(**kw):
    base = dict(rows=8192, cols=16384, sparse_per_col=0, numerics="fast", no_secondary=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_secondary_workload_rides_only_with_the_default_invocation(monkeypatch):
    bench = _bench()
    monkeypatch.delenv("ROCP_TOOL_LIBRARIES", raising=False)
    monkeypatch.setenv("LD_PRELOAD", "")
    assert bench.secondary_wanted(_args())
    assert not bench.secondary_wanted(_args(no_secondary=True))
    assert not bench.secondary_wanted(_args(rows=1024, cols=2048))
    assert not bench.secondary_wanted(_args(sparse_per_col=50))
    assert not bench.secondary_wanted(_args(numerics="strict"))
    assert bench.SECONDARY["rows"] == 32768 and bench.SECONDARY["cols"] == 65536


def test_profiler_detection_keeps_the_run_to_one_workload(monkeypatch):
    bench = _bench()
    monkeypatch.delenv("ROCP_TOOL_LIBRARIES", raising=False)
    monkeypatch.setenv("LD_PRELOAD", "")
    assert not bench.under_profiler()
    monkeypatch.setenv("ROCP_TOOL_LIBRARIES", "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so")
    assert bench.under_profiler() and not bench.secondary_wanted(_args())
    monkeypatch.delenv("ROCP_TOOL_LIBRARIES")
    monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk.so")
    assert bench.under_profiler()


def _main_calls(monkeypatch, capsys, *argv):
    """bench.main() with every measurement replaced by a recorder: what a run would start, in order,
    and the line it prints.  No GPU is touched."""
    import json

    from dantzig_amd import _ffi, sharded

    bench = _bench()
    monkeypatch.delenv("ROCP_TOOL_LIBRARIES", raising=False)
    monkeypatch.setenv("LD_PRELOAD", "")
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    calls = []

    def fake_measure(rows, cols, seed, sparse_per_col, price, numerics, steps, warmup,
                     late_pivots=0, deep_pivots=0, whole_solve=False, mfma_block=False, end_pivots=0,
                     warm_k=0, dump_dir=None):
        calls.append(("measure", rows, steps, warmup, late_pivots, deep_pivots, whole_solve, mfma_block,
                      end_pivots, warm_k))
        return {"value": 1.0, "unit": "iterations/s", "steps": steps, "warmup": warmup, "ms_per_step": 1.0,
                "config": {"k_at_start": 0, "k_at_end": 0}, "roofline": {}}

    monkeypatch.setattr(_ffi, "require_gpu", lambda: None)
    monkeypatch.setattr(bench, "measure", fake_measure)
    monkeypatch.setattr(bench, "pmc_traffic", lambda *a, **kw: calls.append(("pmc_traffic",)))
    monkeypatch.setattr(bench, "pmc_mfma", lambda *a, **kw: calls.append(("pmc_mfma",)))
    monkeypatch.setattr(bench, "refactor_at", lambda *a, **kw: calls.append(("refactor_at",)))
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **kw: calls.append(("cpu_baseline",)) or {})
    monkeypatch.setattr(bench, "sharded_plain", lambda *a: calls.append(("sharded_plain",)) or 0)
    monkeypatch.setattr(sharded, "bench_main", lambda *a: calls.append(("sharded.bench_main",)) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    assert bench.main() == 0
    out = capsys.readouterr().out.strip().splitlines()
    return calls, (json.loads(out[-1]) if out else None)


def test_plain_run_times_its_steps_and_nothing_else(monkeypatch, capsys):
    calls, line = _main_calls(monkeypatch, capsys, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert calls == [("measure", 8192, 20, 5, 0, 0, False, False, 0, 0)]
    assert set(line) == {"value", "unit", "steps", "warmup", "ms_per_step", "config", "roofline"}
    assert line["roofline"]["traffic"] is None
    # (the --no-* options only trim a --full run; on a plain one they change nothing)
    calls_no, _ = _main_calls(monkeypatch, capsys, "--steps", "20", "--warmup", "5", "--no-late",
                              "--no-secondary", "--no-cpu-baseline", "--no-pmc-traffic", "--no-mfma")
    assert calls_no == calls
    calls, _ = _main_calls(monkeypatch, capsys, "--force-sharded", "--steps", "20", "--warmup", "5")
    assert calls == [("sharded_plain",)]


def test_full_run_measures_everything_the_default_run_used_to(monkeypatch, capsys):
    calls, line = _main_calls(monkeypatch, capsys, "--full", "--steps", "20", "--warmup", "5")
    assert calls == [("pmc_traffic",), ("pmc_mfma",),
                     ("measure", 8192, 20, 5, 20000, 150000, True, True, 400000, 0),
                     ("measure", 32768, 300, 50, 0, 0, False, False, 0, 0),
                     ("measure", 32768, 300, 50, 0, 0, False, False, 0, 16384),
                     ("cpu_baseline",)]
    assert {"secondary", "cpu_baseline"} <= set(line)
    calls, _ = _main_calls(monkeypatch, capsys, "--full", "--steps", "20", "--warmup", "5", "--no-late",
                           "--no-secondary", "--no-cpu-baseline", "--no-pmc-traffic")
    assert calls == [("measure", 8192, 20, 5, 0, 0, False, False, 0, 0)]
    calls, _ = _main_calls(monkeypatch, capsys, "--full", "--force-sharded", "--steps", "20", "--warmup", "5")
    assert calls == [("sharded.bench_main",)]


def test_bench_fails_loudly_without_a_gpu():
    from dantzig_amd import _ffi

    if _ffi.lib().dzg_device_count() > 0:
        import pytest

        pytest.skip("a GPU is visible")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1",
                          "--no-pmc-traffic", "--no-cpu-baseline", "--no-secondary"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode != 0
    assert "no HIP device" in run.stderr or "no CPU" in run.stderr
    assert run.stdout.strip() == ""  # no JSON line is ever printed for a run that measured nothing


def test_profiler_child_is_killed_with_its_whole_process_group(tmp_path):
    """pmc_traffic's children run in their own process group and a timeout ends the group: the
    profiled program is rocprofv3's grandchild and must not outlive it on the GPU."""
    import time

    bench = _bench()
    marker = tmp_path / "grandchild.pid"
    script = ("import os, subprocess, sys, time\n"
              f"p = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(60)'])\n"
              f"open({str(marker)!r}, 'w').write(str(p.pid))\n"
              "time.sleep(60)\n")
    t0 = time.time()
    try:
        bench._run_in_own_group([sys.executable, "-c", script], str(tmp_path), dict(os.environ), 2)
        raise AssertionError("expected a timeout")
    except subprocess.TimeoutExpired:
        pass
    assert time.time() - t0 < 30
    pid = int(marker.read_text())
    for _ in range(50):
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            break
        time.sleep(0.1)
    else:
        raise AssertionError("the grandchild survived the timeout")


def test_cpu_baseline_measures_the_benchmarks_own_lp_when_asked(monkeypatch):
    """cpu_baseline: `value` is the oracle's blocked twin on real pivots of the benchmark's own LP at
    its own size (threads stated), the literal one-core sample stays beside it; without the at-size
    leg the value is the one-core figure carried to the benchmark size.  (Small sizes here: the
    structure of the block, not its numbers.)"""
    monkeypatch.setenv("OMP_NUM_THREADS", "2")
    bench = _bench()
    both = bench.cpu_baseline(128, 256, 1002, 10, 256, 0, (512, 1003, 3))
    assert both["kind"] == "port" and both["cores"] == 2 and both["extrapolated"] is False
    at = both["at_benchmark_size"]
    assert (at["rows"], at["cols"], at["seed"], at["pivots"], at["threads"]) == (256, 512, 1003, 3, 2)
    assert abs(both["value"] - 1.0 / at["seconds_per_pivot"]) <= 1e-12 * both["value"]
    assert both["one_core"]["extrapolated"] is True and both["measured_rows"] == 128
    assert "pivots_equal_the_literal_oracles" not in at  # (no committed fixture for this LP)
    alone = bench.cpu_baseline(128, 256, 1002, 10, 256, 0, None)
    assert alone["cores"] == 1 and alone["extrapolated"] is True and "at_benchmark_size" not in alone
    # beyond 8192 rows a pivot of the reference algorithm takes minutes on any host: no at-size leg
    big = bench.cpu_baseline(128, 256, 1002, 10, 32768, 0, (65536, 1005, 2))
    assert "at_benchmark_size" not in big and big["cores"] == 1


def test_event_stride_rides_in_the_profile_word():
    bench = _bench()
    from dantzig_amd import _ffi

    bench.EVENT_STRIDE = 8
    assert bench.price_profile() == (1 << _ffi.K_PRICE) | (8 << 16)


def _fake_result(m, q, iterations, seed=0):
    import numpy as np

    rng = np.random.default_rng(seed)
    pivots = [(int(rng.integers(0, 3)), int(rng.integers(0, m + q)), int(rng.integers(0, m)), float(rng.normal()))
              for _ in range(iterations)]
    return argparse.Namespace(x=rng.normal(size=m), xbar=rng.normal(size=m), z=rng.normal(size=q),
                              zbar=rng.normal(size=q), basis=rng.permutation(m + q)[:m].astype(np.int64),
                              nonbasis=rng.permutation(m + q)[:q].astype(np.int64), objective=float(rng.normal()),
                              pivots=pivots, margins=rng.uniform(size=iterations), iterations=iterations)


def test_dump_outputs_writes_the_timed_steps_result_in_float64(tmp_path):
    """--dump-outputs: every array a caller of the timed path receives, float64, the pivot log cut to
    the timed steps; indices exact."""
    import numpy as np

    bench = _bench()
    res = _fake_result(m=40, q=70, iterations=25)
    info = bench.dump_outputs(str(tmp_path), res, first_pivot=10)
    names = {"x", "xbar", "z", "zbar", "basis", "nonbasis", "objective", "pivots", "margins"}
    assert set(info["files"]) == {n + ".npy" for n in names} and info["sampled"] is None
    assert {p.name for p in tmp_path.iterdir()} == set(info["files"])
    got = {n: np.load(tmp_path / (n + ".npy")) for n in names}
    assert all(v.dtype == np.float64 for v in got.values())
    for n in ("x", "xbar", "z", "zbar", "margins"):
        want = getattr(res, n)[10:] if n == "margins" else getattr(res, n)
        assert np.array_equal(got[n], want), n
    assert np.array_equal(got["basis"].astype(np.int64), res.basis)
    assert np.array_equal(got["nonbasis"].astype(np.int64), res.nonbasis)
    assert got["objective"].tolist() == [res.objective]
    assert got["pivots"].shape == (15, 4) and got["pivots"].tolist() == [list(p) for p in res.pivots[10:]]
    assert info["timed_pivots"] == 15 and info["bytes"] == sum(v.nbytes for v in got.values())


def test_dump_outputs_samples_a_large_result_into_its_budget(tmp_path):
    """Above the budget every array over its share keeps a fixed, seeded sample of its rows in
    ascending order, positions beside it; the same result gives the same files."""
    import numpy as np

    bench = _bench()
    res = _fake_result(m=3000, q=5000, iterations=2000, seed=1)
    budget = 64 << 10
    a = bench.dump_outputs(str(tmp_path / "a"), res, 0, budget=budget)
    b = bench.dump_outputs(str(tmp_path / "b"), res, 0, budget=budget)
    assert a["files"] == b["files"] and a["bytes"] == b["bytes"] <= budget
    assert sum((tmp_path / "a" / f).stat().st_size for f in a["files"]) <= budget
    assert set(a["sampled"]) >= {"x", "z", "zbar", "pivots"} and "objective" not in a["sampled"]
    for f in a["files"]:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    for name in a["sampled"]:
        idx = np.load(tmp_path / "a" / f"{name}_index.npy").astype(np.int64)
        assert np.all(np.diff(idx) > 0) and idx[-1] < a["sampled"][name]["rows"]
        full = np.asarray(res.pivots if name == "pivots" else getattr(res, name), dtype=np.float64)
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), full[idx]), name


@pytest.mark.gpu
def test_bench_dumps_the_timed_paths_outputs_the_same_on_every_run(tmp_path):
    """bench.py --steps K --dump-outputs DIR: exactly K timed pivots, `ms_per_step` in the line, and
    the files are what a Solver on the same seeded LP returns after the same warm-up + K pivots --
    bit for bit, and the same from one run to the next."""
    import json

    import numpy as np

    from dantzig_amd import core

    rows, cols, seed, steps, warmup = 256, 512, 1003, 40, 10
    lines = []
    for run_dir in ("a", "b"):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps),
                              "--warmup", str(warmup), "--rows", str(rows), "--cols", str(cols), "--seed", str(seed),
                              "--no-pmc-traffic", "--no-cpu-baseline", "--no-secondary", "--no-late",
                              "--dump-outputs", str(tmp_path / run_dir)],
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        lines.append(json.loads(run.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
        assert line["dump_outputs"]["timed_pivots"] == steps and line["dump_outputs"]["sampled"] is None
    files = lines[0]["dump_outputs"]["files"]
    assert files == lines[1]["dump_outputs"]["files"]
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f), equal_nan=True), f

    a, b, c = core.gen_dense_lp(seed=seed, m=rows, n_struct=cols)
    with core.Solver(core.CoreLP.from_inequality_form(a, b, c), numerics=core.FAST, poll_interval=50) as s:
        assert s.run(warmup) == "iter_limit" and s.run(steps) == "iter_limit"
        want = s.result()
    assert want.iterations == warmup + steps
    for name in ("x", "xbar", "z", "zbar", "basis", "nonbasis"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), getattr(want, name).astype(np.float64)), name
    assert np.load(tmp_path / "a" / "objective.npy").tolist() == [want.objective]
    assert np.load(tmp_path / "a" / "pivots.npy").tolist() == [list(map(float, p)) for p in want.pivots[warmup:]]


@pytest.mark.gpu
def test_plain_bench_line_is_the_timed_steps_alone():
    """bench.py --steps K --warmup W without --full: the headline line of exactly K timed pivots, its
    pricing roofline from the same pivots, and none of what --full adds."""
    import json

    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40",
                          "--warmup", "10", "--rows", "256", "--cols", "512"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "simplex_iterations_per_sec" and line["unit"] == "iterations/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 40 and line["warmup"] == 10 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"]["launches"] == 40 and line["roofline"]["traffic"] is None
    assert not {"late", "deep", "end", "mfma", "whole_solve", "secondary", "cpu_baseline"} & set(line)
