"""bench.py's launcher contract on a box without GPUs: `--gpus N` must start N ranks or fail loudly (never run one
rank and report it as N), and a launcher-provided WORLD_SIZE that disagrees with --gpus is an error."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True,
                          text=True, timeout=300)


def test_gpus_n_without_enough_devices_fails_loudly():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("box has GPUs")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "--gpus 2" in r.stderr and "GPU" in r.stderr
    assert r.stdout.strip() == ""  # no JSON line claiming n_gpus


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "4"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in (r.stderr + r.stdout)


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_headline_is_the_last_line_and_small():
    """Round 5's single 23.5 KB line was cut by the driver's stdout tail (`parsed: null`).  Feed the line builder that
    very result set (profiles/r05_bench_line.json, prose and all, plus a failing secondary): the last line must be the
    headline, parse, stay under 4 KB and carry `roofline` + `cpu_baseline`; every secondary gets its own short line."""
    import json
    bench = _load_bench()
    with open(os.path.join(ROOT, "profiles", "r05_bench_line.json")) as fh:
        full = json.load(fh)
    secondary = full.pop("secondary") + [{"workload": "c3", "error": "RuntimeError: " + "x" * 5000}]
    full["config"]["step"] = "prose " * 400  # whatever a workload writes there must not reach the headline
    full["detail"] = "gpurun_out/bench_detail.json"
    lines = bench.output_lines(full, secondary)
    assert len(lines) == len(secondary) + 1
    head = lines[-1]
    assert "\n" not in head and len(head) < 4096 == bench.HEADLINE_LIMIT
    parsed = json.loads(head)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in parsed, key
    assert "secondary" not in parsed
    assert parsed["value"] == full["value"] and parsed["ms_per_step"] == full["ms_per_step"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in parsed["roofline"], key
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in parsed["cpu_baseline"], key
    assert parsed["config"]["workload"].startswith("DiffPool") and "step" not in parsed["config"]
    for text, sec in zip(lines[:-1], secondary):
        one = json.loads(text)
        assert "\n" not in text and len(text) < 2048, (sec["workload"], len(text))
        assert one["secondary"] == sec["workload"]
        if "error" not in sec:
            assert one["roofline"]["frac"] == sec["roofline"]["frac"] and one["ms_per_step"] == sec["ms_per_step"]


def test_plain_headline_carries_the_contract_fields():
    """A plain run (no --full) has no windows, roofline or CPU baseline: its line must still build and parse."""
    import json
    bench = _load_bench()
    line = {"metric": bench.METRIC, "value": 1.0e8, "unit": "nodes/s", "n_gpus": 1, "steps": 20, "warmup": 5,
            "settle_steps": 700, "ms_per_step": 0.09, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic", "config": {"workload": "DiffPool", "step": "prose " * 100}}
    parsed = json.loads(bench.headline_text(line))
    assert {k: parsed[k] for k in line if k != "config"} == {k: v for k, v in line.items() if k != "config"}
    assert parsed["config"] == {"workload": "DiffPool"} and "roofline" not in parsed


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path):
    """--dump-outputs: float32 for narrow types, float64 for int64 indices (exact), None entries skipped; above the
    byte budget every array keeps the same fraction of its elements, the same ones in every run, in index order."""
    import numpy as np
    import torch
    bench = _load_bench()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 4, generator=g)
    info = bench.dump_outputs(str(tmp_path / "a"), {"x": x, "ei": torch.arange(10).view(2, 5), "none": None,
                                                   "mask": torch.tensor([True, False])})
    assert info == {"dir": str(tmp_path / "a"), "arrays": 3, "sampled": False}
    assert sorted(os.listdir(tmp_path / "a")) == ["ei.npy", "mask.npy", "x.npy"]
    got = np.load(tmp_path / "a" / "x.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    ei = np.load(tmp_path / "a" / "ei.npy")
    assert ei.dtype == np.float64 and np.array_equal(ei, np.arange(10).reshape(2, 5))
    assert np.load(tmp_path / "a" / "mask.npy").tolist() == [1.0, 0.0]

    big = {"a": torch.arange(1000, dtype=torch.float32), "b": torch.arange(500)}  # 4000 + 4000 bytes
    for d in ("s1", "s2"):
        assert bench.dump_outputs(str(tmp_path / d), big, limit=2000)["sampled"]
    a1, a2 = np.load(tmp_path / "s1" / "a.npy"), np.load(tmp_path / "s2" / "a.npy")
    assert a1.shape == (250,) and np.load(tmp_path / "s1" / "b.npy").shape == (125,)
    assert np.array_equal(a1, a2) and (np.diff(a1) > 0).all()
    assert bench.DUMP_LIMIT <= 64_000_000
