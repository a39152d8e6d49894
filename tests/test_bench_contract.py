"""bench.py's one-line JSON contract (the driver parses it), checked on a GPU: single process, plain and --full, and
the N = 2 control flow with bench.py starting its own ranks (both ranks on cuda:0, exchange over gloo: rehearsal only)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}
REQUIRED = HEADLINE | {"roofline", "strong"}  # --full
FULL_ONLY = {"roofline", "strong", "kernel_checks_per_s", "shard_probe", "two_streams", "cpu_baseline"}


def _run(*args):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=900,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_single_gpu(tmp_path):
    d = _run("--full", "--steps", "10", "--warmup", "3", "--cpu-sample", "65536", "--dump-outputs", str(tmp_path / "full"))
    assert REQUIRED <= set(d) and "cpu_baseline" in d
    assert d["n_gpus"] == 1 and d["steps"] == 10 and d["warmup"] == 3 and d["scaling"] == "weak" and d["dtype"] == "f32"
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["higher_is_better"] is True
    assert "workload" in d["config"] and "model" not in d["config"]
    roof = d["roofline"]
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(roof) and roof["bound"] == "hbm"
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12 and roof["kernel_ms"] <= d["ms_per_step"]
    assert abs(d["value"] - d["config"]["configs_per_gpu"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    cpu = d["cpu_baseline"]
    assert {"value", "unit", "cores", "kind", "sample"} <= set(cpu) and cpu["kind"] in ("port", "reference")
    assert 0.55 < d["config"]["valid_fraction"] < 0.70
    assert d["value"] > 1e8  # the north-star floor, by a wide margin
    two = d["two_streams"]  # informational leg: the same steps on two alternating streams, never `value`
    assert two["same_words_as_the_timed_run"] is True and two["value"] > 0 and two["unit"] == d["unit"]
    probe = d["shard_probe"]["shards"]  # the N = 2, 4, 8 shards of the 1M job timed on this GPU
    assert set(probe) == {"2", "4", "8"} and probe["8"]["configs"] == d["config"]["configs_per_gpu"] // 8
    assert all(p["ms_per_step"] > 0 and 0.5 < p["ceiling"] <= int(k) * 1.5 for k, p in probe.items())
    short = _run("--full", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-two-streams", "--no-shard-probe")
    assert "two_streams" not in short and "shard_probe" not in short
    # a plain run: the headline figure only, over the same seeded inputs
    plain = _run("--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path / "plain"))
    assert HEADLINE <= set(plain) and not FULL_ONLY & set(plain)
    assert plain["steps"] == 5 and plain["warmup"] == 2 and plain["dtype"] == "f32" and plain["higher_is_better"] is True
    assert abs(plain["value"] - plain["config"]["configs_per_gpu"] / (plain["ms_per_step"] * 1e-3)) / plain["value"] < 1e-6
    assert plain["config"]["valid_fraction"] == d["config"]["valid_fraction"]
    # --dump-outputs: the booleans of the last timed step, identical from run to run
    outs = [np.load(tmp_path / run / "valid.npy") for run in ("full", "plain")]
    assert all(v.dtype == np.float32 and v.shape == (d["config"]["configs_per_gpu"],) for v in outs)
    assert set(np.unique(outs[0])) <= {0.0, 1.0} and float(outs[0].mean(dtype=np.float64)) == d["config"]["valid_fraction"]
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.gpu
def test_bench_starts_its_own_ranks_and_reports_weak_and_strong():
    d = _run("--full", "--gpus", "2", "--rehearse-on-one-gpu", "--steps", "6", "--warmup", "2")
    assert REQUIRED <= set(d) and d["n_gpus"] == 2 and "cpu_baseline" not in d and "two_streams" not in d
    assert d["strong"]["configs_per_job"] == d["config"]["configs_per_gpu"] and d["strong"]["value"] > 0
    assert abs(d["value"] - 2 * d["config"]["configs_per_gpu"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


def test_dump_outputs_ranks_and_sampling(vamp, tmp_path, monkeypatch):
    """--dump-outputs without a GPU: every rank's n booleans in rank order (the padding bits of each rank's last word
    dropped), and above the size limit a seeded sample with its positions, together within the limit."""
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.DUMP_SAMPLE * (4 + 8) <= bench.DUMP_LIMIT_BYTES
    n, ranks = 1000, 3  # n is not a multiple of 64
    per = (n + 63) // 64
    words = np.random.default_rng(5).integers(0, np.iinfo(np.uint64).max, per * ranks, dtype=np.uint64, endpoint=True)
    want = np.unpackbits(words.view(np.uint8), bitorder="little").reshape(ranks, per * 64)[:, :n].ravel()

    bench.dump_outputs(str(tmp_path / "whole"), words, n, ranks)
    v = np.load(tmp_path / "whole" / "valid.npy")
    assert v.dtype == np.float32 and np.array_equal(v, want.astype(np.float32))
    assert not (tmp_path / "whole" / "valid_index.npy").exists()

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8000)  # 3,000 booleans = 12,000 bytes: sampled
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 600)
    runs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), words, n, ranks)
        runs.append((np.load(tmp_path / d / "valid.npy"), np.load(tmp_path / d / "valid_index.npy")))
    (v, idx), (v2, idx2) = runs
    assert v.dtype == np.float32 and idx.dtype == np.float64 and v.shape == idx.shape == (600,)
    assert v.nbytes + idx.nbytes <= 8000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n * ranks and np.array_equal(idx, np.round(idx))
    assert np.array_equal(v, want[idx.astype(np.int64)].astype(np.float32))
    assert np.array_equal(v, v2) and np.array_equal(idx, idx2)
