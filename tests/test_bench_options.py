"""bench.py's command line without a GPU (the stand-in decoder of LVA_BENCH_STUB, honoured only with LVA_TESTING): a plain run
times exactly --steps steps and prints the headline line without the legs that `--full` adds; --dump-outputs writes the lists of
the last timed step as float32 .npy files, the same on every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = dict(os.environ, LVA_BENCH_STUB="1", LVA_TESTING="1", OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LVA_BENCH_SPAWN", "LVA_FORCE_DIST"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    small = ["--steps", "3", "--warmup", "1", "--reads-per-step", "7", "--pool", "20", "--list-size", "4", "--msg-len", "12"]
    j = _run(small + ["--dump-outputs", str(tmp_path / "a"), "--dump-lists", str(tmp_path / "a.npz")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 3 and len(j["config"]["step_ms_rank0"]) == 3 and j["ms_per_step"] > 0
    assert j["value"] > 0 and j["unit"] == "reads/s" and j["higher_is_better"] is True
    for k in ("cpu_baseline", "cpu_baseline_single_thread", "extra_configs"):
        assert k not in j, k
    assert "cross_check" not in j["config"] and "reference_checked_reads" not in j["config"]
    z = np.load(str(tmp_path / "a.npz"))
    out = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in ("counts", "msgs", "scores", "read_index")}
    assert all(v.dtype == np.float32 for v in out.values())
    assert out["msgs"].shape == (7, 4, 12) and out["scores"].shape == (7, 4)
    for k in ("counts", "msgs", "scores"):
        assert np.array_equal(out[k], z[k].astype(np.float32)), k
    assert np.array_equal(out["read_index"], np.arange(7, dtype=np.float32))
    # 1 warm-up + 3 timed steps over the pool's 3 batches of 7 reads: the last step is batch 0 again (reads 0..6, one error code)
    n = np.array([3 + (gi * 7919) % 57 for gi in range(7)])
    assert np.array_equal(out["counts"], np.where(n < 5, -6, 1 + n % 4).astype(np.float32))
    # the same arguments again: the same outputs
    _run(small + ["--dump-outputs", str(tmp_path / "b")])
    for k in out:
        assert np.array_equal(np.load(str(tmp_path / "b" / (k + ".npy"))), out[k]), k


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    """More lists than fit in the limit: a sorted sample of the reads, drawn with a fixed seed, and their global indices."""
    sys.path.insert(0, ROOT)
    import bench
    L, ml, n = 4, 12, 1000
    gathered = [-6 if i % 7 == 0 else (np.full((1 + i % L, ml), i & 1, np.uint8), -np.arange(1 + i % L, dtype=np.float32) - i)
                for i in range(n)]
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4 * (2 + L + L * ml) * 100 + 4096)
    bench.dump_outputs(str(tmp_path / "a"), gathered, L, ml)
    bench.dump_outputs(str(tmp_path / "b"), gathered, L, ml)
    out = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in ("counts", "msgs", "scores", "read_index")}
    idx = out["read_index"].astype(np.int64)
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in out) <= bench.DUMP_LIMIT
    for j, i in enumerate(idx):
        want = -6 if i % 7 == 0 else 1 + i % L
        assert out["counts"][j] == want
        if want > 0:
            assert np.array_equal(out["scores"][j, :want], gathered[i][1]) and np.all(out["msgs"][j, :want] == (i & 1))
    for k in out:
        assert np.array_equal(np.load(str(tmp_path / "b" / (k + ".npy"))), out[k]), k
