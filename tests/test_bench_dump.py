"""bench.py --dump-outputs: the last timed step's output records land on disk exactly, within the size budget, and two runs with
the same arguments write the same sample; --steps is validated before any work starts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _words(rows, cols, seed=3):
    w = np.random.default_rng(seed).integers(-2**31, 2**31, (rows, cols), dtype=np.int64).astype(np.int32)
    w[0, 0], w[0, 1] = -2**31, 2**31 - 1
    return w


def test_dump_small_batch_is_whole_and_exact(tmp_path):
    out = _words(16, 631)
    bench.dump_outputs(str(tmp_path), "nand_out", out)
    got = np.load(tmp_path / "nand_out.npy")
    assert got.dtype == np.float64 and got.shape == out.shape
    assert np.array_equal(got.astype(np.int64), out.astype(np.int64))
    assert not (tmp_path / "nand_out_rows.npy").exists()


def test_dump_large_batch_is_a_seeded_sample_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 200_000)
    out = _words(1000, 631)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "nand_out", out)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    rows = np.load(tmp_path / "a" / "nand_out_rows.npy").astype(np.int64)
    got = np.load(tmp_path / "a" / "nand_out.npy")
    assert 0 < rows.size < out.shape[0] and np.all(np.diff(rows) > 0)
    assert np.array_equal(got.astype(np.int64), out[rows].astype(np.int64))
    for f in ("nand_out.npy", "nand_out_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    bench.dump_outputs(str(tmp_path / "a"), "nand_out", out[:4])   # a whole batch into the same directory: no stale row indices
    assert not (tmp_path / "a" / "nand_out_rows.npy").exists()
    assert np.load(tmp_path / "a" / "nand_out.npy").shape == (4, 631)


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_bad_step_counts(flags):
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *flags], capture_output=True, text=True, timeout=120)
    assert pr.returncode != 0 and "--steps must be >= 1" in pr.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_on_device(tmp_path):
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "256",
                         "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr[-2000:]
    res = json.loads(pr.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["bit_exact_decrypt_errors"] == 0
    got = np.load(tmp_path / "nand_out.npy")
    assert got.dtype == np.float64 and got.shape == (256, 631)
    assert np.all(got == np.round(got)) and got.min() >= -2**31 and got.max() < 2**31
