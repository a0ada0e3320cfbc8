"""bench.py's plain run and --dump-outputs: a plain run times exactly --steps steps and prints the headline line only (the
roofline passes, bf16x3 figure, MPC iteration and CPU baseline run with --full); --dump-outputs writes what the last timed
step returned, float32, identical from run to run with the same arguments."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writes_everything_within_the_budget(tmp_path):
    import bench
    rewards = np.arange(16, dtype=np.float32)
    seqs = torch.arange(16 * 2 * 5 * 3, dtype=torch.float32).reshape(16, 2, 5, 3)
    bench.dump_outputs(str(tmp_path), rewards, seqs)
    assert sorted(os.listdir(tmp_path)) == ["rewards.npy", "state_seqs.npy"]
    assert np.array_equal(np.load(tmp_path / "rewards.npy"), rewards)
    got = np.load(tmp_path / "state_seqs.npy")
    assert got.dtype == np.float32 and np.array_equal(got, seqs.numpy())


def test_dump_outputs_samples_a_fixed_subset_beyond_the_budget(tmp_path, monkeypatch):
    import bench
    rewards = np.zeros(64, np.float32)
    seqs = torch.randn(64, 2, 100, 3)                      # 2,400 B per candidate
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 4096 + 256 + 20 * 2408)
    ids = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rewards, seqs)
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["rewards.npy", "state_seqs.npy", "state_seqs_candidates.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= bench.DUMP_BYTES
        ids.append(np.load(tmp_path / d / "state_seqs_candidates.npy"))
        got = np.load(tmp_path / d / "state_seqs.npy")
        assert got.dtype == np.float32 and got.shape == (20, 2, 100, 3)
        assert np.array_equal(got, seqs.numpy()[ids[-1].astype(np.int64)])
    assert ids[0].dtype == np.float64 and np.array_equal(ids[0], ids[1]) and np.all(np.diff(ids[0]) > 0)


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                             "AG_BENCH_FORCE_DIST", "AG_BENCH_BACKEND", "AG_BENCH_SHARE_GPU")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--candidates", "64", "--side", "20",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 1, p.stdout[-3000:]
    return json.loads(rows[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_its_outputs(tmp_path):
    line = _plain_run(tmp_path / "a")
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["metric"] == "rollout-steps/sec" and line["unit"] == "rollout-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32"
    assert abs(line["value"] - 64 * 20 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for k in ("roofline", "roofline_second_kernel", "cpu_baseline", "parity_check", "bf16x3_mode", "end_to_end"):
        assert k not in line, k
    rewards = np.load(tmp_path / "a" / "rewards.npy")
    seqs = np.load(tmp_path / "a" / "state_seqs.npy")
    assert rewards.dtype == np.float32 and rewards.shape == (64,) and np.isfinite(rewards).all()
    assert seqs.dtype == np.float32 and seqs.shape == (64, 2, 400, 3) and np.isfinite(seqs).all()
    assert hashlib.sha256(rewards.tobytes()).hexdigest() == line["reward_sha256"]
    # same arguments, same inputs: the outputs of a second run are bit-equal
    again = _plain_run(tmp_path / "b")
    assert again["reward_sha256"] == line["reward_sha256"]
    assert np.array_equal(np.load(tmp_path / "b" / "state_seqs.npy"), seqs)
