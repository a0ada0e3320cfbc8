"""Data-parallel TrainStep on the GPU (-m gpu), children only (tools/train_ranks.py), each under `timeout`: two ranks on the one
GPU of the box over gloo (RCCL refuses two ranks on one device), each with two graphs of train_rope, against one process with all
four; an overflow on one rank only; and a world of ONE rank on nccl (= RCCL), which executes apply()'s three collectives on the
hardware that exists.  RCCL with more than one rank has never run (no multi-GPU node): DESIGN.md section 3.14.  At most three
processes hold the GPU at once (this one and two ranks); after a child that aborted, faulted or timed out nothing more is started."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import train_restate as TR
from test_train import grad_tol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "train_ranks.py")
_FATAL = []


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _child(env, ranks=1, seconds=240):
    """One run of the rank script -> its JSON line.  ranks > 1: through torch.distributed.run."""
    if _FATAL:
        pytest.fail(f"an earlier child ended with {_FATAL[0]}: no further child is started")
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("AG_TRAIN_", "AG_BENCH_")) and k not in (
        "RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    port = str(_free_port())
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable]
    if ranks > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                "--master-port", port]
    r = subprocess.run(cmd + [TOOL], env=dict(clean, MASTER_PORT=port, **env), cwd=ROOT, capture_output=True, text=True)
    if r.returncode in (134, 139, 124, 137, -6, -11):
        _FATAL.append(r.returncode)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"train_ranks"' in ln]
    assert len(rows) == 1, r.stdout[-3000:]
    return json.loads(rows[0])


def test_two_ranks_on_one_gpu_train_like_one_process(tmp_path):
    dump = str(tmp_path / "grads_step1.npz")
    two = _child(dict(AG_BENCH_SHARE_GPU="1", AG_BENCH_BACKEND="gloo", AG_TRAIN_STEPS="3", AG_TRAIN_DUMP=dump), ranks=2)
    one = _child(dict(AG_TRAIN_STEPS="3"))
    assert two["world"] == 2 and two["backend"] == "gloo" and one["world"] == 1 and one["backend"] is None
    r0, r1 = two["ranks"]
    assert (r0["graphs"], r1["graphs"]) == ([0, 1], [2, 3]) and one["ranks"][0]["graphs"] == [0, 1, 2, 3]
    # identical weights on both ranks before the first and after every step, and they move
    assert r0["weights_sha256"] == r1["weights_sha256"] and len(set(r0["weights_sha256"])) == 4
    assert r0["weights_sha256"][0] == one["ranks"][0]["weights_sha256"][0]
    assert r0["losses"] == r1["losses"]                              # the loss vector is all-reduced: one value everywhere
    assert not r0["check_raised"] and not r1["check_raised"] and r0["applied_steps"] == r1["applied_steps"] == 3
    print("two ranks", r0["losses"], "one process", one["ranks"][0]["losses"])
    np.testing.assert_allclose(r0["losses"], one["ranks"][0]["losses"], rtol=1e-4)
    f = TR.load_fixture("train_rope.npz")
    np.testing.assert_allclose(r0["losses"], f["adam_losses"][:3], rtol=1e-3)
    g = np.load(dump)
    bad = []
    for k in TR.KEYS:
        err = np.abs(g[k] - f["g::" + k]).max()
        print(f"  {k}: two-rank gradient vs reference {err:.3e} (bar {grad_tol(f, k):.3e})")
        if not err <= grad_tol(f, k):
            bad.append((k, float(err)))
    assert not bad, bad


def test_overflow_on_one_rank_skips_the_step_on_every_rank():
    two = _child(dict(AG_BENCH_SHARE_GPU="1", AG_BENCH_BACKEND="gloo", AG_TRAIN_STEPS="2", AG_TRAIN_OVERFLOW_RANK="1"), ranks=2)
    r0, r1 = two["ranks"]
    assert r0["check_raised"] and r1["check_raised"]
    assert r0["applied_steps"] == r1["applied_steps"] == 1 and r0["host_step_counter"] == r1["host_step_counter"] == 1
    for r in (r0, r1):
        sha = r["weights_sha256"]
        assert sha[0] != sha[1] and sha[2] == sha[1]                 # step 1 applied, step 2 skipped: the pre-step weights
    assert r0["weights_sha256"] == r1["weights_sha256"]


def test_world_of_one_on_rccl_equals_no_group_and_does_not_wait():
    plain = _child(dict(AG_TRAIN_STEPS="3", AG_TRAIN_PARTS="2"))
    rccl = _child(dict(AG_TRAIN_STEPS="3", AG_TRAIN_PARTS="2", AG_BENCH_FORCE_DIST="1", AG_BENCH_BACKEND="nccl", AG_TRAIN_SPIN="1"))
    assert rccl["backend"] == "nccl" and rccl["world"] == 1 and plain["backend"] is None
    a, b = plain["ranks"][0], rccl["ranks"][0]
    assert a["losses"] == b["losses"] and a["weights_sha256"] == b["weights_sha256"]
    assert b["applied_steps"] == 3 and not b["check_raised"]
    print(f"RCCL world of one: a step's enqueues take {b['host_ms_of_a_step']:.2f} ms on the host, spin {b['spin_ms']:.0f} ms")
    assert b["returned_while_busy"], "apply() with its three collectives waited for the GPU"
