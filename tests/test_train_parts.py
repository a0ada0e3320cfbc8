"""CPU checks of an optimiser step built from parts (TrainStep.accumulate / apply / step_parts, ag_train_step_part): the rule
itself - every part's MSE divided by the row count of the WHOLE step, the shares summed - on the reference's data in float64
(tests/train_restate.py), independent of any kernel; the export at the boundary; and the host bookkeeping
(adaptigraph_amd.train_step.StepParts), which raises every argument error before a GPU call is made."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import train_restate as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_GRAPH = ("state", "attrs", "action", "p_instance", "physics_param", "state_future", "eef_future", "action_future", "n_edges")


def sub_fixture(f, idx):
    """The graphs `idx` of a training fixture, as a fixture of its own (per-graph arrays sliced, edge lists re-concatenated)."""
    idx = np.asarray(idx)
    off = np.concatenate([[0], np.cumsum(f["n_edges"])])
    g = dict(f)
    for k in PER_GRAPH:
        g[k] = f[k][idx]
    g["recv"] = np.concatenate([f["recv"][off[b]:off[b + 1]] for b in idx])
    g["send"] = np.concatenate([f["send"][off[b]:off[b + 1]] for b in idx])
    return g


def splits(sizes):
    """[2, 2] -> [[0, 1], [2, 3]]"""
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [list(range(edges[i], edges[i + 1])) for i in range(len(sizes))]


def _f64_loss_and_grads(f, scale=1.0):
    inp = TR.fixture_inputs(f, torch.float64)
    B, N = inp["attrs"].shape[:2]
    recv, send = TR.fixture_edges(f, B, N)
    W = TR.weights(f, torch.float64)
    step = lambda s, a: TR.forward(W, s, inp["attrs"], a, inp["phys"], inp["group"], recv, send, inp["n_p"],  # noqa: E731
                                   int(f["pstep"]))
    loss = TR.chain_loss(step, inp, int(f["n_future"])) * scale
    loss.backward()
    return loss.item(), {k: W[k].grad.numpy() for k in TR.KEYS}


@pytest.mark.parametrize("name,sizes", [("train_rope.npz", [2, 2]), ("train_rope.npz", [3, 1]), ("train_cloth.npz", [1, 1, 1])])
def test_shares_of_the_parts_sum_to_the_one_batch_values_in_float64(name, sizes):
    f = TR.load_fixture(name)
    B = f["attrs"].shape[0]
    assert sum(sizes) == B
    loss, g = _f64_loss_and_grads(f)
    loss_p, g_p = 0.0, {k: 0.0 for k in TR.KEYS}
    for idx in splits(sizes):
        # MSELoss of a part is a mean over len(idx) * n_p * 3; the same sum over B * n_p * 3 is that mean times len(idx) / B
        lp, gp = _f64_loss_and_grads(sub_fixture(f, idx), scale=len(idx) / B)
        loss_p += lp
        for k in TR.KEYS:
            g_p[k] = g_p[k] + gp[k]
    assert abs(loss_p - loss) <= 1e-12 * abs(loss), (loss_p, loss)
    for k in TR.KEYS:
        err = np.abs(g_p[k] - g[k]).max()
        assert err <= 1e-12 * np.abs(g[k]).max(), (k, err, np.abs(g[k]).max())


def test_part_entry_is_declared_exported_and_never_waits():
    hdr = open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    whole = re.search(r"\bint ag_train_step\s*\((.*?)\);", src, flags=re.S).group(1)
    part = re.search(r"\bint ag_train_step_part\s*\((.*?)\);", src, flags=re.S).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]   # noqa: E731
    assert norm(part) == norm(whole) + ["int32_t B_total", "int32_t accumulate"]     # every argument of ag_train_step, same order
    assert src.rindex("ag_train_step_part") > max(src.rindex(n) for n in ("ag_mppi_clip", "ag_ctx_reset_stats"))   # appended
    table = hdr[hdr.index("WHICH ENTRY POINTS BLOCK THE HOST"):hdr.index("#ifndef ADAPTIGRAPH_AMD_H")]
    row = [ln for ln in table.splitlines() if "ag_train_step_part" in ln]
    assert len(row) == 1 and "NEVER" in row[0]
    from adaptigraph_amd import _lib
    assert "ag_train_step_part" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T ag_train_step_part$", out, flags=re.M)
    lib = _lib.load()
    assert list(lib.ag_train_step_part.argtypes[:-2]) == list(lib.ag_train_step.argtypes)


def test_bookkeeping_of_a_step_raises_before_anything_runs():
    from adaptigraph_amd.train_step import StepParts
    p = StepParts()
    assert not p.open
    with pytest.raises(ValueError, match="no part"):
        p.close()
    assert p.add(3, 4) == (4, False) and p.open                  # the first part overwrites
    with pytest.raises(ValueError, match="total is required"):
        p.add(1)
    with pytest.raises(ValueError, match="differs"):             # a changing total
        p.add(1, 5)
    with pytest.raises(RuntimeError, match="inside an open step"):   # step() inside an open step
        p.forbid_open("step")
    with pytest.raises(ValueError, match="total is 4"):          # more rows than promised
        p.add(2, 4)
    assert (p.rows, p.parts) == (3, 1)                           # a refused part leaves the step as it was
    with pytest.raises(ValueError, match="hold 3 rows"):         # rows that do not sum to total
        p.close()
    assert p.add(1, 4) == (4, True)                              # later parts accumulate
    p.close()
    assert not p.open
    p.forbid_open("step")
    assert p.add(2) == (2, False)                                # a one-part step: total defaults to its rows
    p.close()
    with pytest.raises(ValueError, match="0 rows"):
        p.add(0, 4)
    # a step that spans ranks: this rank holds a share of the total, never more
    r = StepParts(spans_ranks=True)
    assert r.add(2, 4) == (4, False)
    r.close()
    r.add(2, 4)
    with pytest.raises(ValueError):
        r.add(3, 4)


def test_part_methods_sit_next_to_step_and_a_cpu_model_still_raises():
    """TrainStep's accumulate / apply / step_parts exist next to step(); a CPU model still raises (no fallback)."""
    import adaptigraph_amd as ag
    for name in ("accumulate", "apply", "step_parts", "step", "evaluate"):
        assert callable(getattr(ag.TrainStep, name))
    from test_train_step import _cpu_model
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.TrainStep(_cpu_model(), group=None, global_rows=4)
