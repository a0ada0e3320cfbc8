"""GPU checks (-m gpu) of an optimiser step built from parts: ag_train_step_part through TrainStep.accumulate / apply /
step_parts against the one-call step (bits where the arithmetic is the same, the reference's bars where the summation order
differs), the status protocol across parts, and that nothing waits.  Fixtures: tests/golden/train_*.npz.  Every test prints
the figures it asserts on."""
import time

import numpy as np
import pytest
import torch

import train_restate as TR
from test_train import grad_tol
from test_train_parts import splits
from test_gpu_train import _f64_grads
from test_gpu_train_step import _data, _train_step, _max_edges
from test_gpu_parity import POS_TOL

pytestmark = pytest.mark.gpu
_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _fixture(name):
    """fixture, its float64 gradients and the one-call step's results (computed once, never written to)"""
    if name not in _REF:
        f = TR.load_fixture(name)
        _REF[name] = {"f": f, "g64": _f64_grads(f)[0]}
    return _REF[name]


def _one_call(dev, name, **kw):
    r = _fixture(name)
    key = ("one", tuple(sorted(kw.items())))
    if key not in r:
        ts, _ = _train_step(dev, r["f"], **kw)
        data = _data(r["f"], dev)
        loss = ts.step(data, max_edges=_max_edges(data))
        ts.check()
        r[key] = dict(loss=loss.clone(), pred=ts.last_pred.clone(), grad=[g.clone() for g in ts.grad], w=[w.clone() for w in ts.w])
    return r[key]


def _parts(f, dev, sizes):
    out = [_data(f, dev, idx=idx) for idx in splits(sizes)]
    return out, [_max_edges(d) for d in out]


def _meets_fixture_bars(name, loss, grads, one=None):
    """The bars of tests/test_gpu_train_step.py::test_fused_gradients_match_reference, unchanged."""
    r = _fixture(name)
    f, g64 = r["f"], r["g64"]
    print(name, "loss", loss, "reference", float(f["loss_sum"]))
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"])) + 1e-7
    g = {k: t.cpu().numpy() for k, t in zip(TR.KEYS, grads)}
    bad, worst = [], 0.0
    for i, k in enumerate(TR.KEYS):
        ref = f["g::" + k]
        err = np.abs(g[k] - ref).max()
        e64 = np.abs(g[k] - g64[k]).max()
        line = f"  {k}: vs reference {err:.3e} (bar {grad_tol(f, k):.3e}), vs float64 {e64:.3e}"
        if one is not None:
            d = float((grads[i] - one["grad"][i]).abs().max())
            worst = max(worst, d / grad_tol(f, k))
            line += f", parts vs one call {d:.3e}"
        print(line)
        if not err <= grad_tol(f, k):
            bad.append((k, "vs reference", float(err), float(np.abs(ref).max())))
        if "err64::" + k in f and not e64 <= 4 * float(f["err64::" + k]) + 1e-7 * np.abs(g64[k]).max():
            bad.append((k, "vs float64", float(e64), float(f["err64::" + k])))
    if one is not None:
        print(f"  worst parts-vs-one-call difference: {worst:.3e} of its tensor's bar")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 1. one part = ag_train_step
def test_one_part_step_has_the_bits_of_step(dev):
    f = _fixture("train_rope.npz")["f"]
    one = _one_call(dev, "train_rope.npz")
    ts, _ = _train_step(dev, f)
    data = _data(f, dev)
    share = ts.accumulate(data, max_edges=_max_edges(data), total=data["state"].shape[0])
    loss = ts.apply()
    ts.check()
    assert torch.equal(share, loss) and torch.equal(loss, one["loss"])
    assert isinstance(ts.last_pred, list) and len(ts.last_pred) == 1 and torch.equal(ts.last_pred[0], one["pred"])
    for k, (a, b) in enumerate(zip(ts.grad, one["grad"])):
        assert torch.equal(a, b), TR.KEYS[k]
    for k, (a, b) in enumerate(zip(ts.w, one["w"])):
        assert torch.equal(a, b), TR.KEYS[k]
    # the 22 gradients are views into one buffer, in order
    flat = ts._grad_flat
    ptrs = [g.data_ptr() for g in ts.grad]
    assert ptrs == sorted(ptrs) and ptrs[0] == flat.data_ptr() and ptrs[-1] + ts.grad[-1].numel() * 4 <= flat.data_ptr() + flat.numel() * 4
    assert all(g.is_contiguous() and g.shape == w.shape for g, w in zip(ts.grad, ts.w))


# ------------------------------------------------------------------------------------------------ 2. parts against the reference
@pytest.mark.parametrize("name,sizes", [("train_rope.npz", [2, 2]), ("train_rope.npz", [3, 1]), ("train_rope.npz", [1, 1, 1, 1]),
                                        ("train_cloth.npz", [2, 1])])
def test_accumulated_parts_meet_the_reference_bars(dev, name, sizes):
    f = _fixture(name)["f"]
    one = _one_call(dev, name, lr=0.0)
    ts, _ = _train_step(dev, f, lr=0.0)
    parts, bounds = _parts(f, dev, sizes)
    shares = [ts.accumulate(d, max_edges=k, total=sum(sizes)) for d, k in zip(parts, bounds)]
    loss = ts.apply()
    ts.check()
    print(name, sizes, "shares", [float(s) for s in shares], "sum", float(loss), "one call", float(one["loss"]))
    assert abs(sum(float(s) for s in shares) - float(loss)) <= 1e-6 * abs(float(loss))
    _meets_fixture_bars(name, float(loss), ts.grad, one)


# ------------------------------------------------------------------------------------------------ 3. row independence
@pytest.mark.parametrize("latency", [0, 1, -1])
def test_predictions_of_a_part_are_the_rows_of_the_one_call(dev, latency):
    f = _fixture("train_rope.npz")["f"]
    data = _data(f, dev)
    whole, _ = _train_step(dev, f, lr=0.0)
    whole.engine.set_option("latency", latency)
    whole.step(data, max_edges=_max_edges(data))
    for sizes in ([3, 1], [1, 1, 1, 1]):
        ts, _ = _train_step(dev, f, lr=0.0)
        ts.engine.set_option("latency", latency)
        parts, bounds = _parts(f, dev, sizes)
        ts.step_parts(parts, max_edges=bounds)
        assert len(ts.last_pred) == len(sizes)
        for idx, p in zip(splits(sizes), ts.last_pred):
            want = whole.last_pred[:, idx]
            d = float((p - want).abs().max())
            print(f"latency {latency}, part {idx}: max |pred - one call's rows| {d:.3e}")
            if latency >= 0:
                assert torch.equal(p, want), (latency, idx)
            else:                                                  # by launch size: a B = 1 part may take the other kernel family
                assert d <= POS_TOL, (idx, d)
        ts.check()
    whole.check()


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_two_runs_of_the_same_parts_give_the_same_bits(dev):
    f = _fixture("train_rope.npz")["f"]
    runs = []
    for _ in range(2):
        ts, _ = _train_step(dev, f)
        parts, bounds = _parts(f, dev, [2, 2])
        losses = [ts.step_parts(parts, max_edges=bounds) for _ in range(2)]
        ts.check()
        runs.append((losses, [g.clone() for g in ts.grad], ts.w))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    for k in range(22):
        assert torch.equal(runs[0][1][k], runs[1][1][k]) and torch.equal(runs[0][2][k], runs[1][2][k]), TR.KEYS[k]


# ------------------------------------------------------------------------------------------------ 5. skipped step
def test_overflow_in_a_later_part_skips_the_whole_step(dev):
    f = _fixture("train_cloth.npz")["f"]
    ts, _ = _train_step(dev, f)
    parts, bounds = _parts(f, dev, [2, 1])
    ts.step_parts(parts, max_edges=bounds)                         # one applied step, so m and v are not zero
    ts.check()
    before = [x.clone() for x in ts.w + ts.exp_avg + ts.exp_avg_sq]
    ts.accumulate(parts[0], max_edges=bounds[0], total=3)
    ts.accumulate(parts[1], max_edges=bounds[1] - 5, total=3)      # the guard presents part 2's graph as empty
    ts.apply()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, ts.w + ts.exp_avg + ts.exp_avg_sq))
    assert ts._step == 2
    with pytest.raises(Exception, match="Exceeds max dims"):
        ts.check()
    ts.check()
    assert ts._step == 1 and int(ts._status[1]) == 1               # the counter is back at the applied steps
    ts.step_parts(parts, max_edges=bounds)                         # the next clean step is applied
    ts.check()
    assert ts._step == 2 and int(ts._status[1]) == 2
    assert not torch.equal(ts.w[0], before[0])
    fresh, _ = _train_step(dev, f)
    for _ in range(2):
        fresh.step_parts(parts, max_edges=bounds)
    for a, b in zip(ts.w + ts.exp_avg + ts.exp_avg_sq, fresh.w + fresh.exp_avg + fresh.exp_avg_sq):
        assert torch.equal(a, b)


def test_argument_errors_leave_the_object_usable(dev):
    f = _fixture("train_rope.npz")["f"]
    ts, _ = _train_step(dev, f)
    parts, bounds = _parts(f, dev, [2, 2])
    ts.accumulate(parts[0], max_edges=bounds[0], total=4)
    with pytest.raises(ValueError):
        ts.accumulate(parts[1], max_edges=bounds[1], total=5)
    with pytest.raises(RuntimeError, match="inside an open step"):
        ts.step(parts[1], max_edges=bounds[1])
    with pytest.raises(ValueError, match="hold 2 rows"):
        ts.apply()
    ts.accumulate(parts[1], max_edges=bounds[1], total=4)
    loss = ts.apply()
    ts.check()
    ref, _ = _train_step(dev, f)
    assert torch.equal(loss, ref.step_parts(parts, max_edges=bounds)) and ts._step == 1


# ------------------------------------------------------------------------------------------------ 6. it does not wait
def test_parts_return_while_the_stream_is_busy(dev):
    f = _fixture("train_rope.npz")["f"]
    ts, _ = _train_step(dev, f)
    parts, bounds = _parts(f, dev, [2, 2])

    def step():
        ts.accumulate(parts[0], max_edges=bounds[0], total=4)
        ts.accumulate(parts[1], max_edges=bounds[1], total=4)
        return ts.apply()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    T = time.perf_counter() - t0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    ms_per_cycle = e0.elapsed_time(e1) / 10_000_000
    want_ms = max(100.0, 4e3 * T)
    done = torch.cuda.Event()
    torch.cuda._sleep(int(want_ms / ms_per_cycle))
    done.record()
    step()
    still_busy = not done.query()
    torch.cuda.synchronize()
    print(f"host time of accumulate, accumulate, apply {T * 1e3:.2f} ms, spin {want_ms:.0f} ms")
    assert still_busy, "accumulate / apply waited for the GPU"
    ts.check()


# ------------------------------------------------------------------------------------------------ 7. Adam curve
def test_two_part_loss_curve_matches_the_fixture(dev):
    f = _fixture("train_rope.npz")["f"]
    ts, _ = _train_step(dev, f, lr=0.001)
    parts, bounds = _parts(f, dev, [2, 2])
    curve = [float(ts.step_parts(parts, max_edges=bounds)) for _ in range(5)]
    ts.check()
    print("2 + 2", curve, "fixture", f["adam_losses"].tolist())
    np.testing.assert_allclose(curve, f["adam_losses"], rtol=1e-3)


# ------------------------------------------------------------------------------------------------ 8. mixed bounds
@pytest.mark.parametrize("name,sizes", [("train_rope.npz", [2, 2]), ("train_cloth.npz", [2, 1])])
def test_per_part_bounds_give_the_bits_of_the_common_bound(dev, name, sizes):
    f = _fixture(name)["f"]
    parts, bounds = _parts(f, dev, sizes)
    print(name, "bounds", bounds)
    tight, _ = _train_step(dev, f)
    common, _ = _train_step(dev, f)
    l1 = tight.step_parts(parts, max_edges=bounds)
    l2 = common.step_parts(parts, max_edges=max(bounds) + 37)       # edge_rows only sizes the workspace and the padded rows
    tight.check()
    common.check()
    assert torch.equal(l1, l2)
    for k in range(22):
        assert torch.equal(tight.grad[k], common.grad[k]) and torch.equal(tight.w[k], common.w[k]), TR.KEYS[k]


# ------------------------------------------------------------------------------------------------ 9. clamped motion
def test_clamp_fixture_through_the_part_entry(dev):
    f = _fixture("train_clamp.npz")["f"]
    ts, _ = _train_step(dev, f, lr=0.0)
    data = _data(f, dev)
    B = data["state"].shape[0]
    ts.accumulate(data, max_edges=_max_edges(data), total=B)
    loss = ts.apply()
    ts.check()
    _meets_fixture_bars("train_clamp.npz", float(loss), ts.grad)
    if B > 1:                                                      # and split, so the accumulating epilogue sees the clamped branch
        sizes = [B - 1, 1]
        parts, bounds = _parts(f, dev, sizes)
        loss = ts.step_parts(parts, max_edges=bounds)
        ts.check()
        _meets_fixture_bars("train_clamp.npz", float(loss), ts.grad)
