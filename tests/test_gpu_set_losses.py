"""GPU checks of the training set losses (-m gpu): ag_set_loss / ag_set_loss_backward through ChamferLoss and HausdorffLoss against
the reference's values and autograd gradients (tests/golden/set_losses.npz), and TrainStep(losses=...) - ag_train_step_losses -
against the reference's training chain (train_losses_rope.npz), the autograd path, the default path's bits, and itself in parts.
Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

import train_restate as TR
from test_train import grad_tol
from test_set_losses import standalone_cases, fixture_losses, SHAPES
from test_gpu_train import _model, _fixture_edges, _graph
from test_gpu_train_step import _data, _train_step, _max_edges, _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def train_fx():
    return TR.load_fixture("train_losses_rope.npz")


def _modules():
    import adaptigraph_amd as ag
    return {"mse": torch.nn.MSELoss(), "chamfer": ag.ChamferLoss(), "hausdorff": ag.HausdorffLoss()}


# ------------------------------------------------------------------------------------------------ 1. standalone
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_set_loss_modules_match_reference(dev, k):
    c = standalone_cases()[k]
    mods = _modules()
    y = _t(c["y"], dev)
    for name in ("chamfer", "hausdorff"):
        x = _t(c["x"], dev).requires_grad_(True)
        v = mods[name](x, y)
        assert v.dim() == 0 and v.is_cuda
        (3.0 * v).backward()                                               # a grad_out other than one
        ref, g_ref = float(c[name]), 3.0 * c["g_" + name]
        g = x.grad.cpu().numpy()
        err = np.abs(g - g_ref).max()
        print(f"c{k} {SHAPES[k]} {name}: {float(v.detach()):.8g} reference {ref:.8g}; gradient error {err:.3e}, max|g_ref| {np.abs(g_ref).max():.3e}")
        assert abs(float(v.detach()) - ref) <= 1e-5 * abs(ref)
        assert np.isfinite(g).all()
        assert err <= 1e-4 * np.abs(g_ref).max() + 1e-7
        # the backward that searches again (no tables handed over) writes the same bits
        import adaptigraph_amd as ag
        from adaptigraph_amd.context import ptr, current_stream
        eng = ag.default_engine(dev)
        B, N, M = SHAPES[k]
        g2 = torch.full_like(x, float("nan"))
        go = torch.full((1,), 3.0, device=dev)
        eng.check(eng.lib.ag_set_loss_backward(eng.ctx, current_stream(dev), ptr(x.detach()), ptr(y), B, N, M, B,
                                               {"chamfer": 1, "hausdorff": 2}[name], ptr(go), ptr(g2), None))
        assert torch.equal(g2, x.grad)
    if k == 4:
        # the coincident pair x[0,2] == y[0,4]: alone in a batch its distance is zero and so is every gradient - no NaN
        x = _t(c["x"][:1, 2:3], dev).requires_grad_(True)
        v = mods["chamfer"](x, _t(c["y"][:1, 4:5], dev)) + mods["hausdorff"](x, _t(c["y"][:1, 4:5], dev))
        v.backward()
        assert float(v.detach()) == 0.0 and torch.count_nonzero(x.grad) == 0


def test_set_loss_argument_errors(dev):
    mods = _modules()
    x = torch.zeros(2, 4, 3, device=dev)
    with pytest.raises(NotImplementedError, match="label"):
        mods["chamfer"](x, torch.zeros(2, 5, 3, device=dev, requires_grad=True))
    with pytest.raises(NotImplementedError, match="LDS tile"):           # refused before anything is enqueued
        mods["hausdorff"](torch.zeros(1, 7000, 3, device=dev), torch.zeros(1, 7000, 3, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mods["chamfer"](x.cpu(), x.cpu())


# ------------------------------------------------------------------------------------------------ 2. the training chain
def test_fused_losses_match_reference(dev, train_fx):
    f = train_fx
    ts, _ = _train_step(dev, f, lr=0.0, losses=fixture_losses(f))
    data = _data(f, dev)
    loss = float(ts.step(data, max_edges=_max_edges(data)))
    ts.check()
    terms = ts.last_loss_terms.cpu().double().numpy()
    print("loss_sum", loss, "reference", float(f["loss_sum"]))
    print("terms", terms.tolist(), "reference", f["loss_terms"].tolist())
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"]))
    assert terms.shape == f["loss_terms"].shape
    assert (np.abs(terms - f["loss_terms"]) <= 1e-5 * np.abs(f["loss_terms"])).all()
    bad = []
    for k, t in zip(TR.KEYS, ts.grad):
        ref = f["g::" + k]
        err = np.abs(t.cpu().numpy() - ref).max()
        print(f"  {k}: vs reference {err:.3e} (bar {grad_tol(f, k):.3e}), max|g_ref| {np.abs(ref).max():.3e}")
        if not err <= grad_tol(f, k):
            bad.append((k, float(err), float(grad_tol(f, k))))
    assert not bad, bad


def test_fused_losses_adam_curve(dev, train_fx):
    f = train_fx
    ts, _ = _train_step(dev, f, lr=0.001, losses=fixture_losses(f))
    data = _data(f, dev)
    k = _max_edges(data)
    curve = [float(ts.step(data, max_edges=k)) for _ in range(5)]
    ts.check()
    print("fused", curve, "fixture", f["adam_losses"].tolist())
    np.testing.assert_allclose(curve, f["adam_losses"], rtol=1e-3)


def _autograd_chain(model, f, dev, loss_funcs):
    """train.py:86-121 on the engine model under torch autograd, loss = sum(weight * func(pred, gt)) over loss_funcs."""
    edges = _fixture_edges(f, dev)
    state, action = _t(f["state"], dev), _t(f["action"], dev)
    fut, eef, act_f = _t(f["state_future"], dev), _t(f["eef_future"], dev), _t(f["action_future"], dev)
    n_p, n_future = f["p_instance"].shape[1], int(f["n_future"])
    loss_sum = 0
    for fi in range(n_future):
        gt = fut[:, fi].clone()
        pred, _ = model(**_graph(f, dev, state=state, action=action, edges=edges))
        pred_p = pred[:, :gt.shape[1], :3].clone()
        loss_sum = loss_sum + sum([w * func(pred_p, gt) for func, w in loss_funcs])
        if fi < n_future - 1:
            nxt = eef[:, fi].clone().unsqueeze(1)
            nxt[:, -1, :n_p] = pred_p
            state = torch.cat([state[:, 1:], nxt], 1)
            action = act_f[:, fi]
    return loss_sum


def test_autograd_path_with_the_modules_equals_fused(dev, train_fx):
    f = train_fx
    losses = fixture_losses(f)
    ts, _ = _train_step(dev, f, lr=0.0, losses=losses)
    data = _data(f, dev)
    fused = float(ts.step(data, max_edges=_max_edges(data)))
    ts.check()
    mods = _modules()
    model = _model(dev, TR.fixture_weights(f), pstep=int(f["pstep"])).train()
    loss = _autograd_chain(model, f, dev, [(mods[n], w) for n, w in losses])
    loss.backward()
    print("fused", fused, "autograd", loss.item())
    assert abs(fused - loss.item()) <= 1e-5 * abs(fused)
    bad = []
    for k, p, g in zip(TR.KEYS, model.ordered_parameters(), ts.grad):
        ref = p.grad.detach()
        err, top = float((g - ref).abs().max()), float(ref.abs().max())
        print(f"  {k}: fused vs autograd {err:.3e}, max|g| {top:.3e}")
        if not err <= 1e-4 * top + 1e-7:
            bad.append((k, err, top))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. the default stays
def test_default_and_explicit_mse_are_the_same_bits(dev):
    f = TR.load_fixture("train_rope.npz")
    data = _data(f, dev)
    k = _max_edges(data)
    runs = []
    for kw in ({}, {"losses": [("mse", 1)]}):
        ts, _ = _train_step(dev, f, **kw)
        losses = [ts.step(data, max_edges=k) for _ in range(3)]
        ts.check()
        runs.append((ts, losses))
    (a, la), (b, lb) = runs
    assert a.last_loss_terms is None and b.last_loss_terms.shape == (3, 1)
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    assert torch.equal(a._loss, b._loss) and torch.equal(b.last_loss_terms[:, 0], b._loss[:3])
    for x, y in zip(a.w + a.exp_avg + a.exp_avg_sq + a.grad, b.w + b.exp_avg + b.exp_avg_sq + b.grad):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 4. parts
def test_mse_chamfer_in_two_parts_equals_one_step(dev, train_fx):
    f = train_fx
    losses = [("mse", 1.0), ("chamfer", 0.5)]
    whole, _ = _train_step(dev, f, lr=0.0, losses=losses)
    data = _data(f, dev)
    l1 = float(whole.step(data, max_edges=_max_edges(data)))
    whole.check()
    parts, _ = _train_step(dev, f, lr=0.0, losses=losses)
    B = f["attrs"].shape[0]
    for idx in ([0, 1], [2]):
        d = _data(f, dev, idx=idx)
        parts.accumulate(d, max_edges=_max_edges(d), total=B)
    l2 = float(parts.apply())
    parts.check()
    print("one step", l1, "two parts", l2, "terms", whole.last_loss_terms.tolist(), parts.last_loss_terms.tolist())
    assert abs(l1 - l2) <= 1e-6 * abs(l1)
    assert torch.allclose(whole.last_loss_terms, parts.last_loss_terms, rtol=1e-6, atol=0)
    bad = []
    for k, a, b in zip(TR.KEYS, whole.grad, parts.grad):
        err = float((a - b).abs().max())
        print(f"  {k}: parts vs whole {err:.3e} (bar {grad_tol(f, k):.3e})")
        if not err <= grad_tol(f, k):
            bad.append((k, err))
    assert not bad, bad


def test_hausdorff_refusals_enqueue_nothing(dev, train_fx):
    import adaptigraph_amd as ag
    f = train_fx
    ts, model = _train_step(dev, f, losses=fixture_losses(f))
    data = _data(f, dev)
    before = [t.clone() for t in [ts._loss, ts._status, ts.last_loss_terms] + ts.grad]
    with pytest.raises(ValueError, match="Hausdorff"):
        ts.accumulate(data, max_edges=_max_edges(data))
    with pytest.raises(ValueError, match="Hausdorff"):
        ts.step_parts([data], max_edges=_max_edges(data))
    with pytest.raises(ValueError, match="Hausdorff"):
        ag.TrainStep(model, losses=[("hausdorff", 1)], group=True)
    assert not ts._parts.open and ts._step == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, [ts._loss, ts._status, ts.last_loss_terms] + ts.grad))
    # the boundary refuses the same thing on its own
    from adaptigraph_amd import _lib
    from adaptigraph_amd.context import ptr, current_stream
    eng = ag.default_engine(dev)
    x = torch.zeros(2, 4, 3, device=dev)
    out = torch.zeros((), device=dev)
    assert eng.lib.ag_set_loss(eng.ctx, current_stream(dev), ptr(x), ptr(x), 2, 4, 4, 3, _lib.AG_LOSS_HAUSDORFF, ptr(out),
                               None) == _lib.AG_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 5. evaluate, determinism
def test_evaluate_gives_the_bits_of_step(dev, train_fx):
    f = train_fx
    ts, _ = _train_step(dev, f, lr=0.0, losses=fixture_losses(f))
    data = _data(f, dev)
    k = _max_edges(data)
    l_step = ts.step(data, max_edges=k)
    terms = ts.last_loss_terms.clone()
    l_eval = ts.evaluate(data, max_edges=k)
    ts.check()
    assert torch.equal(l_step, l_eval) and torch.equal(terms, ts.last_loss_terms)


def test_losses_determinism(dev, train_fx):
    f = train_fx
    data = _data(f, dev)
    k = _max_edges(data)
    runs = []
    for _ in range(2):
        ts, _ = _train_step(dev, f, losses=fixture_losses(f))
        out = [ts.step(data, max_edges=k) for _ in range(3)]
        ts.check()
        runs.append((ts, out))
    (a, la), (b, lb) = runs
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    for x, y in zip(a.w + a.exp_avg + a.exp_avg_sq + a.grad + [a.last_loss_terms], b.w + b.exp_avg + b.exp_avg_sq + b.grad + [b.last_loss_terms]):
        assert torch.equal(x, y)
    assert not torch.equal(a.w[0], _t(TR.fixture_weights(f)[TR.KEYS[0]], dev))   # the steps moved the weights
