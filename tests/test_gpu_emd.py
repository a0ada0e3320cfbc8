"""GPU checks of the Earth-mover loss (-m gpu): ag_set_loss / ag_set_loss_backward with AG_LOSS_EMD through EarthMoverLoss and
earth_mover_assignment against the reference's values, autograd gradients and scipy assignments (tests/golden/emd.npz), seeded
random shapes against the numpy restatement (tests/emd_restate.py), the non-finite rule, the refusals, and TrainStep with the term
against the reference's training chain (train_emd_rope.npz), the autograd path, itself in parts, and the default path's bits.
Every test prints the figures it asserts on.

The bars on value and gradient are those tests/test_gpu_set_losses.py applies to Chamfer (value 1e-5 relative; gradient 1e-4 of
the largest reference element + 1e-7).  That file writes them inline, so there is no name to import: value_ok / grad_ok below
are the same expressions."""
import numpy as np
import pytest
import torch

import emd_restate as ER
import train_restate as TR
from test_train import grad_tol
from test_emd import emd_cases, fixture_losses, seeded_clouds, SHAPES, SEEDED
from test_gpu_set_losses import _autograd_chain
from test_gpu_train import _model
from test_gpu_train_step import _data, _train_step, _max_edges, _t

pytestmark = pytest.mark.gpu


def value_ok(v, ref):
    return abs(v - ref) <= 1e-5 * abs(ref)


def grad_ok(err, g_ref):
    return err <= 1e-4 * np.abs(g_ref).max() + 1e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def train_fx():
    return TR.load_fixture("train_emd_rope.npz")


def _losses(f):
    """The fixture's loss list for TrainStep: the Earth-mover term is taken as the package's module (its strings stay refused)."""
    import adaptigraph_amd as ag
    return [((ag.EarthMoverLoss() if n == "earth_mover" else n), w) for n, w in fixture_losses(f)]


def _raw(dev, x, y, kind=3, work=True, B_total=None):
    """ag_set_loss at the boundary: (return code, out, work)."""
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import ptr, current_stream
    eng = ag.default_engine(dev)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out = torch.full((), -7.0, device=dev)
    wk = torch.full((B * (N + M) + 4,), -7, device=dev, dtype=torch.int32)
    rc = eng.lib.ag_set_loss(eng.ctx, current_stream(dev), ptr(x), ptr(y), B, N, M, B if B_total is None else B_total, kind, ptr(out),
                             ptr(wk) if work else None)
    torch.cuda.synchronize()
    return rc, out, wk


# ------------------------------------------------------------------------------------------------ 1. standalone
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_earth_mover_matches_reference(dev, k):
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import ptr, current_stream
    c = emd_cases()[k]
    B, N, M = SHAPES[k]
    y = _t(c["y"], dev)
    x = _t(c["x"], dev).requires_grad_(True)
    ind1, ind2 = ag.earth_mover_assignment(x, y)
    assert ind1.dtype == ind2.dtype == torch.int64 and ind1.is_cuda and ind1.shape == ind2.shape == (B, min(N, M))
    assert np.array_equal(ind1.cpu().numpy(), c["ind1"]) and np.array_equal(ind2.cpu().numpy(), c["ind2"])
    v = ag.EarthMoverLoss()(x, y)
    assert v.dim() == 0 and v.is_cuda
    (3.0 * v).backward()                                                   # a grad_out other than one
    ref, g_ref = float(c["emd"]), 3.0 * c["g_emd"]
    g = x.grad.cpu().numpy()
    err = np.abs(g - g_ref).max()
    print(f"c{k} {SHAPES[k]}: {float(v.detach()):.8g} reference {ref:.8g}; gradient error {err:.3e}, max|g_ref| {np.abs(g_ref).max():.3e}")
    assert value_ok(float(v.detach()), ref)
    assert np.isfinite(g).all()
    assert grad_ok(err, g_ref)
    matched = np.zeros((B, N), bool)
    matched[np.arange(B)[:, None], c["ind1"]] = True
    assert (g[~matched] == 0).all() and (~matched).sum() == B * max(0, N - M)      # unmatched x rows: exactly zero
    if k == 8:
        assert (g[0, 2] == 0).all()                                         # the coincident pair: zero distance, zero gradient
    # the backward that solves again (no table handed over) writes the same bits
    eng = ag.default_engine(dev)
    g2 = torch.full_like(x, float("nan"))
    go = torch.full((1,), 3.0, device=dev)
    eng.check(eng.lib.ag_set_loss_backward(eng.ctx, current_stream(dev), ptr(x.detach()), ptr(y), B, N, M, B, 3, ptr(go), ptr(g2), None))
    assert torch.equal(g2, x.grad)


@pytest.mark.parametrize("case", SEEDED, ids=lambda c: "x".join(map(str, c[:3])))
def test_seeded_shapes_match_restatement(dev, case):
    import adaptigraph_amd as ag
    B, N, M, seed = case
    xn, yn = seeded_clouds(B, N, M, seed)
    r1, r2 = ER.assignment(xn, yn, np.float32)
    x, y = _t(xn, dev).requires_grad_(True), _t(yn, dev)
    ind1, ind2 = ag.earth_mover_assignment(x, y)
    assert np.array_equal(ind1.cpu().numpy(), r1) and np.array_equal(ind2.cpu().numpy(), r2)
    v = ag.EarthMoverLoss()(x, y)
    v.backward()
    ref, g_ref = ER.value_and_grad(xn, yn, r1, r2)
    err = np.abs(x.grad.cpu().numpy() - g_ref).max()
    print(f"{case}: {float(v.detach()):.8g} restatement {ref:.8g}; gradient error {err:.3e}, max|g_ref| {np.abs(g_ref).max():.3e}")
    assert value_ok(float(v.detach()), ref) and grad_ok(err, g_ref)


def test_two_runs_give_the_same_bits(dev):
    import adaptigraph_amd as ag
    xn, yn = seeded_clouds(*SEEDED[3])
    runs = []
    for _ in range(2):
        x, y = _t(xn, dev).requires_grad_(True), _t(yn, dev)
        v = ag.EarthMoverLoss()(x, y)
        v.backward()
        rc, out, wk = _raw(dev, x.detach(), y)
        assert rc == 0
        runs.append((v.detach().clone(), x.grad.clone(), out, wk[:xn.shape[0] * xn.shape[1] + xn.shape[0]].clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(runs[0][0], runs[0][2])


def test_non_finite_graph_fails_alone(dev):
    import adaptigraph_amd as ag
    B, N, M = 3, 9, 7
    xn, yn = seeded_clouds(B, N, M, 5)
    clean = ag.earth_mover_assignment(_t(xn, dev), _t(yn, dev))
    rc, _, wk_clean = _raw(dev, _t(xn, dev), _t(yn, dev))
    assert rc == 0 and (wk_clean[B * N:B * N + B] == 0).all()
    xb = xn.copy()
    xb[1, 4, 1] = np.nan
    x, y = _t(xb, dev).requires_grad_(True), _t(yn, dev)
    v = ag.EarthMoverLoss()(x, y)
    v.backward()
    g = x.grad.cpu().numpy()
    rc, out, wk = _raw(dev, x.detach(), y)
    table, status = wk[:B * N].view(B, N).cpu().numpy(), wk[B * N:B * N + B].cpu().numpy()
    print("loss", float(v.detach()), "status", status.tolist(), "table of graph 1", table[1].tolist())
    assert rc == 0 and np.isnan(float(v.detach())) and np.isnan(float(out))
    assert np.isnan(g[1]).all() and np.isfinite(g[[0, 2]]).all()
    assert (table[1] == -1).all() and status.tolist() == [0, 1, 0]
    assert np.array_equal(table[[0, 2]], wk_clean[:B * N].view(B, N).cpu().numpy()[[0, 2]])
    ind1, ind2 = ag.earth_mover_assignment(x, y)
    assert (ind1[1] == -1).all() and (ind2[1] == -1).all()
    for b in (0, 2):
        assert torch.equal(ind1[b], clean[0][b]) and torch.equal(ind2[b], clean[1][b])
    # an infinite coordinate on the label side fails its graph as well
    yb = yn.copy()
    yb[2, 0, 0] = np.inf
    rc, out, wk = _raw(dev, _t(xn, dev), _t(yb, dev))
    assert rc == 0 and np.isnan(float(out)) and wk[B * N:B * N + B].tolist() == [0, 0, 1]


def test_refusals_enqueue_nothing(dev):
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    loss = ag.EarthMoverLoss()
    cap = _lib.EMD_MAX_MATCH
    x = torch.zeros(2, 4, 3, device=dev)
    with pytest.raises(NotImplementedError, match="label"):
        loss(x, torch.zeros(2, 5, 3, device=dev, requires_grad=True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.earth_mover_assignment(x.cpu(), x.cpu())
    with pytest.raises(NotImplementedError, match="at most %d" % cap):       # K above the cap
        loss(torch.zeros(1, cap + 1, 3, device=dev), torch.zeros(1, cap + 1, 3, device=dev))
    with pytest.raises(NotImplementedError, match="LDS tile"):              # N + M above the tile, K small
        loss(torch.zeros(1, 8, 3, device=dev), torch.zeros(1, 4200, 3, device=dev))
    loss(torch.rand(1, 8, 3, device=dev), torch.rand(1, 3000, 3, device=dev))        # inside both limits: served
    # at the boundary: the code, and neither the value nor the work buffer is touched
    for N, M in ((cap + 1, cap + 1), (8, 4200)):
        rc, out, wk = _raw(dev, torch.zeros(1, N, 3, device=dev), torch.zeros(1, M, 3, device=dev))
        assert rc == _lib.AG_ERR_UNSUPPORTED and float(out) == -7.0 and (wk == -7).all()
    rc, out, wk = _raw(dev, x, x, kind=4)
    assert rc == _lib.AG_ERR_INVALID and float(out) == -7.0 and (wk == -7).all()


def test_a_part_is_its_share_of_the_whole(dev):
    xn, yn = seeded_clouds(4, 5, 9, 0)
    rc, whole, _ = _raw(dev, _t(xn, dev), _t(yn, dev))
    parts = [_raw(dev, _t(xn[s], dev), _t(yn[s], dev), B_total=4)[1] for s in (slice(0, 3), slice(3, 4))]
    print("whole", float(whole), "parts", [float(p) for p in parts])
    assert rc == 0 and abs(float(parts[0]) + float(parts[1]) - float(whole)) <= 1e-6 * float(whole)


# ------------------------------------------------------------------------------------------------ 2. the training chain
def test_fused_step_matches_reference(dev, train_fx):
    f = train_fx
    ts, _ = _train_step(dev, f, lr=0.0, losses=_losses(f))
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
    # evaluate gives the bits of step
    l_step = ts.step(data, max_edges=_max_edges(data))
    kept = ts.last_loss_terms.clone()
    l_eval = ts.evaluate(data, max_edges=_max_edges(data))
    ts.check()
    assert torch.equal(l_step, l_eval) and torch.equal(kept, ts.last_loss_terms)


def test_fused_adam_curve(dev, train_fx):
    f = train_fx
    ts, _ = _train_step(dev, f, lr=0.001, losses=_losses(f))
    data = _data(f, dev)
    k = _max_edges(data)
    curve = [float(ts.step(data, max_edges=k)) for _ in range(5)]
    ts.check()
    print("fused", curve, "fixture", f["adam_losses"].tolist())
    np.testing.assert_allclose(curve, f["adam_losses"], rtol=1e-3)


def test_autograd_path_with_the_module_equals_fused(dev, train_fx):
    import adaptigraph_amd as ag
    f = train_fx
    ts, _ = _train_step(dev, f, lr=0.0, losses=_losses(f))
    data = _data(f, dev)
    fused = float(ts.step(data, max_edges=_max_edges(data)))
    ts.check()
    mods = {"mse": torch.nn.MSELoss(), "earth_mover": ag.EarthMoverLoss()}
    model = _model(dev, TR.fixture_weights(f), pstep=int(f["pstep"])).train()
    loss = _autograd_chain(model, f, dev, [(mods[n], w) for n, w in fixture_losses(f)])
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


def test_term_beside_chamfer_equals_autograd(dev, train_fx):
    """Both kinds of set term in one list: the nearest-neighbour pass and the solve share a step, their gradient kernels add to the
    same dLoss/dpred one after the other."""
    import adaptigraph_amd as ag
    f = train_fx
    ts, _ = _train_step(dev, f, lr=0.0, losses=[("mse", 1.0), ("chamfer", 0.5), (ag.EarthMoverLoss(), 0.25)])
    data = _data(f, dev)
    fused = float(ts.step(data, max_edges=_max_edges(data)))
    ts.check()
    model = _model(dev, TR.fixture_weights(f), pstep=int(f["pstep"])).train()
    loss = _autograd_chain(model, f, dev, [(torch.nn.MSELoss(), 1.0), (ag.ChamferLoss(), 0.5), (ag.EarthMoverLoss(), 0.25)])
    loss.backward()
    print("fused", fused, "autograd", loss.item(), "terms", ts.last_loss_terms.tolist())
    assert abs(fused - loss.item()) <= 1e-5 * abs(fused)
    assert torch.allclose(ts.last_loss_terms[:, 2].double().cpu(), torch.from_numpy(f["loss_terms"][:, 1]), rtol=1e-5, atol=0)
    bad = []
    for k, p, g in zip(TR.KEYS, model.ordered_parameters(), ts.grad):
        ref = p.grad.detach()
        err, top = float((g - ref).abs().max()), float(ref.abs().max())
        print(f"  {k}: fused vs autograd {err:.3e}, max|g| {top:.3e}")
        if not err <= 1e-4 * top + 1e-7:
            bad.append((k, err, top))
    assert not bad, bad


def test_two_parts_equal_one_step(dev, train_fx):
    f = train_fx
    whole, _ = _train_step(dev, f, lr=0.0, losses=_losses(f))
    data = _data(f, dev)
    l1 = float(whole.step(data, max_edges=_max_edges(data)))
    whole.check()
    parts, _ = _train_step(dev, f, lr=0.0, losses=_losses(f))
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


def test_default_step_keeps_its_bits_beside_the_term(dev, train_fx):
    """TrainStep() with no list runs the entry points it always ran: the same bits as the explicit [("mse", 1)] list, before and
    after a step with the Earth-mover term ran on the same engine."""
    f = TR.load_fixture("train_rope.npz")
    data = _data(f, dev)
    k = _max_edges(data)

    def run(**kw):
        ts, _ = _train_step(dev, f, **kw)
        out = [ts.step(data, max_edges=k) for _ in range(2)]
        ts.check()
        return ts, out
    a, la = run()
    e, _ = _train_step(dev, train_fx, losses=_losses(train_fx))
    d = _data(train_fx, dev)
    e.step(d, max_edges=_max_edges(d))
    e.check()
    b, lb = run()
    m, lm = run(losses=[("mse", 1)])
    assert a.last_loss_terms is None and b.last_loss_terms is None
    for other, lo in ((b, lb), (m, lm)):
        assert all(torch.equal(p, q) for p, q in zip(la, lo))
        for p, q in zip(a.w + a.exp_avg + a.exp_avg_sq + a.grad, other.w + other.exp_avg + other.exp_avg_sq + other.grad):
            assert torch.equal(p, q)
