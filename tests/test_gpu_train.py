"""GPU checks of the training path (-m gpu): DynamicsPredictor under torch autograd (ag_forward + ag_backward) against the
reference's own gradients (tests/golden/train_*.npz) and the float64 torch restatement (tests/train_restate.py)."""
import numpy as np
import pytest
import torch

import train_restate as TR
from test_train import CFG, FIXTURES, grad_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(dev, W, n_his=4, pstep=3, material="rope"):
    import adaptigraph_amd as ag
    cfg = dict(CFG, pstep=pstep)
    mat = {"material_index": {material: 0}, material: {"physics_params": [{"name": "p", "use": True}]}}
    m = ag.DynamicsPredictor(cfg, mat, {"n_his": n_his, "materials": [material]}, dev)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in W.items()})
    return m.to(dev)


def _edge_list(recv_l, send_l, N, dev):
    """Per-graph (recv, send) lists sorted by receiver -> EdgeList (CSR by receiver, padded to the largest graph)."""
    from adaptigraph_amd.graph import EdgeList
    B = len(recv_l)
    cap = max(1, max(len(r) for r in recv_l))
    recv = np.zeros((B, cap), np.int32)
    send = np.zeros((B, cap), np.int32)
    row_ptr = np.zeros((B, N + 1), np.int32)
    for b, (r, s) in enumerate(zip(recv_l, send_l)):
        assert np.all(np.diff(r) >= 0)
        recv[b, :len(r)], send[b, :len(s)] = r, s
        row_ptr[b, 1:] = np.cumsum(np.bincount(r, minlength=N))
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    return EdgeList(t(recv), t(send), t(row_ptr), t(np.array([len(r) for r in recv_l], np.int32)), N)


def _fixture_edges(f, dev):
    B, N = f["attrs"].shape[:2]
    off = np.concatenate([[0], np.cumsum(f["n_edges"])])
    return _edge_list([f["recv"][off[b]:off[b + 1]] for b in range(B)], [f["send"][off[b]:off[b + 1]] for b in range(B)], N, dev)


def _graph(f, dev, state=None, action=None, edges=None):
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)   # noqa: E731
    return dict(state=t(f["state"]) if state is None else state, attrs=t(f["attrs"]), p_instance=t(f["p_instance"]),
                action=t(f["action"]) if action is None else action, edges=edges if edges is not None else _fixture_edges(f, dev),
                phys_physics_param=t(f["physics_param"]))


def _chain(model, f, dev, state0):
    """train.py:86-121 on the engine model, n_future from the fixture."""
    edges = _fixture_edges(f, dev)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)   # noqa: E731
    inp = dict(state=state0, action=t(f["action"]), n_p=f["p_instance"].shape[1], state_future=t(f["state_future"]),
               eef_future=t(f["eef_future"]), action_future=t(f["action_future"]))
    step = lambda s, a: model(**_graph(f, dev, state=s, action=a, edges=edges))   # noqa: E731
    return TR.chain_loss(step, inp, int(f["n_future"]))


def _engine_grads(f, dev):
    model = _model(dev, TR.fixture_weights(f), pstep=int(f["pstep"])).train()
    state0 = torch.from_numpy(f["state"]).to(dev).requires_grad_(True)
    loss = _chain(model, f, dev, state0)
    loss.backward()
    g = {k: p.grad.detach().cpu().numpy() for k, p in zip(TR.KEYS, model.ordered_parameters())}
    return loss.item(), g, state0.grad.cpu().numpy()


def _f64_grads(f):
    inp = TR.fixture_inputs(f, torch.float64)
    B, N = inp["attrs"].shape[:2]
    recv, send = TR.fixture_edges(f, B, N)
    W = TR.weights(f, torch.float64)
    inp["state"].requires_grad_(True)
    step = lambda s, a: TR.forward(W, s, inp["attrs"], a, inp["phys"], inp["group"], recv, send, inp["n_p"],  # noqa: E731
                                   int(f["pstep"]))
    TR.chain_loss(step, inp, int(f["n_future"])).backward()
    return {k: W[k].grad.numpy() for k in TR.KEYS}, inp["state"].grad.numpy()


def test_grad_forward_is_bit_equal_to_inference(dev):
    f = TR.load_fixture("train_rope.npz")
    model = _model(dev, TR.fixture_weights(f))
    with torch.no_grad():
        p0, m0 = model(**_graph(f, dev))
    model.train()
    st = torch.from_numpy(f["state"]).to(dev).requires_grad_(True)
    p1, m1 = model(**_graph(f, dev, state=st))
    assert p1.requires_grad and m1.requires_grad
    assert torch.equal(p0, p1.detach()) and torch.equal(m0, m1.detach())


@pytest.mark.parametrize("name", FIXTURES)
def test_chained_gradients_match_reference(dev, name):
    """n_future-step loss_sum.backward() (train.py:86-123) vs the reference's own autograd, and vs float64."""
    f = TR.load_fixture(name)
    loss, g, dstate = _engine_grads(f, dev)
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"])) + 1e-7
    g64, d64 = _f64_grads(f)
    bad = []
    for k in TR.KEYS:
        ref = f["g::" + k]
        err = np.abs(g[k] - ref).max()
        if not err <= grad_tol(f, k):
            bad.append((k, "vs reference", float(err), float(np.abs(ref).max())))
        if "err64::" + k in f:   # our error against float64 at most 4x the reference's own (floor: fp32 resolution of the tensor)
            e64 = np.abs(g[k] - g64[k]).max()
            if not e64 <= 4 * float(f["err64::" + k]) + 1e-7 * np.abs(g64[k]).max():
                bad.append((k, "vs float64", float(e64), float(f["err64::" + k])))
    assert not bad, bad
    ref = f["dstate0"]
    assert np.abs(dstate - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-7 + 2 * np.abs(ref - f["dstate0_64"]).max()
    assert np.abs(dstate - d64).max() <= 4 * np.abs(ref - d64).max() + 1e-7 * np.abs(d64).max()


def test_clamped_rows_pass_no_gradient(dev):
    """Rows with |motion| > 100 contribute exactly zero through the clamp (torch clamp_backward, inclusive bounds)."""
    f = TR.load_fixture("train_clamp.npz")
    model = _model(dev, TR.fixture_weights(f)).train()
    pos, mot = model(**_graph(f, dev))
    inside = (mot.detach().abs() <= 100).float()
    assert 0 < inside.sum() < inside.numel()
    gp = torch.randn(pos.shape, generator=torch.Generator().manual_seed(0)).to(dev)
    params = model.ordered_parameters()
    ga = torch.autograd.grad(pos, params, gp, retain_graph=True)
    gb = torch.autograd.grad(pos, params, gp * inside)
    for k, a, b in zip(TR.KEYS, ga, gb):
        assert torch.equal(a, b), k
    assert any(a.abs().max() > 0 for a in ga)


def test_adam_loss_curve(dev):
    for name in ("train_rope.npz", "train_cloth.npz"):
        f = TR.load_fixture(name)
        model = _model(dev, TR.fixture_weights(f))
        opt = torch.optim.Adam(model.parameters(), lr=0.001)
        curve = []
        for _ in range(5):
            model.train()
            opt.zero_grad()
            loss = _chain(model, f, dev, torch.from_numpy(f["state"]).to(dev))
            loss.backward()
            opt.step()
            curve.append(loss.item())
        np.testing.assert_allclose(curve, f["adam_losses"], rtol=1e-3, err_msg=name)


def test_backward_is_deterministic(dev):
    f = TR.load_fixture("train_rope.npz")
    runs = [_engine_grads(f, dev) for _ in range(2)]
    for k in TR.KEYS:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k
    assert np.array_equal(runs[0][2], runs[1][2])


def test_candidate_gradient_independent_of_batch(dev):
    f = TR.load_fixture("train_rope.npz")
    rng = np.random.default_rng(3)
    B = 8
    idx = np.arange(B) % f["state"].shape[0]
    state = (f["state"][idx] + rng.normal(0, 0.01, f["state"][idx].shape)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(f["n_edges"])])
    recv_l = [f["recv"][off[i]:off[i + 1]] for i in idx]
    send_l = [f["send"][off[i]:off[i + 1]] for i in idx]
    recv_l[5], send_l[5] = recv_l[5][:700], send_l[5][:700]      # graphs of different sizes in one batch
    N = f["attrs"].shape[1]
    model = _model(dev, TR.fixture_weights(f)).train()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    gp = t(rng.normal(0, 1, (B, f["p_instance"].shape[1], 3)))

    def dstate(sel):
        st = t(state[sel]).requires_grad_(True)
        g = dict(state=st, attrs=t(f["attrs"][idx][sel]), p_instance=t(f["p_instance"][idx][sel]), action=t(f["action"][idx][sel]),
                 edges=_edge_list([recv_l[i] for i in sel], [send_l[i] for i in sel], N, dev),
                 phys_physics_param=t(f["physics_param"][idx][sel]))
        pos, _ = model(**g)
        return torch.autograd.grad(pos, st, gp[sel])[0].cpu().numpy()

    full = dstate(list(range(B)))
    for b in (0, 5, 7):
        assert np.array_equal(dstate([b]), full[b:b + 1]), b


def _synthetic_case(dev, n_obj, topk, adj, n_his, pstep, seed, B=3):
    import adaptigraph_amd as ag
    rng = np.random.default_rng(seed)
    N = n_obj + 1
    cloud = rng.uniform(-1, 1, (n_obj, 3)).astype(np.float32) * np.float32([1.0, 0.2, 1.0])
    state = np.zeros((B, n_his, N, 3), np.float32)
    for b in range(B):
        base = np.concatenate([cloud, [[0.0, 0.1, 0.0]]], 0)
        for tt in range(n_his):
            state[b, tt] = base + rng.normal(0, 0.01, (N, 3))
    attrs = np.zeros((B, N, 2), np.float32)
    attrs[:, :n_obj, 0] = 1
    attrs[:, n_obj:, 1] = 1
    action = np.zeros((B, N, 3), np.float32)
    action[:, n_obj:] = rng.normal(0, 0.05, (B, 1, 3))
    mask = torch.ones(B, N, dtype=torch.bool, device=dev)
    tool = torch.zeros(B, N, dtype=torch.bool, device=dev)
    tool[:, n_obj:] = True
    edges = ag.construct_edges_index(torch.from_numpy(state[:, -1]).to(dev), adj, mask, tool, topk=topk)
    ne = edges.n_edges.cpu().numpy()
    recv_l = [edges.recv[b, :ne[b]].cpu().numpy() for b in range(B)]
    send_l = [edges.send[b, :ne[b]].cpu().numpy() for b in range(B)]
    return dict(state=state, attrs=attrs, action=action, p_instance=np.ones((B, n_obj, 1), np.float32),
                physics_param=rng.uniform(0.2, 0.8, (B, 1)).astype(np.float32)), recv_l, send_l, N


@pytest.mark.parametrize("kind", ["granular", "softbody"])
def test_larger_models_match_float64_restatement(dev, kind):
    """Granular size (400 + 1 particles, topk 20) and the softbody model (n_his 5, pstep 4) against float64.  Bar per tensor:
    3e-4 max|g64|, or 4x the error of the same restatement in fp32 on the GPU if that is larger.  At these sizes a few of the
    ~10^7 ReLU inputs sit within fp32 rounding of zero, and the gradient jumps there: perturbing the granular case's weights by
    6e-8 relative (fp32 rounding) moves its float64 gradients by up to 1.2e-2 of a tensor's max.  Which kinks an fp32 run lands
    on the other side of is luck: the engine's relation_propagator.linear.bias is 2e-4 off float64, torch fp32's 1.9e-5, and
    torch fp32 on the CPU 4e-7; every other tensor of the engine is within 1e-4."""
    n_obj, topk, adj, n_his, pstep = (400, 20, 0.4, 4, 3) if kind == "granular" else (200, 10, 0.5, 5, 4)
    f, recv_l, send_l, N = _synthetic_case(dev, n_obj, topk, adj, n_his, pstep, seed=21)
    B = f["state"].shape[0]
    W = TR.make_weights(5, n_his=n_his)
    model = _model(dev, W, n_his=n_his, pstep=pstep).train()
    edges = _edge_list(recv_l, send_l, N, dev)
    rng = np.random.default_rng(1)
    gp = rng.normal(0, 1, (B, n_obj, 3)).astype(np.float32)
    gm = rng.normal(0, 1, (B, n_obj, 3)).astype(np.float32)
    st = torch.from_numpy(f["state"]).to(dev).requires_grad_(True)
    pos, mot = model(**_graph(f, dev, state=st, edges=edges))
    ((pos * torch.from_numpy(gp).to(dev)).sum() + (mot * torch.from_numpy(gm).to(dev)).sum()).backward()
    # float64 restatement on the GPU
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dev, torch.float64)   # noqa: E731
    W64 = {k: t(W[k]).requires_grad_(True) for k in TR.KEYS}
    s64 = t(f["state"]).requires_grad_(True)
    phys = torch.zeros(B, N, dtype=torch.float64, device=dev)
    phys[:, :n_obj] = t(f["physics_param"])
    group = torch.zeros(B, N, 1, dtype=torch.float64, device=dev)
    group[:, :n_obj] = 1
    recv = torch.from_numpy(np.concatenate([r.astype(np.int64) + b * N for b, r in enumerate(recv_l)])).to(dev)
    send = torch.from_numpy(np.concatenate([s.astype(np.int64) + b * N for b, s in enumerate(send_l)])).to(dev)
    p64, m64 = TR.forward(W64, s64, t(f["attrs"]), t(f["action"]), phys, group, recv, send, n_obj, pstep)
    ((p64 * t(gp)).sum() + (m64 * t(gm)).sum()).backward()
    # the same restatement in fp32 under torch autograd: its error against float64 is the scale of fp32 rounding here
    W32 = {k: v.detach().float().requires_grad_(True) for k, v in W64.items()}
    s32 = s64.detach().float().requires_grad_(True)
    p32, m32 = TR.forward(W32, s32, t(f["attrs"]).float(), t(f["action"]).float(), phys.float(), group.float(), recv, send, n_obj,
                          pstep)
    ((p32 * t(gp).float()).sum() + (m32 * t(gm).float()).sum()).backward()
    assert torch.equal(pos.detach(), model(**_graph(f, dev, state=st.detach(), edges=edges))[0].detach())
    np.testing.assert_allclose(pos.detach().cpu().numpy(), p64.detach().cpu().numpy(), atol=1e-4)
    bad = []
    pairs = [(k, p.grad, W64[k].grad, W32[k].grad) for k, p in zip(TR.KEYS, model.ordered_parameters())]
    for k, ours, g64, g32 in pairs + [("state", st.grad, s64.grad, s32.grad)]:
        ref = g64.cpu().numpy()
        err = np.abs(ours.cpu().numpy() - ref).max()
        err32 = np.abs(g32.double().cpu().numpy() - ref).max()
        if not err <= max(3e-4 * np.abs(ref).max() + 1e-7, 4 * err32):
            bad.append((k, float(err), float(err32), float(np.abs(ref).max())))
    assert not bad, (kind, bad)


def test_data_gradients_are_refused(dev):
    f = TR.load_fixture("train_rope.npz")
    model = _model(dev, TR.fixture_weights(f))
    g = _graph(f, dev)
    g["phys_physics_param"] = g["phys_physics_param"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        model(**g)
    g = _graph(f, dev)
    g["action"] = g["action"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        model.train()(**g)


def test_backward_overflow_raises(dev):
    """ag_backward refuses a graph with more edges than edge_cap, as ag_forward does."""
    import ctypes as C
    from adaptigraph_amd.context import ptr, current_stream
    f = TR.load_fixture("train_rope.npz")
    model = _model(dev, TR.fixture_weights(f))
    eng = model.engine(dev)
    e = _fixture_edges(f, dev)
    n_bad = e.n_edges.clone()
    n_bad[1] = e.edge_cap + 5
    B, N = f["attrs"].shape[:2]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)   # noqa: E731
    w = [p.detach().contiguous() for p in model.ordered_parameters()]
    warr = (C.c_void_p * 22)(*[x.data_ptr() for x in w])
    dstate = torch.zeros(f["state"].shape, device=dev)
    gpos = torch.ones((B, 100, 3), device=dev)
    phys = torch.zeros(B, N, device=dev)
    group = torch.zeros(B, N, 1, device=dev)
    ins = [t(f["state"]), t(f["attrs"]), t(f["action"]), phys, group]
    with pytest.raises(Exception, match="Exceeds max dims"):
        eng.check(eng.lib.ag_backward(eng.ctx, current_stream(dev), *[ptr(x) for x in ins], 1, ptr(e.recv), ptr(e.send),
                                      ptr(e.row_ptr), ptr(n_bad), e.edge_cap, B, N, 100, warr, ptr(gpos), None, ptr(dstate),
                                      None))
    assert float(dstate.abs().max()) == 0.0


def test_step_reuploads_weights(dev):
    f = TR.load_fixture("train_rope.npz")
    model = _model(dev, TR.fixture_weights(f)).train()
    opt = torch.optim.Adam(model.parameters(), lr=0.001)
    with torch.no_grad():
        before = model(**_graph(f, dev))[0]
    loss = _chain(model, f, dev, torch.from_numpy(f["state"]).to(dev))
    loss.backward()
    opt.step()
    with torch.no_grad():
        after = model(**_graph(f, dev))[0]
    fresh = _model(dev, {k: v.detach().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        want = fresh(**_graph(f, dev))[0]
    assert not torch.equal(before, after)
    assert torch.equal(after, want)
