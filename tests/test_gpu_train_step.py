"""GPU checks of the device-resident training step (-m gpu): ag_ctx_load_weights_device, ag_adam_step, ag_train_step and
adaptigraph_amd.TrainStep against the autograd path, the reference's gradients (tests/golden/train_*.npz), the float64 torch
restatement (tests/train_restate.py) and torch.optim.Adam.  Every test prints the figures it asserts on."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import train_restate as TR
from test_train import FIXTURES, grad_tol
from test_gpu_train import _model, _fixture_edges, _graph, _chain, _f64_grads, _edge_list, _synthetic_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _data(f, dev, idx=None):
    """The dict train.py hands to model(**data), from a training fixture (idx: graphs to take, repeats allowed)."""
    idx = np.arange(f["attrs"].shape[0]) if idx is None else np.asarray(idx)
    N = f["attrs"].shape[1]
    off = np.concatenate([[0], np.cumsum(f["n_edges"])])
    edges = _edge_list([f["recv"][off[b]:off[b + 1]] for b in idx], [f["send"][off[b]:off[b + 1]] for b in idx], N, dev)
    d = {k: _t(f[k][idx], dev) for k in ("state", "attrs", "p_instance", "action", "state_future", "eef_future", "action_future")}
    d["phys_physics_param"] = _t(f["physics_param"][idx], dev)
    d["edges"] = edges
    return d


def _train_step(dev, f, **kw):
    import adaptigraph_amd as ag
    model = _model(dev, TR.fixture_weights(f), n_his=f["state"].shape[1], pstep=int(f["pstep"]))
    kw.setdefault("n_future", int(f["n_future"]))
    return ag.TrainStep(model, **kw), model


def _max_edges(data):
    return int(data["edges"].n_edges.max().item())


# ------------------------------------------------------------------------------------------------ 1. device pack = host pack
def _raw_forward(eng, d, dev):
    from adaptigraph_amd.context import ptr, current_stream
    B, N = d["attrs"].shape[:2]
    n_p, n_inst = d["p_instance"].shape[1:]
    phys = torch.zeros(B, N, device=dev)
    phys[:, :n_p] = d["phys_physics_param"]
    group = torch.cat([d["p_instance"], torch.zeros(B, N - n_p, n_inst, device=dev)], 1).contiguous()
    pos = torch.empty(B, n_p, 3, device=dev)
    mot = torch.empty(B, n_p, 3, device=dev)
    e = d["edges"]
    eng.check(eng.lib.ag_forward(eng.ctx, current_stream(dev), ptr(d["state"]), ptr(d["attrs"]), ptr(d["action"]), ptr(phys),
                                 ptr(group), n_inst, ptr(e.recv), ptr(e.send), ptr(e.row_ptr), ptr(e.n_edges), e.edge_cap, B, N,
                                 n_p, ptr(pos), ptr(mot)))
    return pos, mot


@pytest.mark.parametrize("case", ["chip_filling", "one_graph", "bf16x3"])
def test_device_packed_weights_equal_host_packed(dev, case):
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import current_stream
    f = TR.load_fixture("train_rope.npz")
    W = TR.fixture_weights(f)
    host, device = ag.Engine(dev), ag.Engine(dev)
    if case == "bf16x3":
        host.set_precision("bf16x3")
        device.set_precision("bf16x3")
    host.load_state_dict_tensors({k: torch.from_numpy(v) for k, v in W.items()})
    wd = [_t(W[k], dev) for k in TR.KEYS]
    arr = (C.c_void_p * 22)(*[w.data_ptr() for w in wd])
    device.check(device.lib.ag_ctx_load_weights_device(device.ctx, current_stream(dev), arr))
    d = _data(f, dev, idx=[0] if case == "one_graph" else np.arange(128) % 4)
    if case != "one_graph":
        d["state"] = d["state"] + 0.01 * torch.randn(d["state"].shape, generator=torch.Generator().manual_seed(1)).to(dev)
    p0, m0 = _raw_forward(host, d, dev)
    p1, m1 = _raw_forward(device, d, dev)
    assert torch.isfinite(p0).all() and float(m0.abs().max()) > 0
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    host.close()
    device.close()


def test_device_packed_weights_equal_host_packed_n_his_5(dev):
    """The rel_dim = 20 first layer (n_his 5, softbody-shaped): host-loaded against device-loaded engine through ag_forward."""
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import current_stream
    n_obj, n_his, pstep = 200, 5, 4
    f, recv_l, send_l, N = _synthetic_case(dev, n_obj, 10, 0.5, n_his, pstep, seed=21)
    W = TR.make_weights(5, n_his=n_his)
    kw = dict(pstep=pstep, n_his=n_his, rel_dim=5 + 3 * n_his)
    host, device = ag.Engine(dev, **kw), ag.Engine(dev, **kw)
    host.load_state_dict_tensors({k: torch.from_numpy(v) for k, v in W.items()})
    wd = [_t(W[k], dev) for k in TR.KEYS]
    arr = (C.c_void_p * 22)(*[w.data_ptr() for w in wd])
    device.check(device.lib.ag_ctx_load_weights_device(device.ctx, current_stream(dev), arr))
    d = {k: _t(f[k], dev) for k in ("state", "attrs", "p_instance", "action")}
    d["phys_physics_param"] = _t(f["physics_param"], dev)
    d["edges"] = _edge_list(recv_l, send_l, N, dev)
    p0, m0 = _raw_forward(host, d, dev)
    p1, m1 = _raw_forward(device, d, dev)
    assert torch.isfinite(p0).all() and float(m0.abs().max()) > 0
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    host.close()
    device.close()


# ------------------------------------------------------------------------------------------------ 2. predictions
@pytest.mark.parametrize("name", FIXTURES)
def test_evaluate_predictions_are_the_bits_of_the_model(dev, name):
    f = TR.load_fixture(name)
    ts, model = _train_step(dev, f)
    data = _data(f, dev)
    vloss = ts.evaluate(data)
    preds = []

    def step(s, a):
        out = model(**_graph(f, dev, state=s, action=a, edges=data["edges"]))
        preds.append(out[0])
        return out
    with torch.no_grad():
        inp = dict(state=data["state"], action=data["action"], n_p=f["p_instance"].shape[1], state_future=data["state_future"],
                   eef_future=data["eef_future"], action_future=data["action_future"])
        loss = TR.chain_loss(step, inp, int(f["n_future"]))
    assert ts.last_pred.shape[0] == len(preds) == int(f["n_future"])
    for fi, p in enumerate(preds):
        assert torch.equal(ts.last_pred[fi], p), fi
    print(name, "valid loss", float(vloss), "torch chain", float(loss))
    assert abs(float(vloss) - float(loss)) <= 1e-5 * abs(float(loss)) + 1e-7
    ts.check()


# ------------------------------------------------------------------------------------------------ 3. loss and gradients
@pytest.mark.parametrize("name", FIXTURES)
def test_fused_gradients_match_reference(dev, name):
    f = TR.load_fixture(name)
    ts, _ = _train_step(dev, f, lr=0.0)
    data = _data(f, dev)
    w0 = [w.clone() for w in ts.w]
    loss = float(ts.step(data, max_edges=_max_edges(data)))
    ts.check()
    print(name, "loss", loss, "reference", float(f["loss_sum"]))
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"])) + 1e-7
    assert all(torch.equal(a, b) for a, b in zip(w0, ts.w))          # lr = 0 leaves the weights alone
    g = {k: t.cpu().numpy() for k, t in zip(TR.KEYS, ts.grad)}
    g64, _ = _f64_grads(f)
    bad = []
    for k in TR.KEYS:
        ref = f["g::" + k]
        err = np.abs(g[k] - ref).max()
        e64 = np.abs(g[k] - g64[k]).max()
        print(f"  {k}: vs reference {err:.3e} (bar {grad_tol(f, k):.3e}), vs float64 {e64:.3e}, reference's own "
              f"{float(f.get('err64::' + k, np.nan)):.3e}")
        if not err <= grad_tol(f, k):
            bad.append((k, "vs reference", float(err), float(np.abs(ref).max())))
        if "err64::" + k in f and not e64 <= 4 * float(f["err64::" + k]) + 1e-7 * np.abs(g64[k]).max():
            bad.append((k, "vs float64", float(e64), float(f["err64::" + k])))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 4. Adam kernel
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adam_kernel_against_float64_adam(dev, weight_decay):
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import ptr, current_stream
    rng = np.random.default_rng(4)
    W = TR.make_weights(2)
    eng = ag.Engine(dev)
    w = [_t(W[k], dev) for k in TR.KEYS]
    m = [torch.zeros_like(x) for x in w]
    v = [torch.zeros_like(x) for x in w]
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    p64 = [torch.from_numpy(W[k]).double().requires_grad_(True) for k in TR.KEYS]
    p32 = [torch.from_numpy(W[k].copy()).requires_grad_(True) for k in TR.KEYS]
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    o64, o32 = torch.optim.Adam(p64, **hyper), torch.optim.Adam(p32, **hyper)
    arr = lambda ts: (C.c_void_p * 22)(*[t.data_ptr() for t in ts])   # noqa: E731
    for step in range(1, 11):
        grads = [rng.normal(0, 10.0 ** rng.uniform(-4, 0), W[k].shape).astype(np.float32) for k in TR.KEYS]
        for a, b, g in zip(p64, p32, grads):
            a.grad, b.grad = torch.from_numpy(g).double(), torch.from_numpy(g.copy())
        o64.step()
        o32.step()
        g = [_t(x, dev) for x in grads]
        eng.check(eng.lib.ag_adam_step(eng.ctx, current_stream(dev), arr(w), arr(g), arr(m), arr(v), step, 1e-3, 0.9, 0.999, 1e-8,
                                       weight_decay, ptr(status)))
    assert status.cpu().tolist()[:2] == [0, 10]
    bad = []
    for k, a, b, ours in zip(TR.KEYS, p64, p32, w):
        ref = a.detach().numpy()
        err32 = np.abs(b.detach().double().numpy() - ref).max()
        err = np.abs(ours.cpu().double().numpy() - ref).max()
        print(f"  wd {weight_decay} {k}: kernel {err:.3e}, torch fp32 {err32:.3e}, max|w64| {np.abs(ref).max():.3e}")
        if not err <= 4 * err32 + 1e-7 * np.abs(ref).max():
            bad.append((k, float(err), float(err32)))
    assert not bad, bad
    # a raised flag: nothing moves, the step is not counted
    status[0] = 7
    before = [x.clone() for x in w + m + v]
    eng.check(eng.lib.ag_adam_step(eng.ctx, current_stream(dev), arr(w), arr(g), arr(m), arr(v), 11, 1e-3, 0.9, 0.999, 1e-8,
                                   weight_decay, ptr(status)))
    assert all(torch.equal(a, b) for a, b in zip(before, w + m + v)) and status.cpu().tolist()[:2] == [7, 10]
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. Adam curve
def test_fused_adam_loss_curve(dev):
    for name in ("train_rope.npz", "train_cloth.npz"):
        f = TR.load_fixture(name)
        ts, _ = _train_step(dev, f, lr=0.001)
        data = _data(f, dev)
        k = _max_edges(data)
        curve = [float(ts.step(data, max_edges=k)) for _ in range(5)]
        ts.check()
        model = _model(dev, TR.fixture_weights(f))
        opt = torch.optim.Adam(model.parameters(), lr=0.001)
        auto = []
        for _ in range(5):
            model.train()
            opt.zero_grad()
            loss = _chain(model, f, dev, torch.from_numpy(f["state"]).to(dev))
            loss.backward()
            opt.step()
            auto.append(loss.item())
        print(name, "fused", curve, "autograd", auto, "fixture", f["adam_losses"].tolist())
        np.testing.assert_allclose(curve, f["adam_losses"], rtol=1e-3, err_msg=name)
        np.testing.assert_allclose(curve, auto, rtol=1e-4, err_msg=name)


# ------------------------------------------------------------------------------------------------ 6. store_rest_state
def _rest_chain_loss(step, inp, n_future):
    """train.py:86-124 with store_rest_state (:111-114): frame 0 stays, frame 1 leaves."""
    state, action = inp["state"], inp["action"]
    n_p = inp["n_p"]
    loss = 0
    for fi in range(n_future):
        gt = inp["state_future"][:, fi]
        pred, _ = step(state, action)
        loss = loss + torch.nn.functional.mse_loss(pred[:, :gt.shape[1], :3], gt)
        if fi < n_future - 1:
            nxt = inp["eef_future"][:, fi].clone().unsqueeze(1)
            nxt[:, -1, :n_p] = pred[:, :n_p]
            tail = torch.cat([state[:, 2:], nxt], 1)
            state = torch.cat([state[:, 0].unsqueeze(1), tail], 1)
            action = inp["action_future"][:, fi]
    return loss


def test_store_rest_state_matches_float64_restatement(dev):
    import adaptigraph_amd as ag
    n_obj, topk, adj, n_his, pstep, n_future = 200, 10, 0.5, 5, 4, 3
    f, recv_l, send_l, N = _synthetic_case(dev, n_obj, topk, adj, n_his, pstep, seed=21)
    B = f["state"].shape[0]
    rng = np.random.default_rng(6)
    fut = (f["state"][:, -1:, :n_obj] + rng.normal(0, 0.02, (B, n_future, n_obj, 3))).astype(np.float32)
    eef = np.repeat(f["state"][:, -1:], n_future - 1, 1) + rng.normal(0, 0.01, (B, n_future - 1, N, 3)).astype(np.float32)
    act_f = np.zeros((B, n_future - 1, N, 3), np.float32)
    act_f[:, :, n_obj:] = rng.normal(0, 0.05, (B, n_future - 1, 1, 3))
    W = TR.make_weights(5, n_his=n_his)
    model = _model(dev, W, n_his=n_his, pstep=pstep)
    edges = _edge_list(recv_l, send_l, N, dev)
    ts = ag.TrainStep(model, lr=0.0, n_future=n_future, store_rest_state=True)
    data = dict(_graph(f, dev, edges=edges), state_future=_t(fut, dev), eef_future=_t(eef, dev), action_future=_t(act_f, dev))
    loss = float(ts.step(data, max_edges=_max_edges(data)))
    ts.check()
    # the float64 restatement, and the same in fp32, both on the GPU
    t64 = lambda a: torch.from_numpy(np.asarray(a)).to(dev, torch.float64)   # noqa: E731
    recv = torch.from_numpy(np.concatenate([r.astype(np.int64) + b * N for b, r in enumerate(recv_l)])).to(dev)
    send = torch.from_numpy(np.concatenate([s.astype(np.int64) + b * N for b, s in enumerate(send_l)])).to(dev)
    phys = torch.zeros(B, N, dtype=torch.float64, device=dev)
    phys[:, :n_obj] = t64(f["physics_param"])
    group = torch.zeros(B, N, 1, dtype=torch.float64, device=dev)
    group[:, :n_obj] = 1

    def grads(dt):
        Wd = {k: t64(W[k]).to(dt).requires_grad_(True) for k in TR.KEYS}
        inp = dict(state=t64(f["state"]).to(dt), action=t64(f["action"]).to(dt), n_p=n_obj, state_future=t64(fut).to(dt),
                   eef_future=t64(eef).to(dt), action_future=t64(act_f).to(dt))
        step = lambda s, a: TR.forward(Wd, s, t64(f["attrs"]).to(dt), a, phys.to(dt), group.to(dt), recv, send, n_obj, pstep)  # noqa: E731
        ls = _rest_chain_loss(step, inp, n_future)
        ls.backward()
        return float(ls.detach()), {k: Wd[k].grad.double().cpu().numpy() for k in TR.KEYS}
    l64, g64 = grads(torch.float64)
    l32, g32 = grads(torch.float32)
    print("store_rest_state loss", loss, "float64", l64, "torch fp32", l32)
    assert abs(loss - l64) <= 1e-5 * abs(l64) + 1e-7
    # the shifted chain must differ from the plain one, or the test shows nothing
    plain = ag.TrainStep(model, lr=0.0, n_future=n_future, store_rest_state=False)
    assert float(plain.step(data, max_edges=_max_edges(data))) != loss
    bad = []
    for k, ours in zip(TR.KEYS, ts.grad):
        ref = g64[k]
        err = np.abs(ours.cpu().double().numpy() - ref).max()
        err32 = np.abs(g32[k] - ref).max()
        print(f"  {k}: engine {err:.3e}, torch fp32 {err32:.3e}, max|g64| {np.abs(ref).max():.3e}")
        if not err <= max(3e-4 * np.abs(ref).max() + 1e-7, 4 * err32):
            bad.append((k, float(err), float(err32), float(np.abs(ref).max())))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 7. it does not wait
def test_step_returns_while_the_stream_is_busy(dev):
    f = TR.load_fixture("train_rope.npz")
    ts, _ = _train_step(dev, f)
    data = _data(f, dev)
    k = _max_edges(data)
    for _ in range(3):
        ts.step(data, max_edges=k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ts.step(data, max_edges=k)
    T = time.perf_counter() - t0                                   # host time of an enqueue on an idle stream
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
    ts.step(data, max_edges=k)
    still_busy = not done.query()
    torch.cuda.synchronize()
    print(f"host time of a step {T * 1e3:.2f} ms, spin {want_ms:.0f} ms")
    assert still_busy, "TrainStep.step waited for the GPU"
    ts.check()


# ------------------------------------------------------------------------------------------------ 8. skipped step
def test_overflowing_batch_is_skipped_and_reported(dev):
    f = TR.load_fixture("train_cloth.npz")
    data = _data(f, dev)
    k = _max_edges(data)
    ts, _ = _train_step(dev, f)
    before = [x.clone() for x in ts.w + ts.exp_avg + ts.exp_avg_sq]
    loss = ts.step(data, max_edges=k - 5)                          # the guard presents the offending graphs as empty
    assert loss.dim() == 0 and loss.is_cuda
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, ts.w + ts.exp_avg + ts.exp_avg_sq))
    with pytest.raises(Exception, match="Exceeds max dims"):
        ts.check()
    ts.check()                                                     # the flag is cleared
    assert ts._step == 0
    l1 = ts.step(data, max_edges=k)
    fresh, _ = _train_step(dev, f)
    l2 = fresh.step(data, max_edges=k)
    ts.check()
    fresh.check()
    assert torch.equal(l1, l2)
    for a, b in zip(ts.w + ts.exp_avg + ts.exp_avg_sq, fresh.w + fresh.exp_avg + fresh.exp_avg_sq):
        assert torch.equal(a, b)
    assert not torch.equal(ts.w[0], before[0])
    # a skipped step that nobody has checked yet must not leak into a saved optimiser state
    ts.step(data, max_edges=k - 5)
    with pytest.raises(Exception, match="Exceeds max dims"):
        ts.optimizer_state_dict()
    sd = ts.optimizer_state_dict()
    assert all(float(st["step"]) == 1.0 for st in sd["state"].values()) and ts._step == 1


# ------------------------------------------------------------------------------------------------ 9. determinism, hand-back
def test_determinism_and_hand_back(dev):
    f = TR.load_fixture("train_rope.npz")
    data = _data(f, dev)
    k = _max_edges(data)
    runs = []
    for _ in range(2):
        ts, model = _train_step(dev, f)
        for _ in range(3):
            ts.step(data, max_edges=k)
        ts.check()
        runs.append((ts, model))
    for a, b in zip(runs[0][0].w, runs[1][0].w):
        assert torch.equal(a, b)
    ts, model = runs[0]
    ts.sync_to_module()
    sd = model.state_dict()
    for key, w in zip(TR.KEYS, ts.w):
        assert torch.equal(sd[key], w), key
    ts.evaluate(data)
    preds = []

    def step(s, a):
        out = model(**_graph(f, dev, state=s, action=a, edges=data["edges"]))
        preds.append(out[0])
        return out
    with torch.no_grad():
        inp = dict(state=data["state"], action=data["action"], n_p=f["p_instance"].shape[1], state_future=data["state_future"],
                   eef_future=data["eef_future"], action_future=data["action_future"])
        TR.chain_loss(step, inp, int(f["n_future"]))
    for fi, p in enumerate(preds):
        assert torch.equal(ts.last_pred[fi], p), fi
    # Adam's state into a real torch.optim.Adam over the synced parameters: one autograd step there, one fused step here
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=0.001)
    opt.load_state_dict(ts.optimizer_state_dict())
    assert all(float(opt.state[p]["step"]) == 3.0 for p in model.parameters())
    opt.zero_grad()
    _chain(model, f, dev, torch.from_numpy(f["state"]).to(dev)).backward()
    opt.step()
    ts.step(data, max_edges=k)
    ts.check()
    # bar of the Adam-kernel test, with the reference = float64 Adam on the CPU from the same state and the autograd gradient
    bad = []
    sd3 = runs[1][0].optimizer_state_dict()                       # the state after three steps (runs[1] took no fourth)
    for i, (key, p) in enumerate(zip(TR.KEYS, model.ordered_parameters())):
        w64 = runs[1][0].w[i].double().cpu().requires_grad_(True)
        w32 = runs[1][0].w[i].cpu().clone().requires_grad_(True)
        for wx in (w64, w32):
            o = torch.optim.Adam([wx], lr=0.001)
            st = sd3["state"][i]
            o.load_state_dict({"state": {0: {"step": st["step"].clone(), "exp_avg": st["exp_avg"].cpu().to(wx.dtype),
                                             "exp_avg_sq": st["exp_avg_sq"].cpu().to(wx.dtype)}},
                               "param_groups": [dict(sd3["param_groups"][0], params=[0])]})
            wx.grad = p.grad.detach().cpu().to(wx.dtype)
            o.step()
        ref = w64.detach().numpy()
        err32 = np.abs(w32.detach().double().numpy() - ref).max()
        bar = 4 * err32 + 1e-7 * np.abs(ref).max()
        e_auto = np.abs(p.detach().double().cpu().numpy() - ref).max()
        e_fused = np.abs(ts.w[i].double().cpu().numpy() - ref).max()
        d = float((ts.w[i] - p.detach()).abs().max())
        print(f"  {key}: fused vs autograd {d:.3e}, fused vs float64 Adam {e_fused:.3e}, autograd {e_auto:.3e}, bar {bar:.3e}")
        if not d <= bar:
            bad.append((key, d, float(bar), float(e_fused), float(e_auto)))
    assert not bad, bad
