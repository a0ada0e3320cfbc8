"""GPU checks of the training backward (-m gpu) where its other tests never take it: degenerate graphs, more than one batch chunk
on each of the three entries that drive train_backward_chunk, and split-K slabs of more than one K tile.

The reference of every numeric comparison is the float64 torch restatement (tests/train_restate.py through
tests/backward_shapes.py) on the GPU; the bar is the project's: per tensor max|g - g64| <= max(3e-4 max|g64| + 1e-7, 4 err32),
err32 = the same restatement in fp32 under torch autograd.  Engine-against-engine comparisons are bit equalities that DESIGN.md
(3.10, 3.12, 3.13) promises: a row's input gradient and prediction do not depend on which rows share its launch, and two calls on
the same inputs give the same bits.  tests/test_backward_shapes.py keeps the batches from being vacuous.  Every test prints the
figures it asserts on."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import backward_shapes as BS
import ppm_grad_support as S
import train_restate as TR
from test_train import grad_tol
from test_set_losses import fixture_losses
from test_gpu_train import _model, _edge_list, _f64_grads
from test_gpu_train_step import _data, _train_step, _max_edges, _t
from test_gpu_ppm_fit import _problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ shared pieces
@functools.lru_cache(maxsize=None)
def _case(name, B):
    """(batch, weights, float64 gradients, fp32-restatement gradients, float64 pred_pos), computed once on the GPU and shared."""
    N, n_p, n_his, pstep = BS.CONFIGS[name]
    bt = BS.make_batch(N, n_p, n_his, B=B)
    W = TR.make_weights(5, n_his)
    g64, p64, m64 = BS.restate(bt, W, pstep, torch.float64, "cuda:0")
    g32, _, _ = BS.restate(bt, W, pstep, torch.float32, "cuda:0")
    assert np.abs(m64).max() < 100.0
    for v in list(g64.values()) + [p64]:
        v.setflags(write=False)
    return bt, W, g64, g32, p64


def _graph(bt, dev, edges, **leaves):
    d = dict(state=_t(bt["state"], dev), attrs=_t(bt["attrs"], dev), p_instance=_t(bt["p_instance"], dev),
             action=_t(bt["action"], dev), edges=edges, phys_physics_param=_t(bt["phys"], dev))
    d.update(leaves)
    return d


def _engine_grads(model, bt, dev, edges, diff):
    """diff False: DynamicsPredictor.forward (ag_backward) -> the 22 weight gradients and dstate; True: forward_diff
    (DynamicsDiffFunction, ag_backward_inputs) -> those and dphys, daction.  -> ({name: tensor}, pred_pos)."""
    for p in model.parameters():
        p.grad = None
    leaves = dict(state=_t(bt["state"], dev).requires_grad_(True))
    if diff:
        leaves.update(action=_t(bt["action"], dev).requires_grad_(True), phys_physics_param=_t(bt["phys"], dev).requires_grad_(True))
    pos, mot = (model.forward_diff if diff else model)(**_graph(bt, dev, edges, **leaves))
    ((pos * _t(bt["gp"], dev)).sum() + (mot * _t(bt["gm"], dev)).sum()).backward()
    g = {k: p.grad.detach().clone() for k, p in zip(TR.KEYS, model.ordered_parameters())}
    g["state"] = leaves["state"].grad
    if diff:
        g["phys"], g["action"] = leaves["phys_physics_param"].grad, leaves["action"].grad
    return g, pos.detach()


def _compare(label, ours, g64, g32, names):
    """the bar on every tensor of `names`; -> the offenders"""
    bad = []
    for k in names:
        ref = g64[k]
        assert np.abs(ref).max() > 0, (label, k)                                     # nothing compared is identically zero
        got = ours[k].double().cpu().numpy() if torch.is_tensor(ours[k]) else np.asarray(ours[k], np.float64)
        assert got.shape == ref.shape, (label, k, got.shape, ref.shape)
        err, err32 = np.abs(got - ref).max(), np.abs(g32[k] - ref).max()
        lim = BS.bar(ref, err32)
        print(f"  {label} {k}: err {err:.3e}  err32 {err32:.3e}  max|g64| {np.abs(ref).max():.3e}  bar {lim:.3e}")
        if not err <= lim:
            bad.append((k, float(err), float(err32), float(np.abs(ref).max())))
    return bad


def _chunked(eng, chunk, fn):
    eng.set_chunk(chunk)
    try:
        return fn()
    finally:
        eng.set_chunk(0)


# ------------------------------------------------------------------------------------------------ A. degenerate graphs
@pytest.mark.parametrize("name", list(BS.CONFIGS))
def test_degenerate_batch_matches_float64(dev, name):
    """Dense, empty, hub and half-isolated graph in one batch (tests/backward_shapes.py) with one tool row at pstep 3, with no
    tool row (n_p == N) at pstep 1 and with two tool rows, n_his 5, at pstep 7: the 22 weight gradients and dstate through
    ag_backward, and those plus dphys and daction through ag_backward_inputs, against float64.  The forward serves n_p == N, so
    no refusal is asserted for it."""
    N, n_p, n_his, pstep = BS.CONFIGS[name]
    bt, W, g64, g32, p64 = _case(name, 4)
    model = _model(dev, W, n_his=n_his, pstep=pstep).train()
    edges = _edge_list(bt["recv_l"], bt["send_l"], N, dev)
    assert edges.n_edges.cpu().tolist() == [12 * N, 0, 2 * (N - 1), 3 * (N // 2)]
    ga, pos_a = _engine_grads(model, bt, dev, edges, diff=False)
    gb, pos_b = _engine_grads(model, bt, dev, edges, diff=True)
    assert torch.equal(pos_a, pos_b)
    np.testing.assert_allclose(pos_a.cpu().numpy(), p64, atol=1e-4)
    bad = _compare(f"{name} ag_backward", ga, g64, g32, TR.KEYS + ["state"])
    bad += _compare(f"{name} ag_backward_inputs", gb, g64, g32, BS.NAMES)
    assert not bad, (name, bad)
    # the sender CSR's consequence: the hub node of graph 2 sends N-1 edges, which fill a 64-edge sweep and run into the next
    hub = {k: v["state"][2, :, N - 1] for k, v in (("ours", ga), ("g64", g64), ("g32", g32))}
    assert not _compare(f"{name} hub node", {"state": hub["ours"]}, {"state": hub["g64"]}, {"state": hub["g32"]}, ["state"])
    # ... and sender 0 of graph 3 (2 (N//2) duplicate edges over every sweep), with the isolated half next to it
    half = {k: v["state"][3] for k, v in (("ours", ga), ("g64", g64), ("g32", g32))}
    assert not _compare(f"{name} half-isolated graph", {"state": half["ours"]}, {"state": half["g64"]}, {"state": half["g32"]}, ["state"])


def test_pstep_8_is_refused_and_writes_nothing(dev):
    """pstep 1 and 7 are served (above); 8 would overrun the eff / agg / er arrays of train_backward_chunk and is refused by
    ag_backward with its "not served" error before anything is enqueued."""
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    from adaptigraph_amd.context import ptr, current_stream
    N, n_p, n_his, _ = BS.CONFIGS["tool_row"]
    bt = BS.make_batch(N, n_p, n_his)
    edges = _edge_list(bt["recv_l"], bt["send_l"], N, dev)
    W = TR.make_weights(5, n_his)
    eng = ag.Engine(dev, pstep=8, n_his=n_his, rel_dim=5 + 3 * n_his)
    w = [_t(W[k], dev) for k in TR.KEYS]
    gw = [torch.full_like(x, 7.0) for x in w]
    dstate = torch.full(bt["state"].shape, 7.0, device=dev)
    B = len(bt["recv_l"])
    phys = torch.cat([_t(bt["phys"], dev), torch.zeros(B, N - n_p, device=dev)], 1).contiguous()
    group = torch.cat([_t(bt["p_instance"], dev), torch.zeros(B, N - n_p, 1, device=dev)], 1).contiguous()
    ins = [_t(bt["state"], dev), _t(bt["attrs"], dev), _t(bt["action"], dev), phys, group]
    gp, gm = _t(bt["gp"], dev), _t(bt["gm"], dev)
    arr = lambda ts: (C.c_void_p * 22)(*[x.data_ptr() for x in ts])   # noqa: E731
    rc = eng.lib.ag_backward(eng.ctx, current_stream(dev), *[ptr(x) for x in ins], 1, ptr(edges.recv), ptr(edges.send),
                             ptr(edges.row_ptr), ptr(edges.n_edges), edges.edge_cap, B, N, n_p, arr(w), ptr(gp), ptr(gm),
                             ptr(dstate), arr(gw))
    assert rc == _lib.AG_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="pstep 8 not served"):
        eng.check(rc)
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in gw + [dstate])
    eng.close()


# ------------------------------------------------------------------------------------------------ B. the batch-chunk loop
def test_autograd_backward_in_chunks(dev):
    """ag_backward_inputs over five graphs in chunks of 1, 2 and 3 (short last chunks; a chunk that is the empty graph alone):
    dstate, dphys and daction carry the bits of the unchunked call, the weight gradients - summed over the chunks in chunk
    order - meet the float64 bar, and a second call at the same chunk size gives the same bits."""
    N, n_p, n_his, pstep = BS.CONFIGS["tool_row"]
    bt, W, g64, g32, _ = _case("tool_row", 5)
    model = _model(dev, W, n_his=n_his, pstep=pstep).train()
    edges = _edge_list(bt["recv_l"], bt["send_l"], N, dev)
    eng = model.engine(dev)
    run = lambda: _engine_grads(model, bt, dev, edges, diff=True)   # noqa: E731
    whole, pos = _chunked(eng, 0, run)
    bad = _compare("unchunked", whole, g64, g32, BS.NAMES)
    for chunk in (1, 2, 3):
        g, p = _chunked(eng, chunk, run)
        g2, _ = _chunked(eng, chunk, run)
        assert torch.equal(p, pos), chunk
        for k in ("state", "phys", "action"):
            assert torch.equal(g[k], whole[k]), (chunk, k)
        for k in BS.NAMES:
            assert torch.equal(g[k], g2[k]), (chunk, k)
        bad += _compare(f"chunk {chunk}", g, g64, g32, TR.KEYS)
    assert not bad, bad


def _fixture_bars(f, grads, label, with_f64):
    bad = []
    g64 = _f64_grads(f)[0] if with_f64 else None
    for k, t in zip(TR.KEYS, grads):
        ref, g = f["g::" + k], t.cpu().numpy()
        err = np.abs(g - ref).max()
        line = f"  {label} {k}: vs reference {err:.3e} (bar {grad_tol(f, k):.3e})"
        if not err <= grad_tol(f, k):
            bad.append((k, "vs reference", float(err)))
        if with_f64 and "err64::" + k in f:
            e64 = np.abs(g - g64[k]).max()
            line += f", vs float64 {e64:.3e}, reference's own {float(f['err64::' + k]):.3e}"
            if not e64 <= 4 * float(f["err64::" + k]) + 1e-7 * np.abs(g64[k]).max():
                bad.append((k, "vs float64", float(e64)))
        print(line)
    return bad


@pytest.mark.parametrize("name", ["train_rope.npz", "train_losses_rope.npz"])
def test_train_step_in_chunks(dev, name):
    """TrainStep (ag_train_step / ag_train_step_losses) with the forward and the backward chunked (one option feeds both), chunks
    of 1 and 3: the predictions are the bits of the unchunked step, loss and gradients meet the bars the fixture's own tests use
    (tests/test_gpu_train_step.py, tests/test_gpu_set_losses.py)."""
    f = TR.load_fixture(name)
    losses = fixture_losses(f) if "loss_names" in f else None
    data = _data(f, dev)
    k = _max_edges(data)
    ts, _ = _train_step(dev, f, lr=0.0, losses=losses)
    ts.step(data, max_edges=k)
    ts.check()
    pred0 = ts.last_pred.clone()
    bad = []
    for chunk in (1, 3):
        loss = float(_chunked(ts.engine, chunk, lambda: ts.step(data, max_edges=k)))
        ts.check()
        print(name, "chunk", chunk, "loss", loss, "reference", float(f["loss_sum"]))
        assert torch.equal(ts.last_pred, pred0), chunk
        assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"])) + 1e-7
        bad += _fixture_bars(f, ts.grad, f"{name} chunk {chunk}", with_f64=losses is None)
    assert not bad, bad


def test_accumulated_step_in_chunks(dev):
    """step_parts over [graph 0], [graphs 1..3] with chunks of 2: the second part runs two chunks whose weight gradients join the
    first part's sums in fp64 (the `wide` k_reduce).  Bars of the whole step."""
    f = TR.load_fixture("train_rope.npz")
    ts, _ = _train_step(dev, f, lr=0.0)
    parts = [_data(f, dev, idx=[0]), _data(f, dev, idx=[1, 2, 3])]
    loss = float(_chunked(ts.engine, 2, lambda: ts.step_parts(parts, max_edges=[_max_edges(d) for d in parts])))
    ts.check()
    print("two parts, chunk 2: loss", loss, "reference", float(f["loss_sum"]))
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"])) + 1e-7
    bad = _fixture_bars(f, ts.grad, "two parts, chunk 2", with_f64=True)
    assert not bad, bad


def test_ppm_gradient_in_chunks(dev):
    """ag_ppm_grad_step on the rope fixture's three interactions (repeat 2, 4, 3; per-particle parameter) in chunks of 1 and 2:
    a row's reductions walk its own rows only, so captured states, errors and the (3, 120) gradient carry the
    bits of the unchunked call - which meets the fixture's bar against float64."""
    import adaptigraph_amd as ag
    f = S.load("rope")
    ppm, inits, reals, acts = _problem(f, "rope", dev)
    eng = ppm.model.engine(dev)

    def run():
        out = {}
        err, grad = ag.dynamics_error_grad_device(f["particles::phys"], ppm, inits, reals, acts, _out=out)
        return err, grad, out["state_seqs"].clone(), out["chamfer"].clone()
    e0, g0, s0, c0 = _chunked(eng, 0, run)
    assert g0.shape == (3, 120) and np.abs(g0).max() > 0
    lim = S.bar(f["particles::dphys_64"], f["particles::dphys"])
    print(f"ppm dphys: error {np.abs(g0 - f['particles::dphys_64']).max():.3e}, bar {lim:.3e}")
    assert np.abs(g0 - f["particles::dphys_64"]).max() <= lim
    for chunk in (1, 2):
        e, g, s, c = _chunked(eng, chunk, run)
        assert e == e0 and torch.equal(s, s0) and torch.equal(c, c0), chunk
        assert np.array_equal(g, g0), (chunk, float(np.abs(g - g0).max()))


# ------------------------------------------------------------------------------------------------ C. split-K beyond one K tile
def _padded(edges, cap, dev):
    """the same EdgeList with recv / send padded to `cap` columns"""
    from adaptigraph_amd.graph import EdgeList
    B, have = edges.recv.shape
    pad = torch.zeros((B, cap - have), dtype=torch.int32, device=dev)
    return EdgeList(torch.cat([edges.recv, pad], 1).contiguous(), torch.cat([edges.send, pad], 1).contiguous(), edges.row_ptr,
                    edges.n_edges, edges.N)


def test_split_k_slabs_through_train_step(dev):
    """linear_dw's slab is 32 rows (one K tile of k_gemm) up to 32,768 rows and grows beyond.  TrainStep's edge rows per graph are
    the caller's max_edges, so with four graphs of about 1,150 edges: max_edges 8192 -> 32,768 rows, slab 32, exactly 1,024
    slabs; 8193 -> 32,772 rows, slab 64 (two K tiles), 513 slabs, the last of 4 rows; the real maximum -> the usual path.  All
    three meet the float64 bar on every weight gradient, and their predictions are the same bits."""
    import adaptigraph_amd as ag
    N, n_p, n_his, pstep = BS.CONFIGS["tool_row"]
    bt = BS.dense_batch(N, n_p, n_his, B=4, per_recv=12, seed=11)
    for b in range(1, 4):                                                # graphs of different sizes: 1,164 down to 1,128 edges
        keep = 12 * (N - b)
        bt["recv_l"][b], bt["send_l"][b] = bt["recv_l"][b][:keep], bt["send_l"][b][:keep]
    rng = np.random.default_rng(12)
    fut = (bt["state"][:, -1:, :n_p] + rng.normal(0, 0.02, (4, 1, n_p, 3))).astype(np.float32)
    W = TR.make_weights(5, n_his)

    def loss(step, state, action, t):
        pos, mot = step(state, action)
        torch.nn.functional.mse_loss(pos, t(fut[:, 0])).backward()
        return pos, mot
    g64, p64, _ = BS.restate(bt, W, pstep, torch.float64, dev, loss=loss)
    g32, _, _ = BS.restate(bt, W, pstep, torch.float32, dev, loss=loss)
    model = _model(dev, W, n_his=n_his, pstep=pstep)
    edges = _padded(_edge_list(bt["recv_l"], bt["send_l"], N, dev), 8193, dev)
    data = dict(_graph(bt, dev, edges), state_future=_t(fut, dev))
    ts = ag.TrainStep(model, lr=0.0, n_future=1)
    bad, preds = [], []
    for max_edges in (12 * N, 8192, 8193):
        ts.step(data, max_edges=max_edges)
        ts.check()
        preds.append(ts.last_pred.clone())
        bad += _compare(f"max_edges {max_edges}", dict(zip(TR.KEYS, ts.grad)), g64, g32, TR.KEYS)
    np.testing.assert_allclose(preds[0][0].cpu().numpy(), p64, atol=1e-4)
    assert torch.equal(preds[0], preds[1]) and torch.equal(preds[0], preds[2])
    assert not bad, bad


def test_split_k_slabs_all_real_rows(dev):
    """ag_backward with 4 x 8,400 real edge rows (N = 300, 28 senders per receiver): 33,600 rows, slab 64, 525 slabs, every row
    live.  Bar as above.  As at granular size (tests/test_gpu_train.py::test_larger_models_match_float64_restatement), with ~10^7
    ReLU inputs a few sit within fp32 rounding of zero, the gradient jumps there, and which side an fp32 run lands on is luck:
    the bar's 4 err32 term is what allows for it - when the fp32 restatement happens to land on the other side too.  It need not:
    at seed 21 (a head-layer ReLU input of 2.4e-8) the engine was 1.9e-3 of max|g64| off on non_rigid_predictor.linear_1.weight,
    and so, to four digits, was the fp32 restatement on the CPU, while the one on the GPU stayed on float64's side (err32
    1.9e-6); at seed 57 the engine was 4.71e-4 off on relation_propagator.linear.weight and 2.58e-4 on dstate, and the float64
    gradients themselves move by exactly 4.71e-4 and 2.58e-4 when the weights are perturbed by fp32 rounding.  Neither is the
    split-K path's doing (node-side tensors of 1,200 rows, one-tile slabs, show the same error).  BS.SPLITK_SEED is therefore
    chosen by the reference alone: a seed at which such perturbations move float64 by 2e-7 (tests/test_backward_shapes.py).
    Observed figures: docs/EXPERIMENTS.md."""
    N, n_p, n_his, pstep = BS.SPLITK_CONFIG
    bt = BS.dense_batch(N, n_p, n_his, B=4, per_recv=28, seed=BS.SPLITK_SEED)
    W = TR.make_weights(5, n_his)
    g64, p64, m64 = BS.restate(bt, W, pstep, torch.float64, dev)
    g32, _, _ = BS.restate(bt, W, pstep, torch.float32, dev)
    assert np.abs(m64).max() < 100.0
    model = _model(dev, W, n_his=n_his, pstep=pstep).train()
    edges = _edge_list(bt["recv_l"], bt["send_l"], N, dev)
    assert edges.n_edges.cpu().tolist() == [8400] * 4
    g, pos = _engine_grads(model, bt, dev, edges, diff=False)
    np.testing.assert_allclose(pos.cpu().numpy(), p64, atol=1e-4)
    bad = _compare("33,600 rows", g, g64, g32, TR.KEYS + ["state"])
    assert not bad, bad
