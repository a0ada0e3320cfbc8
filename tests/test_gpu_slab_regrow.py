"""A call sizes its workspace by running its own carve (csrc/ag_host.h: carve_slab), so the slab of a call slot follows the call
shapes a context sees (-m gpu).  For every entry point that carves: small, large, small calls on ONE context and stream - the
second small call has the bits of the first and of the same call on a fresh context, and makes no allocation (the slab the
large call grew serves it).  Small: B = 2, N_o = 12, M = 1, topk = 5; large: B = 5, N_o = 40; edge capacities follow the
graphs, so nothing overflows (every status is checked)."""
import numpy as np
import pytest
import torch

from test_gpu_train import _model, _edge_list, _synthetic_case
from test_gpu_parity import _ppm
from test_gpu_more import _task, _actions

pytestmark = pytest.mark.gpu

SHAPES = {"small": dict(B=2, n_obj=12, seed=11), "large": dict(B=5, n_obj=40, seed=12)}
TOPK, ADJ, N_FUTURE = 5, 0.8, 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def W():
    from oracle import adaptigraph_oracle as O
    return O.random_weights(7)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


@pytest.fixture(scope="module")
def data(dev):
    """model(**data) / TrainStep.step(data) inputs of both shapes, built once and never written to"""
    out = {}
    for name, s in SHAPES.items():
        f, recv_l, send_l, N = _synthetic_case(dev, s["n_obj"], TOPK, ADJ, 4, 3, s["seed"], B=s["B"])
        rng = np.random.default_rng(s["seed"] + 100)
        B, n_obj = s["B"], s["n_obj"]
        d = {k: _t(f[k], dev) for k in ("state", "attrs", "p_instance", "action")}
        d["phys_physics_param"] = _t(f["physics_param"], dev)
        d["edges"] = _edge_list(recv_l, send_l, N, dev)
        d["state_future"] = _t(f["state"][:, -1:, :n_obj] + rng.normal(0, 0.02, (B, N_FUTURE, n_obj, 3)), dev)
        d["eef_future"] = _t(f["state"][:, -1:] + rng.normal(0, 0.02, (B, N_FUTURE - 1, N, 3)), dev)
        d["action_future"] = _t(np.repeat(f["action"][:, None], N_FUTURE - 1, 1), dev)
        assert int(d["edges"].n_edges.min()) > 0
        out[name] = d
    return out


def _small_large_small(make, run, counts):
    """make() -> a fresh context; run(ctx, shape) -> tensors of one call (overflow raises); counts(ctx) -> ag_ctx_alloc_counts"""
    ctx = make()
    first = [t.clone() for t in run(ctx, "small")]
    run(ctx, "large")
    torch.cuda.synchronize()
    before = counts(ctx)
    second = [t.clone() for t in run(ctx, "small")]
    torch.cuda.synchronize()
    assert counts(ctx) == before, counts(ctx) - before
    fresh = run(make(), "small")
    assert len(first) == len(second) == len(fresh) > 0
    for i, (a, b, c) in enumerate(zip(first, second, fresh)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(a, b), (i, "second small call")
        assert torch.equal(a, c), (i, "fresh context")


def _call_inputs(d):
    return {k: v for k, v in d.items() if k not in ("state_future", "eef_future", "action_future")}


def test_forward(dev, W, data):
    def run(m, shape):
        with torch.no_grad():
            return m(**_call_inputs(data[shape]))                 # ag_forward waits and raises "Exceeds max dims" itself
    _small_large_small(lambda: _model(dev, W), run, lambda m: m.engine(dev).alloc_counts())


def test_backward_inputs(dev, W, data):
    def run(m, shape):
        d = dict(_call_inputs(data[shape]))
        leaves = [d[k].clone().requires_grad_(True) for k in ("state", "action", "phys_physics_param")]
        d["state"], d["action"], d["phys_physics_param"] = leaves
        pos, motion = m.forward_diff(**d)
        (pos.square().sum() + motion.sum()).backward()             # ag_backward_inputs: raises on an overflowed graph
        return [pos.detach(), motion.detach()] + [t.grad for t in leaves]
    _small_large_small(lambda: _model(dev, W), run, lambda m: m.engine(dev).alloc_counts())


def test_train_step_with_gradients(dev, W, data):
    import adaptigraph_amd as ag

    def run(ts, shape):
        d = data[shape]
        loss = ts.step(d, max_edges=int(d["edges"].n_edges.max().item()))
        ts.check()                                                 # status word 0, or it raises
        assert ts._status.tolist()[0] == 0
        return [loss.reshape(1), ts.last_pred] + list(ts.grad)
    # lr = 0: the weights stay, so a repeated call is the same call
    _small_large_small(lambda: ag.TrainStep(_model(dev, W), lr=0.0, n_future=N_FUTURE), run, lambda ts: ts.engine.alloc_counts())


def test_ppm_grad_step_with_gradients(dev, W):
    import adaptigraph_amd as ag
    rng = np.random.default_rng(21)
    prob = {}
    for name, s in SHAPES.items():
        B, n_obj = s["B"], s["n_obj"]
        clouds = [(rng.uniform(-1, 1, (n_obj - b % 2, 3)) * [1.0, 0.05, 1.0]).astype(np.float32) for b in range(B)]
        after = [c + rng.normal(0, 0.02, c.shape).astype(np.float32) for c in clouds]
        acts = list(_actions(np.concatenate(clouds), B, 1, rng.integers(1, 4, B), rng, spread=0.5)[:, 0])
        task = _task("rope", topk=TOPK, adj_thresh=ADJ, max_nobj=n_obj, max_nR=(n_obj + 1) * (TOPK + 1))
        prob[name] = (task, clouds, after, acts)

    def run(m, shape):
        task, clouds, after, acts = prob[shape]
        ppm = _ppm(task, "rope")
        ppm.model, ppm.device = m, dev
        out = {}
        err, grad = ag.dynamics_error_grad_device([0.4], ppm, clouds, after, acts, _out=out)   # raises on a non-zero status
        return [out["state_seqs"], out["chamfer"], torch.from_numpy(np.concatenate([[err], grad.ravel()]))]
    _small_large_small(lambda: _model(dev, W), run, lambda m: m.engine(dev).alloc_counts())


@pytest.mark.parametrize("latency", [-1, 0])
def test_rollout_sharing_first_forward_and_prefix(dev, W, latency):
    """share_first = 1 and share_prefix = 1: the prefix scratch and the shared base graph are carved with the workspaces.  At
    these sizes the default picks the latency-mode chains, which keep their own C rows; latency = 0 makes the shared table real
    (ag_ctx_share_counts says so)."""
    import adaptigraph_amd as ag
    rng = np.random.default_rng(31)
    prob = {}
    for name, s in SHAPES.items():
        B, n_obj = s["B"], s["n_obj"]
        cloud = (rng.uniform(-1, 1, (n_obj, 3)) * [1.0, 0.05, 1.0]).astype(np.float32)
        a = _actions(cloud, B, 1, rng.integers(2, 5, (B, 1)), rng, spread=1.5)
        task = _task("rope", topk=TOPK, adj_thresh=ADJ, max_nR=(n_obj + 1) * (TOPK + 1))
        prob[name] = (torch.from_numpy(cloud).to(dev), torch.from_numpy(a), _ppm(task, "rope"))   # (actions decoded on the host)

    def run(m, shape):
        s0, a, ppm = prob[shape]
        eng = m.engine(dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        with eng.options(share_first=1, share_prefix=1, latency=latency):
            out = ag.dynamics(s0, a, m, dev, ppm, _sync=False, _overflow_flag=flags)["state_seqs"]
            torch.cuda.synchronize()
            assert flags.tolist() == [0, 0]
            if latency == 0:
                assert eng.share_counts()[0] > 0                   # edges of the once-per-call base encode
        return [out]
    _small_large_small(lambda: _model(dev, W), run, lambda m: m.engine(dev).alloc_counts())
