"""The host code between the Python entry points and the C-ABI, on the CPU: DynamicsPredictor._inputs (model inputs), ModelInputs.c_args
(the 14-argument forward prefix), forward_dynamics._rollout_params / _pusher_offsets / _physics (the rollout's parameters).

Needs neither a GPU nor the built library.  Every expected value is written out here, restated in numpy from the reference's
src/dynamics/gnn/model.py:186-207,222 and src/planning/forward_dynamics.py:16-21,42-78,152-153 - never taken from the code under test.
"""
import itertools
import types

import numpy as np
import pytest
import torch

import adaptigraph_amd as ag
from adaptigraph_amd import _lib
from adaptigraph_amd import forward_dynamics as FD

B, N_P, N_S, N_INST, N_HIS = 2, 5, 2, 3, 4
N = N_P + N_S
# four edges per graph as (receiver, sender), NOT in receiver order; receivers 2, 3, 4, 6 of graph 0 have degree 0
EDGES = [[(5, 0), (1, 2), (5, 6), (0, 1)],
         [(6, 3), (2, 4), (2, 0), (3, 6)]]
PAD_ROW = 2                                   # the dense form carries one all-zero row here (pad_torch's padding)
# the same edges in CSR order: by receiver, equal receivers in the order given (the reference's nonzero order)
CSR_RECV = np.array([[0, 1, 5, 5], [2, 2, 3, 6]], np.int32)
CSR_SEND = np.array([[1, 2, 0, 6], [4, 0, 6, 3]], np.int32)
CSR_ROW_PTR = np.array([[0, 1, 2, 2, 2, 2, 4, 4], [0, 0, 0, 2, 3, 3, 3, 4]], np.int32)


def _model():
    cfg = dict(verbose=False, nf_particle=150, nf_relation=150, nf_effect=150, nf_physics=10, attr_dim=2, state_dim=0,
               offset_dim=0, action_dim=3, density_dim=0, pstep=3, sequence_len=4, rel_particle_dim=0, rel_attr_dim=2,
               rel_group_dim=1, rel_distance_dim=3, rel_density_dim=0)
    mat = {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "r", "use": True}]}}
    return ag.DynamicsPredictor(cfg, mat, {"n_his": N_HIS, "materials": ["rope"]}, "cpu")


def _dense():
    Rr, Rs = np.zeros((B, 5, N), np.float32), np.zeros((B, 5, N), np.float32)
    for b, es in enumerate(EDGES):
        rows = [r for r in range(5) if r != PAD_ROW]
        for row, (r, s) in zip(rows, es):
            Rr[b, row, r] = Rs[b, row, s] = 1
    return torch.from_numpy(Rr), torch.from_numpy(Rs)


def _edge_list(n=N):
    t = lambda a: torch.from_numpy(a.copy())   # noqa: E731
    return ag.EdgeList(t(CSR_RECV), t(CSR_SEND), t(CSR_ROW_PTR), torch.full((B,), 4, dtype=torch.int32), n)


def _raw(seed=0):
    """forward()'s arguments the way a caller may hand them over: float64 attrs, a transposed (non-contiguous) action."""
    rng = np.random.default_rng(seed)
    state = torch.from_numpy(rng.normal(0, 1, (B, N_HIS, N, 3)).astype(np.float32))
    attrs = torch.from_numpy(rng.normal(0, 1, (B, N, 2)))                                  # float64
    action = torch.from_numpy(rng.normal(0, 1, (B, 3, N)).astype(np.float32)).transpose(1, 2)
    assert not action.is_contiguous()
    p_instance = torch.from_numpy((rng.random((B, N_P, N_INST)) < 0.5).astype(np.float32))
    return state, attrs, action, p_instance


def _param(shape, seed=1):
    return torch.from_numpy(np.random.default_rng(seed).uniform(0.1, 0.9, (B,) + shape).astype(np.float32))


def _build(model, raw, pp, dense=True, edges=None, diff=False, **more):
    state, attrs, action, p_instance = raw
    Rr, Rs = _dense() if dense else (None, None)
    return model._inputs(torch.device("cpu"), state, attrs, Rr, Rs, p_instance, action, edges, dict(rope_physics_param=pp, **more),
                         diff=diff)


# ------------------------------------------------------------------------------------------------ model inputs
@pytest.mark.parametrize("dense", [True, False], ids=["Rr_Rs", "EdgeList"])
@pytest.mark.parametrize("pshape", [(1,), (N_P,)], ids=["B_1", "B_np"])
def test_model_inputs(pshape, dense):
    model, raw, pp = _model(), _raw(), _param(pshape)
    given = None if dense else _edge_list()
    inp = _build(model, raw, pp, dense=dense, edges=given)
    state, attrs, action, p_instance = raw
    for name, shape in (("state", (B, N_HIS, N, 3)), ("attrs", (B, N, 2)), ("action", (B, N, 3)), ("phys", (B, N)),
                        ("group", (B, N, N_INST))):
        t = getattr(inp, name)
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, name
        assert not t.requires_grad, name
    assert (inp.B, inp.N, inp.n_inst, inp.n_p) == (B, N, N_INST, N_P)
    assert np.array_equal(inp.state.numpy(), state.numpy())
    assert np.array_equal(inp.attrs.numpy(), attrs.numpy().astype(np.float32))
    assert np.array_equal(inp.action.numpy(), np.ascontiguousarray(action.numpy()))
    # model.py:191-207: (B,1) repeated over the n_p object rows, or (B,n_p) as it is; zeros on the n_s tool rows
    want = np.zeros((B, N), np.float32)
    want[:, :N_P] = np.repeat(pp.numpy(), N_P, 1) if pshape == (1,) else pp.numpy()
    assert np.array_equal(inp.phys.numpy(), want)
    assert np.array_equal(inp.phys.numpy()[:, :N_P], np.broadcast_to(pp.numpy(), (B, N_P))) and np.all(inp.phys.numpy()[:, N_P:] == 0)
    assert np.array_equal(inp.group.numpy()[:, :N_P], p_instance.numpy()) and np.all(inp.group.numpy()[:, N_P:] == 0)
    e = inp.edges
    if not dense:
        assert e is given
    assert e.N == N and e.edge_cap >= 4
    for t in (e.recv, e.send, e.row_ptr, e.n_edges):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert e.n_edges.tolist() == [4, 4]
    assert np.array_equal(e.recv.numpy()[:, :4], CSR_RECV) and np.array_equal(e.send.numpy()[:, :4], CSR_SEND)
    assert np.array_equal(e.row_ptr.numpy(), CSR_ROW_PTR)


def test_model_inputs_refuse_what_the_reference_asserts():
    model, raw = _model(), _raw()
    state, attrs, action, p_instance = raw
    with pytest.raises(AssertionError):                                                    # model.py:186-187: two keys
        _build(model, raw, _param((1,)), cloth_physics_param=_param((1,)))
    with pytest.raises(AssertionError):                                                    # ... and none
        model._inputs(torch.device("cpu"), state, attrs, *_dense(), p_instance, action, None, {})
    with pytest.raises(AssertionError):                                                    # model.py:222
        _build(model, (state, attrs, None, p_instance), _param((1,)))
    with pytest.raises(AssertionError):                                                    # an EdgeList of another graph size
        _build(model, raw, _param((1,)), dense=False, edges=_edge_list(N + 1))
    with pytest.raises(AssertionError):                                                    # neither form of edges
        _build(model, raw, _param((1,)), dense=False)
    with pytest.raises(AssertionError):                                                    # state of another history length
        _build(model, (state[:, 1:], attrs, action, p_instance), _param((1,)))


# weights over (B, N) that span several binades: in row 0 an fp32 running sum loses every one of the four small terms, the
# float64 sum rounded once does not (2**24 + 4 is an fp32 number)
W_PHYS = np.array([[2.0 ** 24, 1.0, 1.0, 1.0, 1.0, -3.0, 0.5],
                   [1e-3, -3.5, 2.0 ** -20, 1024.25, 7e5, 11.0, 2.0 ** 30]], np.float32)


def test_differentiable_inputs_expand_rows_sums_in_float64():
    model, raw = _model(), _raw()
    pp = _param((1,)).requires_grad_(True)
    act = raw[2].clone().requires_grad_(True)
    inp = _build(model, (raw[0], raw[1], act, raw[3]), pp, diff=True)
    assert inp.phys.requires_grad and inp.action.requires_grad
    assert not inp.attrs.requires_grad and not inp.group.requires_grad
    assert inp.phys.dtype == torch.float32 and inp.phys.is_contiguous() and inp.action.is_contiguous()
    (inp.phys * torch.from_numpy(W_PHYS)).sum().backward()
    want = W_PHYS[:, :N_P].astype(np.float64).sum(1, keepdims=True).astype(np.float32)    # the tool columns give nothing
    assert want[0, 0] == np.float32(2.0 ** 24 + 4)
    assert pp.grad.shape == (B, 1) and pp.grad.dtype == torch.float32
    assert np.array_equal(pp.grad.numpy(), want)
    # (B, n_p): the object columns of the gradient, unchanged
    pq = _param((N_P,)).requires_grad_(True)
    inp = _build(model, raw, pq, diff=True)
    (inp.phys * torch.from_numpy(W_PHYS)).sum().backward()
    assert np.array_equal(pq.grad.numpy(), W_PHYS[:, :N_P])
    # the gradient toward action reaches the caller's (transposed) tensor
    g = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (B, N, 3)).astype(np.float32))
    inp = _build(model, (raw[0], raw[1], act, raw[3]), _param((1,)), diff=True)
    (inp.action * g).sum().backward()
    assert np.array_equal(act.grad.numpy(), g.numpy())


def test_plain_inputs_carry_no_graph():
    model, raw = _model(), _raw()
    for pshape in ((1,), (N_P,)):
        pp = _param(pshape).requires_grad_(True)
        act = raw[2].clone().requires_grad_(True)
        inp = _build(model, (raw[0], raw[1], act, raw[3]), pp)
        for t in (inp.state, inp.attrs, inp.action, inp.phys, inp.group):
            assert not t.requires_grad


def test_forward_prefix_in_abi_order():
    """ag_forward(ctx, stream, state, attrs, action, phys, group, n_inst, recv, send, row_ptr, n_edges, edge_cap, B, N, n_p, ...)."""
    import ctypes as C
    inp = _build(_model(), _raw(), _param((1,)))
    got = inp.c_args()
    e = inp.edges
    want = (inp.state.data_ptr(), inp.attrs.data_ptr(), inp.action.data_ptr(), inp.phys.data_ptr(), inp.group.data_ptr(), N_INST,
            e.recv.data_ptr(), e.send.data_ptr(), e.row_ptr.data_ptr(), e.n_edges.data_ptr(), 5, B, N, N_P)
    assert len(got) == 14 and len({w for w in want[:5] + want[6:10]}) == 9                 # nine distinct buffers
    for k, (g, w) in enumerate(zip(got, want)):
        pointer = k < 5 or 6 <= k < 10
        assert isinstance(g, C.c_void_p) == pointer, k
        assert (g.value if pointer else g) == w, k
        assert pointer or type(g) is int, k


# ------------------------------------------------------------------------------------------------ rollout parameters
PTS = {1: [[0.0, 0.0, 0.12]],
       3: [[0.0, 0.0, 0.1], [0.0, 0.05, 0.1], [0.0, -0.05, 0.1]],
       5: [[0.0, 0.0, 0.1], [0.0, 0.05, 0.1], [0.0, 0.025, 0.1], [0.0, -0.025, 0.1], [0.0, -0.05, 0.1]]}


def _task(M, grip=False, cta=False, n_his=N_HIS):
    return dict(adj_thresh=0.5, topk=10, connect_tools_all=cta, sim_real_ratio=10, push_length=0.1, gripper_enable=grip,
                max_n=1, max_nR=4000, n_his=n_his, eef_num=M, material="rope", pusher_points=PTS[M], material_dims={"rope": 1},
                material_indices={"rope": 0})


def _ppm(task, physics_param=None):
    return types.SimpleNamespace(task_config=task, eef_num=task["eef_num"], material="rope", material_dims=task["material_dims"],
                                 material_indices=task["material_indices"], adj_thresh=0.5,
                                 physics_param={"rope": torch.tensor([0.5])} if physics_param is None else physics_param)


@pytest.mark.parametrize("grip,cta,M", list(itertools.product([False, True], [False, True, 1], [1, 5])))
def test_rollout_params_field_by_field(grip, cta, M):
    task = _task(M, grip, cta)
    p = FD._rollout_params(task, _ppm(task), _model(), 6, 3, 120, 1, 0.25)
    assert isinstance(p, _lib.AgRolloutParams)
    got = {name: getattr(p, name) for name, _ in _lib.AgRolloutParams._fields_}
    want = dict(B=6, H=3, N_o=120, M=M, topk=10, connect_tools_all=1 if cta else 0, max_nR=4000, y_mode=1,
                adj_thresh=float(np.float32(0.5)), gripper_offset=float(np.float32(0.01 * 10)) if grip else 0.0,
                gripper_enable=1 if grip else 0, physics_param=0.25)
    assert got == want
    assert FD._rollout_params(task, _ppm(task), _model(), 1, 1, 7, 0, 0.75).y_mode == 0


@pytest.mark.parametrize("M", [1, 5])
def test_pusher_offsets(M):
    offs = FD._pusher_offsets(_task(M), M)
    want = {1: [0.0] * 8, 5: [0.0, 0.05 * 10, 0.025 * 10, -0.025 * 10, -0.05 * 10, 0.0, 0.0, 0.0]}[M]
    assert len(offs) == 8 and list(offs) == [float(np.float32(w)) for w in want]


def test_rollout_params_refuse_what_the_kernels_lack():
    with pytest.raises(NotImplementedError, match="pusher not implemented"):
        FD._pusher_offsets(_task(3), 3)                                                    # forward_dynamics.py:77-78
    with pytest.raises(NotImplementedError, match="pusher not implemented"):
        FD._pusher_offsets(_task(5), 1)                                                    # five points for one tool particle
    task = _task(1, n_his=5)
    with pytest.raises(AssertionError, match="must be the model's n_his"):
        FD._rollout_params(task, _ppm(task), _model(), 6, 3, 120, 0, 0.5)


def test_physics_scalar_vector_missing():
    dev, N_o = torch.device("cpu"), 6
    task = _task(1)
    assert FD._physics(_ppm(task), None, N_o, dev) == (0.5, None)                          # the optimizer's own, one value
    assert FD._physics(_ppm(task), {"rope": torch.tensor([[0.125]], dtype=torch.float64)}, N_o, dev) == (0.125, None)
    vec = torch.arange(N_o, dtype=torch.float64) / 8
    val, got = FD._physics(_ppm(task), {"rope": vec.reshape(1, N_o)}, N_o, dev)            # model.py:204: one value per particle
    assert val == 0.0 and got.device == dev and got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got.numpy(), (np.arange(N_o) / 8).astype(np.float32))
    assert FD._physics(_ppm(task, {}), None, N_o, dev) == (0.0, None)                      # forward_dynamics.py:152-153: zeros
    assert FD._physics(_ppm(task), {"cloth": torch.tensor([0.5])}, N_o, dev) == (0.0, None)
    with pytest.raises(AssertionError):
        FD._physics(_ppm(task), {"rope": torch.zeros(N_o - 1)}, N_o, dev)
