"""CPU checks of the training path: the ag_backward boundary, the parameter freeze contract of DynamicsPredictor.train(),
and the float64 torch restatement (tests/train_restate.py) against the reference's own gradients (tests/golden/train_*.npz)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import train_restate as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["train_rope.npz", "train_cloth.npz", "train_clamp.npz"]
CFG = dict(verbose=False, nf_particle=150, nf_relation=150, nf_effect=150, nf_physics=10, attr_dim=2, state_dim=0, offset_dim=0,
           action_dim=3, density_dim=0, pstep=3, sequence_len=4, rel_particle_dim=0, rel_attr_dim=2, rel_group_dim=1,
           rel_distance_dim=3, rel_density_dim=0)


def test_backward_is_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint ag_backward\s*\(", src)
    from adaptigraph_amd import _lib
    assert "ag_backward" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T ag_backward$", out, flags=re.M)
    assert hasattr(_lib.load(), "ag_backward")


def test_train_mode_unfreezes_parameters():
    import adaptigraph_amd as ag
    mat = {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "r", "use": True}]}}
    model = ag.DynamicsPredictor(CFG, mat, {"n_his": 4, "materials": ["rope"]}, "cpu")
    params = list(model.parameters())
    assert len(params) == 22
    assert not any(p.requires_grad for p in params)              # a fresh model stays frozen: inference callers see no change
    assert model.train() is model
    assert all(p.requires_grad for p in params) and model.training
    model.eval()
    assert not any(p.requires_grad for p in params) and not model.training
    model.requires_grad_(True)                                   # the plain nn.Module switch keeps working
    assert all(p.requires_grad for p in params)
    model.train(False)
    assert not any(p.requires_grad for p in params)
    names = [n for n, _ in model.named_parameters()]
    assert [id(p) for p in model.ordered_parameters()] == [id(dict(model.named_parameters())[k]) for k in TR.KEYS]
    assert sorted(names) == sorted(TR.KEYS)


def grad_tol(f, k):
    """max|g - g_ref| bar per tensor: 1e-4 max|g_ref| + 1e-7, widened by the reference's own fp32 error against float64 where it is
    larger than that (train_clamp: linear_2 scaled by ~1e4 leaves the reference's fp32 gradients 2e-4 off float64)."""
    return 1e-4 * np.abs(f["g::" + k]).max() + 1e-7 + 2.0 * float(f.get("err64::" + k, 0.0))


def _restated_grads(f):
    inp = TR.fixture_inputs(f, torch.float64)
    B, N = inp["attrs"].shape[:2]
    recv, send = TR.fixture_edges(f, B, N)
    W = TR.weights(f, torch.float64)
    inp["state"].requires_grad_(True)
    step = lambda s, a: TR.forward(W, s, inp["attrs"], a, inp["phys"], inp["group"], recv, send, inp["n_p"],  # noqa: E731
                                   int(f["pstep"]))
    loss = TR.chain_loss(step, inp, int(f["n_future"]))
    loss.backward()
    return loss.item(), {k: W[k].grad.numpy() for k in TR.KEYS}, inp["state"].grad.numpy()


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_reference_gradients(name):
    f = TR.load_fixture(name)
    loss, g, dstate = _restated_grads(f)
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"]))
    if "loss_sum_64" in f:
        assert abs(loss - float(f["loss_sum_64"])) <= 1e-12 * abs(loss)
    for k in TR.KEYS:
        ref = f["g::" + k]
        err = np.abs(g[k] - ref).max()
        assert err <= grad_tol(f, k), (k, err, np.abs(ref).max())
        if "err64::" + k in f:   # the reference's fp32 error, re-derived from our float64 gradients (up to the 14-bit rounding)
            assert abs(err - float(f["err64::" + k])) <= 4e-5 * np.abs(ref).max() + 1e-9, (k, err, float(f["err64::" + k]))
    assert np.abs(dstate - f["dstate0"]).max() <= 1e-4 * np.abs(f["dstate0"]).max() + 1e-7
    if "dstate0_64" in f:
        assert np.abs(dstate - f["dstate0_64"]).max() <= 1e-10 * np.abs(f["dstate0_64"]).max()


def test_clamp_fixture_has_both_signs():
    m = TR.load_fixture("train_clamp.npz")["pred_motion"]
    assert (m > 100).any() and (m < -100).any() and (np.abs(m) <= 100).any()
