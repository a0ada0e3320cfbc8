"""CPU checks of the device-resident training step: the three exports at the boundary, the no-CPU-fallback rule of TrainStep,
and the optimiser-state mapping to and from torch.optim.Adam.state_dict() (a pure host function)."""
import os
import re
import subprocess

import pytest
import torch

import train_restate as TR
from test_train import CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["ag_ctx_load_weights_device", "ag_adam_step", "ag_train_step"]


def _cpu_model():
    import adaptigraph_amd as ag
    mat = {"material_index": {"rope": 0}, "rope": {"physics_params": [{"name": "r", "use": True}]}}
    return ag.DynamicsPredictor(CFG, mat, {"n_his": 4, "materials": ["rope"]}, "cpu")


@pytest.mark.parametrize("name", NEW_EXPORTS)
def test_train_step_exports_are_declared_and_exported(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % name, src)
    from adaptigraph_amd import _lib
    assert name in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T %s$" % name, out, flags=re.M)
    assert hasattr(_lib.load(), name)


def test_header_says_the_three_exports_never_wait():
    hdr = open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()
    table = hdr[hdr.index("WHICH ENTRY POINTS BLOCK THE HOST"):hdr.index("#ifndef ADAPTIGRAPH_AMD_H")]
    row = [ln for ln in table.splitlines() if "ag_train_step" in ln]
    assert len(row) == 1 and all(n in row[0] for n in NEW_EXPORTS) and "NEVER" in row[0]


def test_train_step_on_a_cpu_model_raises():
    import adaptigraph_amd as ag
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # the model's parameters are on the host, GPU present or not
        ag.TrainStep(_cpu_model())


def test_api_file_keeps_no_pack_call_lists():
    """The per-layer pack_layer / pack_first call lists of ag_ctx_load_weights are gone: host and device packers share ag_optim.hip."""
    api = open(os.path.join(ROOT, "adaptigraph_amd", "csrc", "ag_api.hip")).read()
    assert "pack_layer" not in api and "pack_first" not in api


def _order(model):
    ids = {id(p): k for k, p in enumerate(model.ordered_parameters())}
    return [ids[id(p)] for p in model.parameters()]


def test_optimizer_state_round_trips_through_torch_adam():
    from adaptigraph_amd.train_step import adam_state_to_torch, adam_state_from_torch
    model = _cpu_model().train()
    order = _order(model)
    assert sorted(order) == list(range(22))
    gen = torch.Generator().manual_seed(0)
    shapes = [p.shape for p in model.ordered_parameters()]
    m = [torch.randn(s, generator=gen) for s in shapes]
    v = [torch.rand(s, generator=gen) for s in shapes]
    hyper = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    sd = adam_state_to_torch(7, m, v, hyper, order)
    # torch's own layout: a real Adam over the model's parameters loads it and gives it back
    opt = torch.optim.Adam(model.parameters(), lr=1.0)
    ref = opt.state_dict()
    assert sorted(sd["param_groups"][0].keys()) == sorted(ref["param_groups"][0].keys())
    opt.load_state_dict(sd)
    back = opt.state_dict()
    g = back["param_groups"][0]
    assert g["lr"] == 3e-4 and tuple(g["betas"]) == (0.8, 0.99) and g["eps"] == 1e-7 and g["weight_decay"] == 0.01
    assert g["params"] == list(range(22)) and not g["amsgrad"] and not g["maximize"]
    assert sorted(back["state"].keys()) == list(range(22))
    for i, p in enumerate(model.parameters()):
        st = opt.state[p]
        assert float(st["step"]) == 7.0
        assert torch.equal(st["exp_avg"], m[order[i]]) and torch.equal(st["exp_avg_sq"], v[order[i]])
        assert st["exp_avg"].shape == p.shape
    step, m2, v2, h2 = adam_state_from_torch(back, order)
    assert step == 7 and h2 == hyper
    for k in range(22):
        assert torch.equal(m2[k], m[k]) and torch.equal(v2[k], v[k])
    # a fresh optimiser has no state
    sd0 = adam_state_to_torch(0, m, v, hyper, order)
    assert sd0["state"] == {}
    assert adam_state_from_torch(sd0, order)[:3] == (0, None, None)
    assert adam_state_from_torch(ref, order)[0] == 0
    # the state of a real Adam after real steps maps in: key i is parameter i of model.parameters()
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt2 = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt2.step()
    opt2.step()
    step, m3, v3, _ = adam_state_from_torch(opt2.state_dict(), order)
    assert step == 2
    for k, p in enumerate(model.ordered_parameters()):
        assert torch.equal(m3[k], opt2.state[p]["exp_avg"])
    with pytest.raises(NotImplementedError):
        bad = opt2.state_dict()
        bad["param_groups"][0]["amsgrad"] = True
        adam_state_from_torch(bad, order)


def test_state_dict_keys_follow_the_load_order():
    model = _cpu_model()
    assert [k for k, _ in model.named_parameters()] == TR.KEYS   # model.parameters() order = ag_ctx_load_weights order
    assert _order(model) == list(range(22))
