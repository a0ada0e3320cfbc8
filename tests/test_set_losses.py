"""CPU checks of the training set losses: the float64 restatement (tests/set_loss_restate.py) against the reference's own values
and gradients (tests/golden/set_losses.npz, train_losses_rope.npz), the conditions the fixtures were generated under, the host
argument checks of LossSpec, and the three exports of the boundary."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import set_loss_restate as SR
import train_restate as TR
from test_train import grad_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ["ag_set_loss", "ag_set_loss_backward", "ag_train_step_losses"]
SHAPES = [(1, 1, 1), (3, 7, 5), (2, 70, 37), (2, 257, 300), (2, 9, 9)]


def standalone_cases():
    f = TR.load_fixture("set_losses.npz")
    return [{key.split("::", 1)[1]: f[key] for key in f if key.startswith(f"c{k}::")} for k in range(int(f["n_cases"]))]


def fixture_losses(f):
    return [(str(n), float(w)) for n, w in zip(f["loss_names"], f["loss_weights"])]


def test_fixture_cases_are_the_stated_shapes():
    cases = standalone_cases()
    assert [(c["x"].shape[0], c["x"].shape[1], c["y"].shape[1]) for c in cases] == SHAPES
    c = cases[4]
    assert np.array_equal(c["x"][0, 2], c["y"][0, 4])                       # the coincident pair
    c = cases[1]                                                            # both Hausdorff winners lie in the last graph
    _, _, bx, by = SR.winners(c["x"], c["y"])
    assert bx // 7 == 2 and by // 5 == 2


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_restatement_matches_reference_standalone(k):
    c = standalone_cases()[k]
    for name, fn in (("chamfer", SR.chamfer), ("hausdorff", SR.hausdorff)):
        x = torch.from_numpy(c["x"]).double().requires_grad_(True)
        v = fn(x, torch.from_numpy(c["y"]).double())
        v.backward()
        ref, g_ref = float(c[name]), c["g_" + name]
        assert abs(v.item() - ref) <= 1e-5 * abs(ref), (name, v.item(), ref)
        assert abs(v.item() - float(c[name + "_64"])) <= 1e-12 * abs(ref)
        g = x.grad.numpy()
        assert np.isfinite(g).all()
        assert np.abs(g - g_ref).max() <= 1e-4 * np.abs(g_ref).max() + 1e-7, (name, np.abs(g - g_ref).max())
    if k == 4:      # the coincident pair: zero distance, zero gradient from that pair - x[0,2]'s own nearest is y[0,4]
        x = torch.from_numpy(c["x"]).double().requires_grad_(True)
        SR.pair_dist(x, torch.from_numpy(c["y"]).double())[0, 2, 4].backward()
        assert torch.count_nonzero(x.grad) == 0


def test_fixture_gaps_meet_the_conditions():
    f = TR.load_fixture("set_losses.npz")
    assert float(f["gap_bar"]) == 1e-5
    for c in standalone_cases():
        g = SR.gaps(c["x"], c["y"])
        assert np.array_equal(g, c["gaps"])                                 # recorded = recomputed
        assert (g >= 1e-5).all(), g
        w32, w64 = SR.winners(c["x"], c["y"]), SR.winners(c["x"].astype(np.float64), c["y"].astype(np.float64))
        assert all(np.array_equal(a, b) for a, b in zip(w32, w64))
    t = TR.load_fixture("train_losses_rope.npz")
    assert float(t["gap_bar"]) == 1e-4 and t["step_gaps"].shape == (int(t["n_future"]), 4)
    assert (t["step_gaps"] >= 1e-4).all(), t["step_gaps"]
    assert np.array_equal(t["gaps"], t["step_gaps"].min(0))
    assert fixture_losses(t) == [("mse", 1.0), ("chamfer", 0.5), ("hausdorff", 0.25)] and int(t["n_future"]) == 3


def test_restatement_matches_reference_training_chain():
    f = TR.load_fixture("train_losses_rope.npz")
    loss, terms, preds, g, dstate = SR.restated_chain(f, fixture_losses(f))
    assert abs(loss - float(f["loss_sum"])) <= 1e-5 * abs(float(f["loss_sum"]))
    assert abs(loss - float(f["loss_sum_64"])) <= 1e-12 * abs(loss)
    assert (np.abs(terms - f["loss_terms"]) <= 1e-5 * np.abs(f["loss_terms"])).all(), (terms, f["loss_terms"])
    fut = f["state_future"].astype(np.float64)
    for fi, p in enumerate(preds):                                          # the recorded gaps are those of the chain itself
        assert np.allclose(SR.gaps(p.numpy(), fut[:, fi]), f["step_gaps"][fi], rtol=0, atol=1e-9)
    for k in TR.KEYS:
        err = np.abs(g[k] - f["g::" + k]).max()
        assert err <= grad_tol(f, k), (k, err, np.abs(f["g::" + k]).max())
    assert np.abs(dstate - f["dstate0"]).max() <= 1e-4 * np.abs(f["dstate0"]).max() + 1e-7
    assert np.abs(dstate - f["dstate0_64"]).max() <= 1e-10 * np.abs(f["dstate0_64"]).max()


# ------------------------------------------------------------------------------------------------ LossSpec: host only
def test_loss_spec_parses_names_and_modules():
    from adaptigraph_amd.set_losses import LossSpec, ChamferLoss, HausdorffLoss
    s = LossSpec([(torch.nn.MSELoss(), 1), (ChamferLoss(), 0.5), ("Hausdorff", 0.25)])
    assert s.names == ["mse", "chamfer", "hausdorff"] and s.kinds == [0, 1, 2] and s.weights == [1.0, 0.5, 0.25]
    assert not s.default and s.has_hausdorff and s.n_terms == 3
    d = LossSpec(None)
    assert d.default and d.names == ["mse"] and d.weights == [1.0] and not d.has_hausdorff
    c = s.c_struct()
    assert c.n_terms == 3 and list(c.kind)[:3] == [0, 1, 2] and list(c.weight)[:3] == [1.0, 0.5, 0.25]


def test_loss_spec_argument_errors():
    from adaptigraph_amd.set_losses import LossSpec
    with pytest.raises(ValueError, match="5 loss terms"):
        LossSpec([("mse", 1)] * 5)
    with pytest.raises(ValueError, match="0 loss terms"):
        LossSpec([])
    with pytest.raises(ValueError, match="weight"):
        LossSpec([("mse", 1), ("chamfer", float("nan"))])
    with pytest.raises(ValueError, match="weight"):
        LossSpec([("chamfer", float("inf"))])
    with pytest.raises(ValueError, match="unknown loss term"):
        LossSpec([("huber", 1)])
    with pytest.raises(ValueError, match="unknown loss term"):
        LossSpec([(torch.nn.L1Loss(), 1)])

    class EarthMoverLoss(torch.nn.Module):                                  # the reference's class is recognised by its name
        pass
    for term in ("emd", EarthMoverLoss()):
        with pytest.raises(NotImplementedError, match="host step"):
            LossSpec([("mse", 1), (term, 1)])


def test_hausdorff_is_refused_with_parts():
    from adaptigraph_amd.set_losses import LossSpec
    s = LossSpec([("mse", 1), ("hausdorff", 0.25)])
    for what in ("accumulate", "step_parts"):
        with pytest.raises(ValueError, match="Hausdorff"):
            s.forbid_parts(what)
    LossSpec([("mse", 1), ("chamfer", 0.5)]).forbid_parts("accumulate")     # means split: nothing raised
    LossSpec(None).forbid_parts("step_parts")


# ------------------------------------------------------------------------------------------------ the boundary
def test_set_loss_exports_are_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read(), flags=re.S)
    from adaptigraph_amd import _lib
    for name in EXPORTS:
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in _lib.EXPORTS
    assert re.search(r"typedef struct ag_loss_spec \{\s*int32_t n_terms;\s*int32_t kind\[4\];\s*float weight\[4\];\s*\} ag_loss_spec;", src)
    for macro, val in (("AG_LOSS_MSE", 0), ("AG_LOSS_CHAMFER", 1), ("AG_LOSS_HAUSDORFF", 2)):
        assert re.search(r"#define %s %d\b" % (macro, val), src) and getattr(_lib, macro) == val
    assert re.search(r"#define AG_ABI_VERSION 7\b", src)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    lib = _lib.load()                                                       # loads without a GPU
    for name in EXPORTS:
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert hasattr(lib, name)
    import ctypes as C
    assert C.sizeof(_lib.AgLossSpec) == 36
