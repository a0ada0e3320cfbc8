"""CPU checks of the physics-parameter gradient path: the ppm_grad_*.npz fixtures are self-consistent, a float64 torch
restatement (tests/ppm_grad_support.py on tests/train_restate.py) reproduces the reference's gradients on the fixture's edges,
and the new entry points exist and refuse a CPU device."""
import os
import re

import numpy as np
import pytest
import torch

import ppm_grad_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("material", S.MATERIALS)
def test_fixture_is_self_consistent(material):
    f = S.load(material)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"ppm_grad_{material}.npz")) < (1 << 20)
    B, N_o, _ = f["state_init"].shape
    repeat = f["action"][:, 3].astype(np.int64)
    assert repeat.min() >= 2 and repeat.max() <= 4 and len(set(repeat.tolist())) == B
    for layout, pshape in zip(S.LAYOUTS, [(1,), (B, 1), (B, N_o)]):
        k = layout + "::"
        assert f[k + "phys"].shape == pshape == f[k + "dphys"].shape == f[k + "dphys_64"].shape
        assert f[k + "dstate_init"].shape == (B, N_o, 3)
        assert int(f[k + "n_steps"]) == repeat.max()
        assert list(f[k + "row_steps"]) == ([repeat.max()] * B if layout == "shared" else list(repeat))
        assert abs(float(f[k + "loss"]) - f[k + "chamfer"].astype(np.float64).mean()) < 1e-6
        assert abs(float(f[k + "loss_64"]) - f[k + "chamfer_64"].mean()) < 1e-12
        assert np.abs(f[k + "state_seqs"] - f[k + "state_seqs_64"]).max() < 1e-5
        for i in range(int(f[k + "n_steps"])):
            for b, (r, s) in enumerate(S.step_edges(f, k, i)):
                assert (len(r) > 0) == (i < f[k + "row_steps"][b]) and np.all(np.diff(r) >= 0) and len(r) == len(s)
        # a gradient that rounding decides would pin nothing
        assert np.abs(f[k + "dphys_64"]).max() > 10 * np.abs(f[k + "dphys"] - f[k + "dphys_64"]).max()
    assert np.abs(f["fwd::daction_64"]).max() > 0 and np.abs(f["fwd::dphys_64"]).max() > 0


@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("material", S.MATERIALS)
def test_float64_restatement_reproduces_reference_gradients(material, layout):
    f = S.load(material)
    loss, ch, seqs, p, state = S.restated_loss(f, material, layout)
    loss.backward()
    k = layout + "::"
    assert np.abs(seqs.detach().numpy() - f[k + "state_seqs_64"]).max() < 1e-9
    assert abs(loss.item() - float(f[k + "loss_64"])) < 1e-9
    for name, got in (("dphys", p.grad.numpy()), ("dstate_init", state.grad.numpy())):
        err = np.abs(got - f[k + name + "_64"]).max()
        print(f"{material} {layout} {name}: restated float64 error {err:.2e}, reference fp32 error "
              f"{np.abs(f[k + name] - f[k + name + '_64']).max():.2e}, bar {S.bar(f[k + name + '_64'], f[k + name]):.2e}")
        assert err <= S.bar(f[k + name + "_64"], f[k + name])


def test_exports_and_entry_points_exist():
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read(), flags=re.S)
    for name in ("ag_backward_inputs", "ag_cost_chamfer_backward"):
        assert re.search(rf"\bint {name}\s*\(", src) and name in _lib.EXPORTS
    for name in ("dynamics_masked_diff", "chamfer_diff", "dynamics_error_grad", "optimize_grad"):
        assert callable(getattr(ag, name)) and name in ag.__all__
    assert callable(ag.DynamicsPredictor.forward_diff)


def test_cpu_device_is_refused():
    import adaptigraph_amd as ag
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    f = S.load("rope")
    ppm = S.ppm_of(S.task_of(f), "rope")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.dynamics_masked_diff(torch.from_numpy(f["state_init"]), torch.from_numpy(f["state_mask"]), torch.from_numpy(f["action"]),
                                None, torch.device("cpu"), ppm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.chamfer_diff(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
