"""CPU checks of the device-resident physics-parameter fit: the two exports at the boundary, the Python names, and the host
restatement of the device kernel's Adam / best-so-far update against the loop body of optimize_grad."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["ag_ppm_grad_step", "ag_ppm_adam_step"]


@pytest.mark.parametrize("name", NEW_EXPORTS)
def test_ppm_fit_exports_are_declared_and_exported(name):
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


def test_header_keeps_the_abi_version_and_lists_the_calls_as_never_waiting():
    hdr = open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()
    assert re.search(r"#define AG_ABI_VERSION 7\b", hdr)
    table = hdr[hdr.index("WHICH ENTRY POINTS BLOCK THE HOST"):hdr.index("#ifndef ADAPTIGRAPH_AMD_H")]
    row = [ln for ln in table.splitlines() if "ag_ppm_grad_step" in ln]
    assert len(row) == 1 and all(n in row[0] for n in NEW_EXPORTS) and "NEVER" in row[0]


def test_python_names_import():
    import adaptigraph_amd as ag
    from adaptigraph_amd import physics_param_optimizer as PPO
    for name in ("PhysParamFit", "optimize_grad_device", "dynamics_error_grad_device"):
        assert getattr(ag, name) is getattr(PPO, name) and name in ag.__all__


def test_fit_on_a_cpu_device_raises():
    import types
    import torch
    import adaptigraph_amd as ag
    task = dict(max_nobj=4, push_length=0.1, n_his=4)
    ppm = types.SimpleNamespace(task_config=task, device=torch.device("cpu"), material_dims={"rope": 1}, eef_num=1,
                                physics_param={"rope": torch.tensor([0.5])}, model=None)
    clouds = [np.zeros((3, 3), np.float32)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.PhysParamFit(ppm, [np.float32([0, 0, 0, 1])], clouds, clouds, n_starts=2)


def test_adam_best_update_restates_the_loop_body_of_optimize_grad():
    """The loop body of optimize_grad (physics_param_optimizer.py), copied here, against adam_best_update on random gradients."""
    from adaptigraph_amd.physics_param_optimizer import adam_best_update, PARAM_BOUNDS, _starting_points
    rng = np.random.default_rng(3)
    K, lr, iterations = 8, 0.05, 40
    x = _starting_points([0.5], K)
    grads_all = rng.normal(0, 1, (iterations, K, 1)) * 10.0 ** rng.integers(-6, 1, (iterations, K, 1))
    errs_all = rng.random((iterations, K))
    errs_all[5] = errs_all[5, 0]                                    # a tie: the first minimum wins
    # optimize_grad's loop
    m, v = np.zeros_like(x), np.zeros_like(x)
    best_x, best_err, best_k = None, np.inf, 0
    xs = []
    for it in range(iterations):
        xe = x.astype(np.float32)
        xs.append(xe)
        errors, grads = errs_all[it], grads_all[it]
        k = int(np.argmin(errors))
        if errors[k] < best_err:
            best_x, best_err, best_k = xe[k].copy(), errors[k], k
        m = 0.9 * m + 0.1 * grads
        v = 0.999 * v + 0.001 * grads * grads
        step = lr * (m / (1 - 0.9 ** (it + 1))) / (np.sqrt(v / (1 - 0.999 ** (it + 1))) + 1e-8)
        x = np.clip(xe.astype(np.float64) - step, *PARAM_BOUNDS)
    # the helper
    x2 = _starting_points([0.5], K).astype(np.float32)
    m2, v2, best = np.zeros((K, 1)), np.zeros((K, 1)), (None, np.inf, 0)
    for it in range(iterations):
        assert np.array_equal(x2, xs[it]), it
        x2, m2, v2, best = adam_best_update(x2, errs_all[it], grads_all[it], m2, v2, it, lr, best)
    assert np.array_equal(x2, x.astype(np.float32)) and np.array_equal(m2, m) and np.array_equal(v2, v)
    assert np.array_equal(best[0], best_x) and best[1] == best_err and best[2] == best_k
    assert x2.min() >= np.float32(PARAM_BOUNDS[0]) and x2.max() <= np.float32(PARAM_BOUNDS[1])
