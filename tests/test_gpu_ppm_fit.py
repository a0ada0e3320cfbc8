"""GPU checks of the device-resident physics-parameter fit (-m gpu): ag_ppm_grad_step / ag_ppm_adam_step behind
dynamics_error_grad_device, PhysParamFit and optimize_grad_device, against the reference's own autograd through its own
dynamics_masked (tests/golden/ppm_grad_*.npz), the autograd path of this package in the same process, and optimize_grad.
Every test prints the figures it asserts on."""
import time

import numpy as np
import pytest
import torch

import ppm_grad_support as S
import train_restate as TR
from test_gpu_parity import POS_TOL
from test_gpu_train import _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ag():
    import adaptigraph_amd
    return adaptigraph_amd


def _problem(f, material, dev, **task_over):
    """the fixture as the lists dynamics_error_grad takes: (ppm, inits, reals, acts)"""
    task = dict(S.task_of(f), max_nobj=f["state_init"].shape[1], **task_over)
    ppm = S.ppm_of(task, material)
    ppm.model = _model(dev, TR.make_weights(int(f["w_seed"]), n_his=int(task["n_his"])), pstep=int(f["pstep"]), material=material)
    ppm.device = dev
    counts, rcounts = f["state_mask"].sum(1), f["real_mask"].sum(1)
    for b in range(len(counts)):                                  # the lists hold prefixes: the fixture's masks must be prefixes
        assert f["state_mask"][b, :counts[b]].all() and f["real_mask"][b, :rcounts[b]].all()
    assert rcounts.max() <= task["max_nobj"]
    inits = [f["state_init"][b, :counts[b]] for b in range(len(counts))]
    reals = [f["state_real"][b, :rcounts[b]] for b in range(len(counts))]
    acts = [f["action"][b] for b in range(len(counts))]
    return ppm, inits, reals, acts


def _within(label, got, ref64, ref32):
    err, lim = float(np.abs(np.asarray(got, np.float64) - ref64).max()), S.bar(ref64, ref32)
    print(f"{label}: error {err:.3e}  reference fp32 error {np.abs(np.asarray(ref32, np.float64) - ref64).max():.3e}  "
          f"max|ref| {np.abs(ref64).max():.3e}  bar {lim:.3e}")
    assert err <= lim, (label, err, lim)


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("material", S.MATERIALS)
def test_device_gradient_vs_reference(ag, dev, material, layout):
    f = S.load(material)
    k = layout + "::"
    ppm, inits, reals, acts = _problem(f, material, dev)
    out = {}
    err, grad = ag.dynamics_error_grad_device(f[k + "phys"], ppm, inits, reals, acts, _out=out)
    e_seq = np.abs(out["state_seqs"].cpu().numpy() - f[k + "state_seqs"]).max()
    e_ch = np.abs(out["chamfer"].cpu().numpy() - f[k + "chamfer"]).max()
    print(f"{material} {layout}: state_seqs error {e_seq:.2e} (bar {POS_TOL:.0e}), chamfer error {e_ch:.2e} (bar 2e-05)")
    assert e_seq <= POS_TOL
    assert e_ch <= 2e-5
    assert grad.dtype == np.float64 and grad.shape == f[k + "dphys_64"].shape
    assert abs(err - out["chamfer"].cpu().numpy().astype(np.float64).mean()) == 0
    _within(f"{material} {layout} dphys", grad, f[k + "dphys_64"], f[k + "dphys"])


# ------------------------------------------------------------------------------------------------ 2. against the existing path
@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("material", S.MATERIALS)
def test_device_path_agrees_with_the_autograd_path(ag, dev, material, layout):
    f = S.load(material)
    k = layout + "::"
    ppm, inits, reals, acts = _problem(f, material, dev)
    e_h, g_h = ag.dynamics_error_grad(f[k + "phys"], ppm, inits, reals, acts)
    e_d, g_d = ag.dynamics_error_grad_device(f[k + "phys"], ppm, inits, reals, acts)
    assert g_h.shape == g_d.shape and g_d.dtype == np.float64
    print(f"{material} {layout}: |error_device - error_host| {abs(e_d - e_h):.3e}, max|grad_device - grad_host| "
          f"{np.abs(g_d - g_h).max():.3e}, max|grad_host| {np.abs(g_h).max():.3e}")
    ch64 = float(np.float64(f[k + "chamfer"]).mean())
    assert abs(e_d - ch64) <= 2e-5 and abs(e_h - ch64) <= 2e-5
    _within(f"{material} {layout} device dphys", g_d, f[k + "dphys_64"], f[k + "dphys"])
    _within(f"{material} {layout} host dphys", g_h, f[k + "dphys_64"], f[k + "dphys"])


# ------------------------------------------------------------------------------------------------ 3. row independence
def test_a_start_inside_the_batch_carries_the_bits_of_the_start_alone(ag, dev):
    from adaptigraph_amd import physics_param_optimizer as PPO
    f = S.load("rope")
    ppm, inits, reals, acts = _problem(f, "rope", dev)
    starts = PPO._starting_points([0.5], 8)

    def one_step(x):
        fit = ag.PhysParamFit(ppm, acts, inits, reals, starts=x, iterations=2)
        fit.step()
        _, _, _, res = fit.result(return_res=True)
        return res["errors"][0], fit.last_grad.cpu().numpy(), fit.x.cpu().numpy()

    e8, g8, x8 = one_step(starts)
    e8b, g8b, x8b = one_step(starts)
    assert np.array_equal(e8, e8b) and np.array_equal(g8, g8b) and np.array_equal(x8, x8b)     # two calls: the same bits
    assert np.abs(g8).max() > 0 and np.isfinite(g8).all()
    for k in range(8):
        e1, g1, x1 = one_step(starts[k:k + 1])
        print(f"start {k}: error {e8[k]!r} / alone {e1[0]!r}, gradient {g8[k]!r} / alone {g1[0]!r}")
        assert e1[0] == e8[k] and g1[0] == g8[k] and x1[0] == x8[k], k
    # the same objective as the one-call function evaluates
    e, g = ag.dynamics_error_grad_device([float(np.float32(starts[3, 0]))], ppm, inits, reals, acts)
    assert abs(e - e8[3]) <= 1e-7 and abs(g[0] - g8[3]) <= 1e-5 * abs(g8[3]) + 1e-9


# ------------------------------------------------------------------------------------------------ 4. it does not wait
def test_steps_return_while_the_stream_is_busy(ag, dev):
    f = S.load("rope")
    ppm, inits, reals, acts = _problem(f, "rope", dev)
    fit = ag.PhysParamFit(ppm, acts, inits, reals, n_starts=8, iterations=16)
    for _ in range(3):
        fit.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit.step()
    T = time.perf_counter() - t0                                   # host time of an enqueue on an idle stream
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    ms_per_cycle = e0.elapsed_time(e1) / 10_000_000
    n_steps = 3
    want_ms = max(100.0, 4e3 * T * n_steps)
    done = torch.cuda.Event()
    torch.cuda._sleep(int(want_ms / ms_per_cycle))
    done.record()
    for _ in range(n_steps):
        fit.step()
    still_busy = not done.query()
    torch.cuda.synchronize()
    print(f"host time of a step {T * 1e3:.2f} ms, spin {want_ms:.0f} ms, {n_steps} steps enqueued behind it")
    assert still_busy, "PhysParamFit.step waited for the GPU"
    _, _, _, res = fit.result(return_res=True)
    assert res["errors"].shape == (7, 8) and np.isfinite(res["errors"]).all()


# ------------------------------------------------------------------------------------------------ 5. overflow
def test_overflowing_step_is_skipped_and_reported(ag, dev):
    f = S.load("rope")
    ppm, inits, reals, acts = _problem(f, "rope", dev, max_nR=200)
    big = int(S.task_of(f)["max_nR"])
    with pytest.raises(Exception, match="Exceeds max dims"):
        ag.dynamics_error_grad_device([0.5], ppm, inits, reals, acts)
    fit = ag.PhysParamFit(ppm, acts, inits, reals, n_starts=4, iterations=4)
    state = lambda: [t.clone() for t in (fit.x, fit.phys, fit.exp_avg, fit.exp_avg_sq, fit.hist_x, fit.hist_err, fit.best)]   # noqa: E731
    before = state()
    fit.step()                                                      # returns: the guard presents the offending graphs as empty
    fit.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, state()))
    with pytest.raises(Exception, match="Exceeds max dims"):
        fit.result()
    assert fit._step == 0 and fit._updates == 0 and all(torch.equal(a, b) for a, b in zip(before, state()))
    fit.max_nR = big
    fit.step()
    fit.evaluate()
    best, err, init_err, res = fit.result(return_res=True)
    assert res["errors"].shape == (2, 4) and not torch.equal(fit.x, before[0])
    ppm2, *_ = _problem(f, "rope", dev)
    fresh = ag.PhysParamFit(ppm2, acts, inits, reals, n_starts=4, iterations=4)
    fresh.step()
    fresh.evaluate()
    best2, err2, init2, res2 = fresh.result(return_res=True)
    assert np.array_equal(res["errors"], res2["errors"]) and np.array_equal(res["params"], res2["params"])
    assert np.array_equal(best, best2) and err == err2 and init_err == init2


def test_an_evaluation_between_two_steps_changes_neither_of_them(ag, dev):
    """step(); evaluate(); step() walks the parameters of step(); step(): evaluate() takes a history row, but it neither counts
    as an Adam update (bias corrections) nor overwrites the gradient of the last step."""
    f = S.load("rope")
    ppm, inits, reals, acts = _problem(f, "rope", dev)
    a = ag.PhysParamFit(ppm, acts, inits, reals, n_starts=2, iterations=4)
    b = ag.PhysParamFit(ppm, acts, inits, reals, n_starts=2, iterations=4)
    a.step()
    a.step()
    b.step()
    g1 = b.last_grad.clone()
    b.evaluate()
    assert torch.equal(b.last_grad, g1) and g1.abs().max() > 0
    b.step()
    assert torch.equal(a.x, b.x) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    _, _, _, ra = a.result(return_res=True)
    _, _, _, rb = b.result(return_res=True)
    assert ra["errors"].shape == (2, 2) and rb["errors"].shape == (3, 2)
    assert np.array_equal(rb["errors"][0], ra["errors"][0])
    assert np.array_equal(rb["errors"][1], ra["errors"][1]) and np.array_equal(rb["errors"][2], ra["errors"][1])


# ------------------------------------------------------------------------------------------------ 6. the planted problem
def test_optimize_grad_device_on_the_planted_problem(ag, dev):
    material, p_star = "granular", 0.83
    f = S.load(material)
    ppm, inits, _, acts = _problem(f, material, dev)
    counts = f["state_mask"].sum(1)
    seen = ag.dynamics_masked(torch.from_numpy(f["state_init"]).to(dev), torch.from_numpy(f["state_mask"]).to(dev),
                              torch.from_numpy(f["action"]), ppm.model, dev, ppm, physics_param={material: torch.tensor([p_star])})
    reals = [seen["state_seqs"][b, :counts[b]].cpu().numpy() for b in range(len(counts))]
    best, err, init_err, res = ag.optimize_grad_device(ppm, acts, inits, None, reals, iterations=30, n_starts=8, return_res=True)
    hb, herr, hinit, hres = ag.optimize_grad(ppm, acts, inits, None, reals, iterations=30, n_starts=8, return_res=True)
    grid = np.linspace(-0.2, 1.2, 57)
    sweep = ag.dynamics_error_sweep([[v] for v in grid], ppm, inits, reals, acts)
    d_start = np.abs(res["errors"][0] - hres["errors"][0]).max()
    print(f"optimize_grad_device: p* {p_star} found {best} error {err:.3e} init_error {init_err:.3e}; optimize_grad found {hb} "
          f"error {herr:.3e}; sweep minimum {sweep.min():.3e} at {grid[sweep.argmin()]:.3f}; start errors differ by {d_start:.3e}; "
          f"largest difference between the two parameter trajectories {np.abs(res['params'] - hres['params']).max():.3e}")
    assert best.shape == (1,) and best.dtype == np.float32 and -0.2 <= best[0] <= 1.2
    assert res["params"].shape == (31, 8, 1) and res["errors"].shape == (31, 8) and 0 <= res["best_start"] < 8
    assert np.all(err <= res["errors"][0])
    assert err < init_err
    assert err <= sweep.min()
    assert d_start <= 2e-5
    assert init_err == res["errors"][0, 0] and err == res["errors"].min()
