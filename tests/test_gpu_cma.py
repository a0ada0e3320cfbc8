"""CMA-ES on the device (csrc/ag_cma.hip, adaptigraph_amd.CmaSearch, Planner(planner_type='CMA')) against the numpy restatement
tests/cma_restate.py: teacher-forced state parity within CMA_STATE_TOL (derived in cma_restate.py), the tie / NaN / skip rules,
run-to-run determinism, free-running convergence, no host waits, and the planner type on closed-form callables and on the
engine's own rollout and cost."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cma_restate as R

pytestmark = pytest.mark.gpu
ALL_FIELDS = R.STATE_FIELDS + ("A_inv",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ag():
    import adaptigraph_amd
    return adaptigraph_amd


def _assert_state(search, restate, what):
    got, want = search.state(), restate.fields()
    for k in ALL_FIELDS:
        d = R.deviation(got[k], want[k])
        print(f"{what} {k}: {d:.3g}")
        assert d <= R.CMA_STATE_TOL, (what, k, d)
    assert got["g"] == restate.g and got["status"] == restate.status, (what, got["g"], got["status"])
    assert got["best_generation"] == restate.best_generation and got["best_value"] == restate.best_value
    assert np.allclose(got["best_x"], restate.best_x, rtol=3e-7, atol=1e-7)       # fp32 phenotypes: equal up to their last bit
    return got


@pytest.mark.parametrize("n,popsize,generations,corner", R.GPU_CASES)
def test_teacher_forced_state_parity(ag, dev, n, popsize, generations, corner):
    """Per generation: device ask(draws); closed-form fitness in fp64 on the host from the DEVICE's phenotypes, cast to fp32; device
    tell; the restatement asks with the same draws and is told the same values."""
    kw, draws, f = R.case(n, popsize, generations, corner=corner)
    search = ag.CmaSearch(device=dev, **kw)
    restate = R.Restate(**kw)
    span = (restate.hi - restate.lo)[None, :]
    for g in range(generations):
        x = search.ask(draws[g]).cpu().numpy()
        want = restate.ask(draws[g])
        if corner and g == 0:
            assert R.moved_fraction(restate) >= 0.25
        ulp = np.spacing(np.maximum(np.abs(want), span).astype(np.float32))
        assert x.dtype == np.float32 and np.all(np.abs(x.astype(np.float64) - want.astype(np.float64)) <= ulp), g
        assert np.all(x >= restate.lo.astype(np.float32)[None, :]) and np.all(x <= restate.hi.astype(np.float32)[None, :])
        v = f(x.astype(np.float64)).astype(np.float32)
        search.tell(torch.from_numpy(v).to(dev))
        restate.tell(v)
        assert np.array_equal(search.order.cpu().numpy(), restate.order), g
        assert bool(search.improved.item()) == restate.improved, g
        _assert_state(search, restate, f"({n},{popsize}) g={g}")
    assert search.state()["g"] == generations


def test_ties_nan_skip_and_infinity(ag, dev):
    nan, inf = float("nan"), float("inf")
    kw, draws, _ = R.case(3, 8, 6, seed=3)
    search, restate = ag.CmaSearch(device=dev, **kw), R.Restate(**kw)

    def both(g, values, ask=True):
        v = np.asarray(values, np.float32)
        if ask:
            search.ask(draws[g])
            restate.ask(draws[g])
        search.tell(torch.from_numpy(v).to(dev))
        restate.tell(v)
        assert np.array_equal(search.order.cpu().numpy(), restate.order), values
        return search.order.cpu().numpy().tolist()

    assert both(0, [2.5] * 8) == list(range(8))                                   # all equal: by index
    _assert_state(search, restate, "equal")
    assert both(1, [0, 1, 2, 3, 3, 3, 5, 6]) == list(range(8))                   # duplicates straddling rank mu = 4
    assert both(2, [6, 3, 5, 3, 0, 3, 1, 2])[:6] == [4, 6, 7, 1, 3, 5]
    _assert_state(search, restate, "duplicates")
    assert both(3, [4, nan, 2, 1, 0, 7, 6, 5])[-1] == 1                          # one NaN: last
    got = _assert_state(search, restate, "one NaN")
    assert got["status"] == 0 and got["g"] == 4
    # popsize - mu + 1 NaNs: bit 0, the state bit for bit, g unchanged
    before = search._state.clone()
    order = both(4, [nan, 1, nan, nan, 0, nan, 2, nan])
    assert order == [4, 1, 6, 0, 2, 3, 5, 7]
    after = search._state.clone()
    assert after[5].item() == 1.0 and not bool(search.improved.item())
    after[5] = before[5]
    assert torch.equal(after.view(torch.int64), before.view(torch.int64))
    # a clean tell of the same population afterwards matches the restatement; an infinity is ordered, not skipped
    assert both(4, [inf, 1, -inf, 3, 0, 4, 2, 5], ask=False)[:2] == [2, 4] and search.order[-1].item() == 0
    got = _assert_state(search, restate, "after the skip")
    assert got["g"] == 5 and got["status"] == 1 and got["best_value"] == -inf
    with pytest.raises(RuntimeError, match="bit 0"):
        search.result()
    best_value, best_x, mean_x, sigma, g, status = search.result()                # raised once, cleared
    assert status == 0 and g == 5 and best_value == -inf and sigma == pytest.approx(restate.sigma, rel=1e-9)
    assert np.allclose(mean_x, restate.phenotype(restate.m), rtol=3e-7, atol=1e-7)
    # maximising ranks the negated values
    kw["popsize"] = 8
    smax, rmax = ag.CmaSearch(device=dev, maximize=True, **kw), R.Restate(maximize=True, **kw)
    v = np.float32([1, 5, nan, 5, -inf, inf, 0, 2])
    smax.ask(draws[5])
    rmax.ask(draws[5])
    smax.tell(torch.from_numpy(v).to(dev))
    rmax.tell(v)
    assert smax.order.cpu().numpy().tolist() == rmax.order.tolist() == [5, 1, 3, 7, 0, 6, 4, 2]
    _assert_state(smax, rmax, "maximise")


def _device_fitness(f_terms, x):
    c, t = f_terms
    return ((x.double() - t) ** 2 * c).sum(dim=1).float()


def test_same_inputs_give_the_same_bits(ag, dev):
    kw, draws, _ = R.case(12, 70, 4, corner=True)
    _, c, t, _, _ = R.ellipsoid(12)
    terms = (torch.from_numpy(c).to(dev), torch.from_numpy(t).to(dev))
    states = []
    for _ in range(2):
        s = ag.CmaSearch(device=dev, **kw)
        for g in range(4):
            s.tell(_device_fitness(terms, s.ask(draws[g])))
        states.append(s._state.clone())
        assert s.waits == 0
    assert torch.equal(states[0].view(torch.int64), states[1].view(torch.int64))
    assert states[0][4].item() == 4.0 and states[0][5].item() == 0.0


def test_free_running_convergence_and_no_waits(ag, dev):
    """n = 12 ellipsoid, 120 generations, fitness by torch on the device, the same draws on both sides.  The device's
    f(mean_G) / f(mean_0) must reach the square root of the restatement's ratio (half the orders of magnitude): an fp32 sum order
    may flip a near-tie in rank, so equality is not asked for."""
    G = 120
    kw, draws, f = R.case(12, 11, G)
    _, c, t, _, _ = R.ellipsoid(12)
    terms = (torch.from_numpy(c).to(dev), torch.from_numpy(t).to(dev))
    search, restate = ag.CmaSearch(device=dev, **kw), R.Restate(**kw)
    start = float(f(restate.phenotype(restate.m)))
    zs = torch.from_numpy(draws).to(dev)
    for g in range(G):
        search.tell(_device_fitness(terms, search.ask(zs[g])))
        restate.tell(f(restate.ask(draws[g]).astype(np.float64)).astype(np.float32))
    assert search.waits == 0
    best_value, best_x, mean_x, sigma, gens, status = search.result()
    assert search.waits == 1 and gens == G and status == 0
    want = float(f(restate.phenotype(restate.m))) / start
    got = float(f(mean_x.astype(np.float64))) / start
    print(f"f(mean_G) / f(mean_0): device {got:.3g}, restatement {want:.3g}")
    assert want < 1e-2 and got <= want ** 0.5
    assert best_value == pytest.approx(float(f(best_x.astype(np.float64))), rel=1e-5)


def test_limits_raise_before_anything_is_enqueued(ag, dev):
    with pytest.raises(NotImplementedError):
        ag.CmaSearch(np.zeros(65), 0.3, -1.0, 1.0, device=dev)
    with pytest.raises(NotImplementedError):
        ag.CmaSearch(np.zeros(4), 0.3, -1.0, 1.0, popsize=3, device=dev)
    from adaptigraph_amd import _lib
    lib = _lib.load_cma()
    assert lib.ag_cma_state_doubles(65, 8) == -4 and lib.ag_cma_state_doubles(4, 32769) == -4
    assert lib.ag_cma_state_doubles(4, 8) == 24 + 3 * 16 + 8 * 4 + 4
    flags = (ctypes.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    state = torch.zeros(lib.ag_cma_state_doubles(4, 8), dtype=torch.float64, device=dev)
    rc = lib.ag_cma_init(0, None, 65, 8, flags, 0.3, flags, flags, flags, None, 6.28, 0, ctypes.c_void_p(state.data_ptr()))
    assert rc == _lib.AG_ERR_UNSUPPORTED and b"65" in lib.ag_cma_last_error()
    rc = lib.ag_cma_init(0, None, 4, 8, flags, 0.3, flags, flags, flags, None, 6.28, 0, ctypes.c_void_p(state.data_ptr()))
    assert rc == _lib.AG_ERR_INVALID and not bool(state.any())                     # scale 0, lo == hi: nothing was written
    s = ag.CmaSearch(np.zeros(4), 0.3, -1.0, 1.0, popsize=20000, device=dev)      # the shipped n_sample is served
    x = s.ask()
    s.tell(-(x ** 2).sum(dim=1))
    assert s.result()[4] == 1


# ------------------------------------------------------------------------------------------------------------- planner
def _closed_form_config(dev, kind, seen, **kw):
    lo = torch.tensor([-1.0, -2.0, -3.14, 2.0], device=dev)
    hi = torch.tensor([1.0, 2.0, 3.14, 4.0], device=dev)
    target = torch.tensor([[0.3, -1.2, 2.9, 3.1], [-0.6, 0.4, -3.0, 2.5]], device=dev)

    def rollout(state_cur, act_seqs):
        return {"state_seqs": act_seqs[:, :, None, :3] + state_cur[None, None, :, :]}

    def cost(state_seqs, act_seqs, state_cur=None, weights=None):
        d = act_seqs - target[None]
        d[..., 2] = torch.remainder(d[..., 2] + torch.pi, 2 * torch.pi) - torch.pi
        sq = (d * d).reshape(d.shape[0], -1)
        reward = -sq[:, 0]
        for k in range(1, sq.shape[1]):                          # one fixed order: a row's reward does not depend on its batch
            reward = reward - sq[:, k]
        seen.append(reward)
        return {"reward_seqs": reward}

    cfg = {"action_dim": 4, "model_rollout_fn": rollout, "evaluate_traj_fn": cost, "n_sample": 64, "n_look_ahead": 2,
           "n_update_iter": 4, "reward_weight": 10.0, "action_lower_lim": lo, "action_upper_lim": hi, "planner_type": kind,
           "device": dev, "noise_level": 0.3}
    cfg.update(kw)
    return cfg, lo, hi


def test_planner_cma_on_closed_form_callables(ag, dev):
    state = torch.zeros((5, 3), device=dev)
    act0 = torch.tensor([[0.0, 0.0, 0.0, 3.0], [0.0, 0.0, 0.0, 3.0]], device=dev)
    seen = []
    cfg, lo, hi = _closed_form_config(dev, "MPPI", seen)
    keys = set(ag.Planner(cfg).trajectory_optimization(state, act0).keys())
    results = {}
    for reuse in (True, False):
        seen.clear()
        cfg, lo, hi = _closed_form_config(dev, "CMA", seen, reuse_best_rollout=reuse)
        planner = ag.Planner(cfg)
        torch.manual_seed(11)
        res = planner.trajectory_optimization(state, act0)
        assert set(res.keys()) == keys
        act = res["act_seq"]
        assert act.shape == (2, 4) and bool(((act >= lo) & (act <= hi)).all())
        generations = seen[:4]
        assert len(seen) == 5 and all(r.shape == (64,) for r in generations)       # four generations + the winner's evaluation
        assert res["best_eval_output"]["reward_seqs"].item() == torch.stack(generations).max().item()
        assert res["best_model_output"]["state_seqs"].shape == (1, 2, 5, 3)
        assert planner.last_cma.waits == 0 and planner.last_cma.result()[4] == 4
        first, last = generations[0].max().item(), generations[-1].max().item()
        print(f"best reward of generation 0: {first:.4g}, of generation 3: {last:.4g}")
        results[reuse] = act.clone()
    assert torch.equal(results[True], results[False])
    # two calls + merge_res: independent restarts
    seen.clear()
    res_all = [planner.trajectory_optimization(state, act0) for _ in range(2)]
    merged = planner.merge_res(res_all)
    scores = [r["best_eval_output"]["reward_seqs"].item() for r in res_all]
    assert merged["best_eval_output"]["reward_seqs"].item() == max(scores)
    assert torch.equal(merged["act_seq"], res_all[int(np.argmax(scores))]["act_seq"])


def test_planner_cma_on_the_engine(ag, dev):
    """The engine's dynamics + running_cost on the 100-particle rope of tests/test_gpu_more.py: n_sample 32, two look-ahead steps,
    three generations, one wait per call; a max_nR that is too small is raised by the call itself."""
    from oracle import adaptigraph_oracle as O
    from test_gpu_more import _task, _rope, _model
    from test_gpu_parity import _ppm
    rng = np.random.default_rng(21)
    cloud = _rope(100, rng)
    lo = torch.tensor([cloud[:, 0].min() - 0.3, cloud[:, 2].min() - 0.3, -3.14, 2.0], device=dev)
    hi = torch.tensor([cloud[:, 0].max() + 0.3, cloud[:, 2].max() + 0.3, 3.14, 4.0], device=dev)
    s0 = torch.from_numpy(cloud).to(dev)
    target = torch.from_numpy(cloud + np.float32([0.2, 0, 0.1])).to(dev)
    _, m = _model(ag, O, "rope", 21, dev)

    def planner_for(max_nR):
        task = _task("rope", max_nR=max_nR, action_lower_lim=lo.tolist(), action_upper_lim=hi.tolist())
        cfg = {"action_dim": 4, "model_rollout_fn": functools.partial(ag.dynamics, model=m, device=dev, ppm_optimizer=_ppm(task, "rope")),
               "evaluate_traj_fn": functools.partial(ag.running_cost, error_func=functools.partial(ag.chamfer, y=target[None]),
                                                     penalty_func=functools.partial(ag.rope_penalty, sim_real_ratio=10.0),
                                                     bbox=np.array([[-4.5, 0.0], [-2.5, 4.5]])),
               "n_sample": 32, "n_look_ahead": 2, "n_update_iter": 3, "reward_weight": 500.0, "action_lower_lim": lo,
               "action_upper_lim": hi, "planner_type": "CMA", "device": dev}
        return ag.Planner(cfg)

    planner = planner_for(6000)
    act0 = (0.5 * (lo + hi))[None].repeat(2, 1)
    assert planner._can_wait_once(s0) and not planner._can_pipeline(s0)
    torch.manual_seed(5)
    res = planner.trajectory_optimization(s0, act0)
    act = res["act_seq"]
    assert act.shape == (2, 4) and bool(torch.isfinite(act).all()) and bool(((act >= lo) & (act <= hi)).all())
    assert res["best_model_output"]["state_seqs"].shape == (1, 2, 100, 3)
    assert bool(torch.isfinite(res["best_model_output"]["state_seqs"]).all())
    assert bool(torch.isfinite(res["best_eval_output"]["reward_seqs"]).all())
    assert planner.last_cma.waits == 0 and planner.last_cma.result()[4] == 3
    with pytest.raises(Exception, match="Exceeds max dims"):
        planner_for(50).trajectory_optimization(s0, act0)
