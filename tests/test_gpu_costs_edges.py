"""The planner-side kernels (csrc/ag_cost.hip, csrc/ag_mppi.hip) at the shapes where their loops end: the 256-lane x 4-point
ownership of k_chamfer (1024), its clamped tail and even padding, the LDS limit, the 1024-wide single-workgroup trees of k_reward /
k_cloth_combine / k_mppi_update, the handed-in maxima - and on non-finite inputs, where they have to do what torch.min / max /
maximum do in the reference: propagate.

Yardstick: tests/costs_restate.py in float64 on the same fp32 inputs (pinned to the reference's recordings by
tests/test_costs_restate.py).  Bar, as in test_gpu_train.py: the kernel's largest error against float64 is at most 4x that of the
same restatement run in fp32 on the CPU, plus 1e-7 max|ref|, and never more than COST_TOL.  Every case prints both errors and
ratio = err / (err32 + 0.25e-7 max|ref|), the quantity the bar holds to 4 (DESIGN.md section 3.5 records the largest seen).
"""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import costs_restate as CR
from test_gpu_more import COST_TOL

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ag():
    import adaptigraph_amd
    return adaptigraph_amd


def state_stats(*a):
    from adaptigraph_amd.losses import state_stats as fn
    return fn(*a)


def _g(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(kernel, case, got, ref64, ref32, circular=None):
    """got: device result; ref64 / ref32: the restatement in float64 / fp32.  circular: boolean mask of angle entries."""
    got, ref64, ref32 = got.detach().cpu().to(F64), ref64.detach().to(F64), ref32.detach().to(F64)
    assert got.shape == ref64.shape and bool(torch.isfinite(ref64).all()) and bool(torch.isfinite(got).all()), (kernel, case)
    e, e32 = (got - ref64).abs(), (ref32 - ref64).abs()
    if circular is not None:
        e = torch.where(circular, CR.circular_diff(got, ref64), e)
        e32 = torch.where(circular, CR.circular_diff(ref32, ref64), e32)
    err, err32, scale = float(e.max()), float(e32.max()), float(ref64.abs().max())
    print(f"RATIO {kernel} {case}: err {err:.3e} fp32-restatement {err32:.3e} max|ref| {scale:.3e} "
          f"ratio {err / (err32 + 0.25e-7 * scale + 1e-300):.2f}")
    assert err <= min(4 * err32 + 1e-7 * scale, COST_TOL), (kernel, case, err, err32)


# ------------------------------------------------------------------------------------------------------------ chamfer forward
@pytest.mark.parametrize("mask_kind", CR.MASK_KINDS)
@pytest.mark.parametrize("By", [1, 3])
@pytest.mark.parametrize("N,M", CR.CHAMFER_SHAPES)
def test_chamfer_forward_at_loop_boundaries(ag, dev, N, M, By, mask_kind):
    x, y, xm, ym = CR.chamfer_case(N, M, By, mask_kind)
    got = ag.chamfer(_g(x, dev), _g(y, dev), _g(xm, dev), _g(ym, dev))
    _check("chamfer", f"N={N} M={M} By={By} mask={mask_kind}", got, CR.chamfer(x, y, xm, ym), CR.chamfer(x, y, xm, ym, F32))
    if mask_kind != "none":          # what sits in a masked-out slot is never looked at: 1e30 / NaN there change no bit
        zx, zy = np.where(xm[..., None], x, 0).astype(np.float32), np.where(ym[..., None], y, 0).astype(np.float32)
        zero = ag.chamfer(_g(zx, dev), _g(zy, dev), _g(xm, dev), _g(ym, dev))
        junk = ag.chamfer(_g(CR.with_garbage(x, xm), dev), _g(CR.with_garbage(y, ym), dev), _g(xm, dev), _g(ym, dev))
        assert torch.equal(_bits(zero), _bits(got)) and torch.equal(_bits(junk), _bits(got))


@pytest.mark.parametrize("N", [1, 3, 5, 255, 1023, 1025])
def test_chamfer_of_a_cloud_with_itself_is_exactly_zero(ag, dev, N):
    x = _g(CR.chamfer_case(N, N, 3, "none")[0], dev)
    assert torch.equal(ag.chamfer(x, x), torch.zeros(3, device=dev))
    assert torch.equal(ag.chamfer(x[:1], x[:1]), torch.zeros(1, device=dev))


def test_chamfer_at_the_lds_limit_and_one_past_it(ag, dev):
    from adaptigraph_amd.context import default_engine, ptr, current_stream
    N, M = 6739, 6741
    assert N + M == CR.CHAMFER_MAX_POINTS
    x, y, _, _ = CR.chamfer_case(N, M, 2, "none", R=2)
    got = ag.chamfer(_g(x, dev), _g(y, dev))
    _check("chamfer", f"N={N} M={M} By=2 (LDS limit)", got, CR.chamfer(x, y), CR.chamfer(x, y, dtype=F32))
    eng = default_engine(dev)
    xg, yg = torch.zeros((2, N + 1, 3), device=dev), _g(y, dev)
    out = torch.full((2,), -7.0, device=dev)
    with pytest.raises(NotImplementedError, match="exceeds the LDS tile"):
        eng.check(eng.lib.ag_cost_chamfer(eng.ctx, current_stream(dev), ptr(xg), ptr(yg), None, None, 2, N + 1, M, 2, ptr(out)))
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0, -7.0]
    with pytest.raises(NotImplementedError):
        ag.chamfer(xg, yg)


# ----------------------------------------------------------------------------------------------------------- chamfer backward
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("By", [1, 3])
@pytest.mark.parametrize("N,M", CR.CHAMFER_GRAD_SHAPES)
def test_chamfer_gradient_vs_float64_autograd(ag, dev, N, M, By, masked):
    x, y, xm, ym = CR.chamfer_grad_case(N, M, By, masked)
    w = np.random.default_rng(N + M).uniform(0.5, 1.5, 3).astype(np.float32)      # dLoss/dout, one weight per row
    refs = []
    for dt in (F64, F32):
        xr = torch.from_numpy(x).to(dt).requires_grad_(True)
        (CR.chamfer(xr, y, xm, ym, dt) * torch.from_numpy(w).to(dt)).sum().backward()
        refs.append(xr.grad)
    xg = _g(x, dev).requires_grad_(True)
    out = ag.chamfer_diff(xg, _g(y, dev), _g(xm, dev), _g(ym, dev))
    (out * _g(w, dev)).sum().backward()
    assert torch.equal(_bits(out), _bits(ag.chamfer(_g(x, dev), _g(y, dev), _g(xm, dev), _g(ym, dev))))
    if masked:
        assert float(xg.grad.cpu()[torch.from_numpy(~xm)].abs().max() if (~xm).any() else 0.0) == 0.0
    _check("chamfer_grad", f"N={N} M={M} By={By} masked={masked}", xg.grad, refs[0], refs[1])


# ----------------------------------------------------------------------------------------------------- box_loss / state_stats
@pytest.mark.parametrize("N", [1, 255, 256, 257, 2025])
def test_box_loss_and_bounds(ag, dev, N):
    s = CR.box_case(N)
    st = state_stats(_g(s, dev), _g(CR.BOX, dev))
    _check("state_stats", f"N={N}", st[:, 0], CR.box_loss(s, CR.BOX), CR.box_loss(s, CR.BOX, F32))
    assert torch.equal(_bits(ag.box_loss(_g(s, dev), _g(CR.BOX, dev))), _bits(st[:, 0]))
    assert torch.equal(_bits(st[:, 1:]), _bits(CR.bounds(s, F32)))                 # min / max: the inputs' own bits
    assert torch.equal(_bits(state_stats(_g(s, dev))[:, 1:]), _bits(st[:, 1:]))


# ------------------------------------------------------------------------------------------------------------------ penalties
@pytest.mark.parametrize("width", [3, 4])
@pytest.mark.parametrize("B,H", [(1, 1), (5, 3)])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_penalties(ag, dev, N, B, H, width):
    pred, act, init = CR.penalty_case(N, B, H, width)
    for kind in ("rope", "cloth", "granular"):
        got = getattr(ag, kind + "_penalty")(_g(pred, dev), _g(act, dev), _g(init, dev), sim_real_ratio=10.0)
        _check("penalty_" + kind, f"N={N} B={B} H={H} width={width}", got, CR.PENALTY[kind](pred, act, init, 10.0),
               CR.PENALTY[kind](pred, act, init, 10.0, F32))
    if H > 1 and N > 1:
        # step 0 reads state_init, step h >= 1 state_pred[:, h-1]: with the steps' clouds 1.5 apart, a kernel reading another
        # step's cloud is off by far more than the bar (tests/test_costs_restate.py checks that on the restatement)
        moved = pred.copy()
        moved[:, -1] += 100.0                                   # the last prediction is read by nobody
        for kind in ("rope", "granular"):
            fn = getattr(ag, kind + "_penalty")
            assert torch.equal(fn(_g(moved, dev), _g(act, dev), _g(init, dev)), fn(_g(pred, dev), _g(act, dev), _g(init, dev)))


def test_cloth_penalty_strided_combine_and_handed_in_maximum(ag, dev):
    from adaptigraph_amd.context import default_engine, ptr, current_stream
    from adaptigraph_amd.losses import _penalty_raw
    B, H, N = 400, 3, 64                                        # B*H = 1200 > 1024: k_cloth_combine strides
    pred, act, init = CR.penalty_case(N, B, H)
    inside = ag.cloth_penalty(_g(pred, dev), _g(act, dev), _g(init, dev), sim_real_ratio=10.0)
    _check("cloth_combine", f"B*H={B * H}", inside, CR.cloth_penalty(pred, act, init, 10.0), CR.cloth_penalty(pred, act, init, 10.0, F32))
    raw = _penalty_raw("cloth", _g(pred, dev), _g(act, dev), _g(init, dev), 10.0)
    _check("penalty_cloth", f"terms B*H={B * H}", raw, CR.cloth_terms(pred, act, init, 10.0), CR.cloth_terms(pred, act, init, 10.0, F32))
    dmax = raw[..., 1].max().reshape(1).contiguous()             # as `group` hands it in (losses._global_max)
    eng = default_engine(dev)
    handed = torch.empty((B, H), device=dev)
    eng.check(eng.lib.ag_cost_cloth_combine(eng.ctx, current_stream(dev), ptr(raw), ptr(dmax), B * H, ptr(handed)))
    assert torch.equal(_bits(handed), _bits(inside))


# --------------------------------------------------------------------------------------------------------------- running_cost
def _reward_funcs(ag, dev, target, err_name, kind):
    if err_name == "chamfer":
        dev_err, ref_err = partial(ag.chamfer, y=_g(target, dev)[None]), lambda dt: partial(CR.chamfer, y=target[None], dtype=dt)
    else:
        dev_err, ref_err = partial(ag.box_loss, target=_g(CR.BOX, dev)), lambda dt: partial(CR.box_loss, target=CR.BOX, dtype=dt)
    dev_pen = partial(getattr(ag, kind + "_penalty"), sim_real_ratio=10.0)
    ref_pen = lambda dt: partial(CR.PENALTY[kind], sim_real_ratio=10.0, dtype=dt)
    return dev_err, dev_pen, ref_err, ref_pen


@pytest.mark.parametrize("err_name", ["chamfer", "box"])
@pytest.mark.parametrize("H", [1, 20])
@pytest.mark.parametrize("B", [1, 1024, 1025, 2500])
def test_running_cost_across_the_reward_tree(ag, dev, B, H, err_name):
    from adaptigraph_amd.context import default_engine, ptr, current_stream
    state, act, init, target = CR.reward_case(B, H)
    dev_err, dev_pen, ref_err, ref_pen = _reward_funcs(ag, dev, target, err_name, "rope")
    sg, ag_, ig = _g(state, dev), _g(act, dev), _g(init, dev)
    got = ag.running_cost(sg, ag_, ig, error_func=dev_err, penalty_func=dev_pen, bbox=CR.BBOX)["reward_seqs"]
    refs = [CR.running_cost(state, act, init, ref_err(dt), ref_pen(dt), CR.BBOX, dt) for dt in (F64, F32)]
    _check("reward", f"B={B} H={H} error={err_name}", got, refs[0], refs[1])
    # d_error_max handed in (a sharded batch's all-reduced maximum) = formed inside: the same bits
    flat = sg.reshape(B * H, -1, 3)
    error = dev_err(flat).reshape(B, H).contiguous()
    pen, st = dev_pen(sg, ag_, ig).contiguous(), state_stats(flat)
    emax = error.max().reshape(1).contiguous()
    bbox4 = (C.c_double * 4)(*[float(v) for v in CR.BBOX.reshape(-1)])
    eng = default_engine(dev)
    handed = torch.empty(B, device=dev)
    eng.check(eng.lib.ag_cost_reward(eng.ctx, current_stream(dev), ptr(error), ptr(pen), ptr(st), ptr(emax), bbox4, B, H, ptr(handed)))
    assert torch.equal(_bits(handed), _bits(got))


# ----------------------------------------------------------------------------------------------------------------------- MPPI
@pytest.mark.parametrize("kind", CR.MPPI_REWARD_KINDS)
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("B", [1, 2, 1023, 1024, 1025, 20000])
def test_mppi_update_across_the_tree(ag, dev, B, H, kind):
    """Every component of every step; theta as a circular difference.  (The length divides |start - end| by push_length = 0.1: a
    kernel that recovers that vector as the difference of two fp32 point sums loses ten times what the sums lose, and missed the
    bar at B=1025 H=1 with equal rewards - k_mppi_update accumulates the vector itself, in double.)"""
    a, r = CR.mppi_case(B, H, kind)
    inf4 = np.full(4, np.inf, np.float32)
    for lo, hi, tag in ((CR.MPPI_LO, CR.MPPI_HI, "limits"), (-inf4, inf4, "free")):
        got = ag.optimize_action_mppi(_g(a, dev), _g(r, dev), CR.MPPI_REWARD_WEIGHT, _g(lo, dev), _g(hi, dev), 0.1)
        refs = [CR.mppi_update(a, r, CR.MPPI_REWARD_WEIGHT, lo, hi, 0.1, dt) for dt in (F64, F32)]
        circ = torch.zeros((H, 4), dtype=torch.bool)
        circ[:, 2] = True
        _check("mppi_update", f"B={B} H={H} rewards={kind} {tag}", got, refs[0], refs[1], circular=circ)


def test_clip_actions_at_the_wrap_bitwise(ag, dev):
    """torch.remainder semantics at -pi, pi, their fp32 neighbours, +-3 pi, +-1e4: the fp32 restatement's bits."""
    a = CR.clip_case()
    inf4 = np.full(4, np.inf, np.float32)
    for lo, hi in ((CR.MPPI_LO, CR.MPPI_HI), (-inf4, inf4)):
        got = ag.clip_actions(_g(a, dev), _g(lo, dev), _g(hi, dev))
        want = CR.clip_actions(a, lo, hi, F32)
        assert torch.equal(_bits(got), _bits(want)), (got.cpu()[:, 2], want[:, 2])
    assert torch.equal(_bits(ag.angle_normalize(_g(a[:, 2].copy(), dev))), _bits(CR.angle_normalize(torch.from_numpy(a[:, 2].copy()))))


def test_mode1_sample_landing_exactly_on_pi_wraps_like_the_reference(ag, dev):
    """Nominal theta = 0 and equal noise on the start's and the end's second coordinate: atan2(+0, negative) = pi exactly, which
    the wrap sends to -pi.  cos 0 = 1 and sin 0 = 0 are exact, so every component is the fp32 restatement's bits."""
    act_seq = np.array([[-2.0, 1.0, 0.0, 5.0]], np.float32)
    noise = np.zeros((1, 4, 4), np.float32)
    noise[0, 1] = [0.5, 0.25, 7.0, 0.25]                       # end point pushed past the start point: the push turns round
    noise[0, 2] = [0.5, 0.25, -1.0, 0.25]                      # ... and not
    noise[0, 3] = [-0.5, 0.75, 6.0, 0.75]
    inf4 = np.full(4, np.inf, np.float32)
    for lo, hi in ((-inf4, inf4), (CR.MPPI_LO, CR.MPPI_HI)):
        got = ag.sample_action_seq(_g(act_seq, dev), _g(lo, dev), _g(hi, dev), 4, dev, iter_index=1, push_length=0.1, _draws=noise)
        want = CR.mppi_perturb(act_seq, noise, lo, hi, 0.1, F32)
        assert torch.equal(_bits(got), _bits(want)), (got.cpu(), want)
    free = CR.mppi_perturb(act_seq, noise, -inf4, inf4, 0.1, F32)
    assert float(free[1, 0, 2]) == -float(np.float32(np.pi)) and float(free[2, 0, 2]) == 0.0


# ---------------------------------------------------------------------------------------------------------- non-finite inputs
def _same_nonfinite(kernel, case, got, want32, ref64=None):
    """NaN pattern and infinities exactly as the fp32 restatement on the CPU; finite entries by the bar above."""
    got_c, want = got.detach().cpu(), want32.detach()
    assert torch.equal(torch.isnan(got_c), torch.isnan(want)), (kernel, case, got_c, want)
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got_c), inf) and torch.equal(got_c[inf], want[inf].to(got_c.dtype)), (kernel, case, got_c, want)
    fin = torch.isfinite(want)
    if ref64 is not None and bool(fin.any()):
        _check(kernel, case, got_c[fin], ref64[fin], want[fin])


@pytest.fixture(scope="module")
def clean(ag, dev):
    """R=3, N=150, M=211 clouds and their clean chamfer (device), shared by the non-finite tests."""
    x, y, _, _ = CR.chamfer_case(150, 211, 1, "none")
    return x, y, ag.chamfer(_g(x, dev), _g(y, dev))


def test_one_nan_coordinate_makes_its_row_nan_and_no_other(ag, dev, clean):
    x, y, base = clean
    bad = x.copy()
    bad[1, 77, 1] = np.nan
    got = ag.chamfer(_g(bad, dev), _g(y, dev))
    assert torch.isnan(got).tolist() == [False, True, False]
    assert torch.equal(_bits(got[[0, 2]]), _bits(base[[0, 2]]))
    _same_nonfinite("chamfer", "one NaN in x", got, CR.chamfer(bad, y, dtype=F32), CR.chamfer(bad, y))


def test_nan_in_a_shared_target_makes_every_row_nan(ag, dev, clean):
    x, y, _ = clean
    bad = y.copy()
    bad[0, 200, 0] = np.nan
    got = ag.chamfer(_g(x, dev), _g(bad, dev))
    assert torch.isnan(got).all()
    _same_nonfinite("chamfer", "one NaN in y", got, CR.chamfer(x, bad, dtype=F32))


def test_infinite_coordinates_give_what_the_restatement_gives(ag, dev, clean):
    x, y, base = clean
    bad = x.copy()
    bad[0, 3, 0] = np.inf
    bad[2, 149, 2] = -np.inf
    got = ag.chamfer(_g(bad, dev), _g(y, dev))
    assert got.tolist()[0] == INF and got.tolist()[2] == INF and torch.equal(_bits(got[1]), _bits(base[1]))
    _same_nonfinite("chamfer", "+inf and -inf in x", got, CR.chamfer(bad, y, dtype=F32), CR.chamfer(bad, y))


def test_an_all_nan_row_is_nan_in_every_reduction_that_reads_it(ag, dev):
    B, H, N = 2, 3, 150
    pred, act, init = CR.penalty_case(N, B, H)
    _, y, _, _ = CR.chamfer_case(N, 211, 1, "none")
    pred[1, 0] = np.nan                                          # read by chamfer / stats row 3 and by the penalties' step (1, 1)
    flat = pred.reshape(B * H, N, 3)
    row = [False, False, False, True, False, False]
    got = ag.chamfer(_g(flat, dev), _g(y, dev))
    assert torch.isnan(got).tolist() == row
    _same_nonfinite("chamfer", "all-NaN row", got, CR.chamfer(flat, y, dtype=F32), CR.chamfer(flat, y))
    st = state_stats(_g(flat, dev), _g(CR.BOX, dev))
    assert torch.isnan(st).tolist() == [[r] * 5 for r in row]
    _same_nonfinite("state_stats", "all-NaN row", st[:, 0], CR.box_loss(flat, CR.BOX, F32), CR.box_loss(flat, CR.BOX))
    _same_nonfinite("state_stats", "all-NaN row bounds", st[:, 1:], CR.bounds(flat, F32))
    step = [[False, False, False], [False, True, False]]
    for kind in ("rope", "granular"):
        got = getattr(ag, kind + "_penalty")(_g(pred, dev), _g(act, dev), _g(init, dev), sim_real_ratio=10.0)
        assert torch.isnan(got).tolist() == step, kind
        _same_nonfinite("penalty_" + kind, "all-NaN row", got, CR.PENALTY[kind](pred, act, init, 10.0, F32),
                        CR.PENALTY[kind](pred, act, init, 10.0))
    ok = np.nan_to_num(pred, nan=0.0)
    cloth = ag.cloth_penalty(_g(pred, dev), _g(act, dev), _g(init, dev), sim_real_ratio=10.0)
    assert torch.equal(_bits(cloth), _bits(ag.cloth_penalty(_g(ok, dev), _g(act, dev), _g(init, dev), sim_real_ratio=10.0)))
    assert bool(torch.isfinite(cloth).all())                     # cloth reads state_init only


@pytest.mark.parametrize("kind", ["rope", "cloth", "granular"])
@pytest.mark.parametrize("err_name", ["box", "chamfer"])
def test_an_all_nan_candidate_makes_every_reward_nan(ag, dev, err_name, kind):
    """What the asynchronous rollout writes for a candidate whose edge list overflowed.  The reference's error.max() is NaN, so
    every reward of the batch is: loud.  Scoring that candidate 0 - the best value a reward can take - would steer MPPI to it."""
    state, act, init, target = CR.reward_case(8, 3)
    state[5] = np.nan
    dev_err, dev_pen, ref_err, ref_pen = _reward_funcs(ag, dev, target, err_name, kind)
    got = ag.running_cost(_g(state, dev), _g(act, dev), _g(init, dev), error_func=dev_err, penalty_func=dev_pen,
                          bbox=CR.BBOX)["reward_seqs"]
    want = CR.running_cost(state, act, init, ref_err(F32), ref_pen(F32), CR.BBOX, F32)
    assert torch.isnan(want).all()
    _same_nonfinite("reward", f"all-NaN candidate {err_name} {kind}", got, want)
    assert not bool((got[5] >= torch.nan_to_num(got, nan=-INF).max()))      # the NaN candidate is not the batch's best


def test_nan_action_makes_the_whole_cloth_penalty_nan(ag, dev):
    pred, act, init = CR.penalty_case(64, 400, 3)
    act[123, 1, 0] = np.nan
    got = ag.cloth_penalty(_g(pred, dev), _g(act, dev), _g(init, dev), sim_real_ratio=10.0)
    want = CR.cloth_penalty(pred, act, init, 10.0, F32)
    assert torch.isnan(want).all()
    _same_nonfinite("cloth_combine", "NaN action", got, want)
