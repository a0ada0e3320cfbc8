"""tests/costs_restate.py against the reference's recorded outputs (tests/golden/costs.npz, mppi.npz), in float64, at the
tolerances the fp32 oracle and the device kernels already meet on those fixtures (test_oracle_vs_golden.py, test_mppi.py) - which
is what makes the restatement a reference for tests/test_gpu_costs_edges.py; and the preconditions of that file's seeded inputs
(unambiguous nearest neighbours, finite clean inputs, the boundaries the shapes are meant to cross).  CPU only.
"""
from functools import partial

import numpy as np
import pytest
import torch

import costs_restate as CR
from helpers import load_golden
from test_oracle_vs_golden import COST_TOL
from test_mppi import ATOL, RTOL

F64 = torch.float64


def test_float64_restatement_reproduces_the_cost_golden():
    g = load_golden("costs")
    B, H, N, _ = g["state"].shape
    flat = g["state"].reshape(B * H, N, 3)
    assert np.abs(CR.chamfer(flat, g["target"][None]).numpy() - g["chamfer"]).max() < COST_TOL
    assert np.abs(CR.box_loss(flat, g["target_box"]).numpy() - g["box_loss"]).max() < COST_TOL
    for kind in ("rope", "cloth", "granular"):
        got = CR.PENALTY[kind](g["state"], g["action"], g["state_cur"], 10.0).numpy()
        assert np.abs(got - g[kind + "_penalty"]).max() < COST_TOL, kind
    mc = CR.chamfer(g["mc_pred"], g["mc_real"], g["mc_pred_mask"], g["mc_real_mask"]).numpy()
    assert np.abs(mc - g["mean_chamfer"]).max() < COST_TOL
    for err_name in ("chamfer", "box"):
        err = partial(CR.chamfer, y=g["target"][None]) if err_name == "chamfer" else partial(CR.box_loss, target=g["target_box"])
        for kind in ("rope", "cloth", "granular"):
            r = CR.running_cost(g["state"], g["action"], g["state_cur"], err, partial(CR.PENALTY[kind], sim_real_ratio=10.0),
                                g["bbox"]).numpy()
            want = g[f"reward::{err_name}::{kind}"]
            assert np.abs(r - want).max() < 5e-5 * max(1.0, np.abs(want).max()), (err_name, kind)


def test_float64_restatement_reproduces_the_mppi_golden():
    g = load_golden("mppi")
    up = CR.mppi_update(g["sample_iter1"], g["rewards"], 500.0, g["lo"], g["hi"], 0.1).numpy()
    assert np.all(np.abs(up - g["mppi"]) <= ATOL + RTOL * np.abs(g["mppi"])), np.abs(up - g["mppi"]).max()
    cl = CR.clip_actions(g["wild"], g["lo"], g["hi"]).numpy()
    assert np.all(np.abs(cl - g["clipped"]) <= ATOL + RTOL * np.abs(g["clipped"])), np.abs(cl - g["clipped"]).max()
    # in fp32 the clip is the reference's own arithmetic: the same bits (what the device is held to at the wrap, too)
    assert np.array_equal(CR.clip_actions(g["wild"], g["lo"], g["hi"], torch.float32).numpy(), g["clipped"])


def test_cloth_terms_recombine_to_cloth_penalty():
    g = load_golden("costs")
    t = CR.cloth_terms(g["state"], g["action"], g["state_cur"], 10.0)
    assert torch.equal(CR.cloth_combine(t), CR.cloth_penalty(g["state"], g["action"], g["state_cur"], 10.0))


def test_restatement_propagates_nan_like_torch():
    """What item 3 of the sweep expects of the kernels is what these give: NaN in, NaN out, through every min / max."""
    g = load_golden("costs")
    x = g["state"].reshape(18, 150, 3)[:3].copy()
    x[1, 7, 2] = np.nan
    c = CR.chamfer(x, g["target"][None], dtype=torch.float32)
    assert torch.isnan(c).tolist() == [False, True, False]
    assert torch.isnan(CR.box_loss(x, g["target_box"], torch.float32)).tolist() == [False, True, False]
    assert torch.isnan(CR.bounds(x, torch.float32)).tolist() == [[False] * 4, [False, False, True, True], [False] * 4]
    x[1, 7, 2] = np.inf
    assert CR.chamfer(x, g["target"][None], dtype=torch.float32)[1] == np.inf


# ---- preconditions of the device sweep's inputs
@pytest.mark.parametrize("N,M", CR.CHAMFER_GRAD_SHAPES)
@pytest.mark.parametrize("By", [1, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_chamfer_gradient_inputs_have_unambiguous_neighbours(N, M, By, masked):
    x, y, xm, ym = CR.chamfer_grad_case(N, M, By, masked)
    assert CR.nn_margin(x, y, xm, ym) > CR.TIE_MARGIN
    assert np.isfinite(x).all() and np.isfinite(y).all()
    if masked:
        assert xm.any(1).all() and ym.any(1).all()


def test_sweep_inputs_are_finite_and_cross_their_boundaries():
    for (N, M) in CR.CHAMFER_SHAPES:
        for By in (1, 3):
            for kind in CR.MASK_KINDS:
                x, y, xm, ym = CR.chamfer_case(N, M, By, kind)
                assert np.isfinite(x).all() and np.isfinite(y).all() and np.abs(x).max() < 8
                if kind != "none":
                    assert xm.any(1).all() and ym.any(1).all()
                    if kind == "one":
                        assert (xm.sum(1) == 1).all() and (ym.sum(1) == 1).all()
                    gx, gy = CR.with_garbage(x, xm), CR.with_garbage(y, ym)
                    assert np.array_equal(gx[xm], x[xm]) and np.array_equal(gy[ym], y[ym])
                    assert xm.all() or not np.isfinite(gx[~xm]).all() or np.abs(gx[~xm]).max() >= 1e30
    assert CR.CHAMFER_MAX_POINTS == 6739 + 6741
    for N in (1, 255, 256, 257, 2025):
        s = CR.box_case(N)
        (x0, x1), (z0, z1) = CR.BOX
        assert np.isfinite(s).all()
        on_edge = ((s[..., 0] == x0) | (s[..., 0] == x1) | (s[..., 2] == z0) | (s[..., 2] == z1))
        assert on_edge.any()
        if N > 8:
            inside = (s[..., 0] > x0) & (s[..., 0] < x1) & (s[..., 2] > z0) & (s[..., 2] < z1)
            assert inside.any() and (~inside & ~on_edge).any()
    for (B, H) in ((1, 1), (5, 3)):
        pred, act, init = CR.penalty_case(257, B, H)
        assert np.isfinite(pred).all() and np.isfinite(act).all()
        if H > 1:      # the steps' clouds are further apart than any pusher size: reading the wrong step cannot go unnoticed
            c = np.concatenate([init[None], pred[0]], 0).mean(1)
            assert np.linalg.norm(c[1:] - c[:-1], axis=1).min() > 1.0 > 0.2
            right = CR.rope_penalty(pred, act, init).numpy()
            wrong = CR.rope_penalty(np.roll(pred, 1, 1), act, init).numpy()
            assert np.abs(right - wrong)[:, 2:].max() > 1e-3
    for kind in CR.MPPI_REWARD_KINDS:
        a, r = CR.mppi_case(20000, 3, kind)
        w = torch.softmax(CR.T(r, torch.float32) * CR.MPPI_REWARD_WEIGHT, 0)
        assert np.isfinite(a).all() and np.isfinite(r).all()
        if kind == "spread":                                  # most candidates' weights leave fp32's normal range (many reach zero)
            assert abs(float(r.max() - r.min()) * CR.MPPI_REWARD_WEIGHT - 200) < 1
            assert float((w < torch.finfo(torch.float32).tiny).float().mean()) > 0.5 and float((w == 0).float().mean()) > 0.4
        if kind == "dominant":
            assert float(w.max()) == 1.0
        th = a[:, 1, 2]
        assert (th > np.pi).any() and (th < np.pi).any()     # candidates on both sides of the wrap
    th = CR.clip_case()[:, 2]
    pi = np.float32(np.pi)
    assert {-pi, pi, 3 * pi, -3 * pi, np.float32(1e4), np.float32(-1e4)} <= set(th.tolist())
    assert (th == np.nextafter(pi, np.float32(4))).any() and (th == np.nextafter(-pi, np.float32(0))).any()
