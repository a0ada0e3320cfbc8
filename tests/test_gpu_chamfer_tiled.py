"""The tiled Chamfer cost (csrc/ag_chamfer_tiled.hip: chamfer_tiled, chamfer_tiled_diff) against chamfer() / chamfer_diff() bit for
bit wherever both apply - at the loop ends of the 1024-point ownership and of the tiles, on non-finite rows, at exact ties - and
against the float64 restatement (tests/costs_restate.py) beyond the LDS limit, under the bar of tests/test_gpu_costs_edges.py:
error against float64 at most 4x the fp32 restatement's plus 1e-7 max|ref|, never more than COST_TOL."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import chamfer_tiled_cases as TC
import costs_restate as CR
from test_gpu_costs_edges import _bits, _check, _g, _same_nonfinite

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
TILES = (2, 64, None)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ag():
    import adaptigraph_amd
    return adaptigraph_amd


# -------------------------------------------------------------------------------------------- 1. chamfer()'s bits at the loop ends
@pytest.mark.parametrize("mask_kind", CR.MASK_KINDS)
@pytest.mark.parametrize("By", [1, 3])
@pytest.mark.parametrize("N,M", CR.CHAMFER_SHAPES + TC.EXTRA_SHAPES)
def test_forward_has_chamfer_s_bits_for_every_tile(ag, dev, N, M, By, mask_kind):
    x, y, xm, ym = CR.chamfer_case(N, M, By, mask_kind)
    want = ag.chamfer(_g(x, dev), _g(y, dev), _g(xm, dev), _g(ym, dev))
    assert bool(torch.isfinite(want).all())
    for tile in TILES:
        got = ag.chamfer_tiled(_g(x, dev), _g(y, dev), _g(xm, dev), _g(ym, dev), tile=tile)
        assert torch.equal(_bits(got), _bits(want)), (tile, got, want)
        if mask_kind != "none":      # what sits in a masked-out slot is never looked at
            junk = ag.chamfer_tiled(_g(CR.with_garbage(x, xm), dev), _g(CR.with_garbage(y, ym), dev), _g(xm, dev), _g(ym, dev), tile=tile)
            assert torch.equal(_bits(junk), _bits(want)), tile
    if mask_kind != "none":
        assert np.array_equal(ag.mean_chamfer_tiled(_g(x, dev), _g(y, dev), _g(xm, dev), _g(ym, dev)),
                              ag.mean_chamfer(_g(x, dev), _g(y, dev), _g(xm, dev), _g(ym, dev)))


@pytest.mark.parametrize("N", [1, 5, 1025, 8192])
def test_a_cloud_against_itself_is_exactly_zero(ag, dev, N):
    x = _g(np.random.default_rng([27, N]).normal(0, 1, (3, N, 3)).astype(np.float32), dev)
    for tile in TILES:
        assert torch.equal(ag.chamfer_tiled(x, x, tile=tile), torch.zeros(3, device=dev))
        assert torch.equal(ag.chamfer_tiled(x[:1], x[:1], tile=tile), torch.zeros(1, device=dev))


# ------------------------------------------------------------------------------------------------------------ 2. non-finite rows
@pytest.fixture(scope="module")
def clean(ag, dev):
    """R=3, N=150, M=211 clouds with one shared target, and their clean chamfer_tiled at tile 64."""
    x, y, _, _ = CR.chamfer_case(150, 211, 1, "none")
    return x, y, ag.chamfer_tiled(_g(x, dev), _g(y, dev), tile=64)


def _nonfinite_cases(x, y):
    a = x.copy(); a[1, 77, 1] = np.nan
    yield "one NaN in a valid x", a, y, [1]
    b = y.copy(); b[0, 200, 0] = np.nan
    yield "one NaN in the shared y", x, b, [0, 1, 2]
    c = x.copy(); c[0, 3, 0] = np.inf; c[2, 149, 2] = -np.inf
    yield "+inf and -inf in x", c, y, [0, 2]
    d, e = x.copy(), y.copy(); d[0, 3, 0] = np.inf; e[0, 5, 0] = np.inf
    yield "inf in both clouds (inf - inf)", d, e, [0, 1, 2]


def test_non_finite_rows_are_what_chamfer_makes_them_and_clean_rows_keep_their_bits(ag, dev, clean):
    x, y, base = clean
    assert torch.equal(_bits(base), _bits(ag.chamfer(_g(x, dev), _g(y, dev))))
    for case, bx, by, rows in _nonfinite_cases(x, y):
        got = ag.chamfer_tiled(_g(bx, dev), _g(by, dev), tile=64)
        ref = ag.chamfer(_g(bx, dev), _g(by, dev))
        print(case, got.tolist(), ref.tolist())
        assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.isinf(got), torch.isinf(ref)), (case, got, ref)
        assert (~torch.isfinite(got)).nonzero().flatten().tolist() == rows, (case, got)
        assert bool((got[torch.isinf(got)] > 0).all())
        _same_nonfinite("chamfer_tiled", case, got, CR.chamfer(bx, by, dtype=F32))
        ok = [r for r in range(3) if r not in rows]
        assert torch.equal(_bits(got[ok]), _bits(base[ok])), case


# ------------------------------------------------------------------------------------ 3. beyond the limit, exact: prefix embedding
@pytest.mark.parametrize("fill", [0.0, np.nan])
@pytest.mark.parametrize("By", [1, 3])
def test_prefix_embedding_past_the_limit_has_the_compact_case_s_bits(ag, dev, By, fill):
    """A point's lane and stride depend on its index alone, and masked-out slots are parked: 257 + 255 points as the first rows of
    7000 + 7000 slots give chamfer()'s and chamfer_diff()'s bits of the compact clouds."""
    (x, y), (X, Y, Xm, Ym) = TC.prefix_embedding(By, fill)
    n, m, N, M = TC.PREFIX
    assert N + M > CR.CHAMFER_MAX_POINTS
    w = _g(np.random.default_rng(n + m).uniform(0.5, 1.5, 3).astype(np.float32), dev)
    xc = _g(x, dev).requires_grad_(True)
    want = ag.chamfer_diff(xc, _g(y, dev))
    (want * w).sum().backward()
    assert torch.equal(_bits(want), _bits(ag.chamfer(_g(x, dev), _g(y, dev))))
    assert torch.equal(_bits(ag.chamfer_tiled(_g(X, dev), _g(Y, dev), _g(Xm, dev), _g(Ym, dev))), _bits(want))
    Xg = _g(X, dev).requires_grad_(True)
    got = ag.chamfer_tiled_diff(Xg, _g(Y, dev), _g(Xm, dev), _g(Ym, dev))
    (got * w).sum().backward()
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(Xg.grad[:, :n]), _bits(xc.grad))
    assert torch.equal(_bits(Xg.grad[:, n:]), torch.zeros((3, N - n, 3), dtype=torch.int32))       # exact +0.0


# ------------------------------------------------------------------------------------------------- 4. beyond the limit, dense
@pytest.fixture(scope="module")
def dense():
    return TC.dense_case()


def test_dense_case_one_point_past_the_limit(ag, dev, dense):
    x, y = dense
    N, M = TC.DENSE
    assert N + M == CR.CHAMFER_MAX_POINTS + 1
    with pytest.raises(NotImplementedError):                 # chamfer() keeps its limit and its refusal
        ag.chamfer(_g(x, dev), _g(y, dev))
    got = ag.chamfer_tiled(_g(x, dev), _g(y, dev))
    _check("chamfer_tiled", f"N={N} M={M} By=2", got, CR.chamfer(x, y), CR.chamfer(x, y, dtype=F32))
    assert torch.equal(_bits(ag.chamfer_tiled(_g(x, dev), _g(y, dev), tile=1024)), _bits(got))


@pytest.mark.parametrize("N,M", [(20000, 33), (3, 20000)])
def test_the_planner_s_shape_one_shared_target(ag, dev, N, M):
    x, y, _, _ = CR.chamfer_case(N, M, 1, "none")
    got = ag.chamfer_tiled(_g(x, dev), _g(y, dev))
    _check("chamfer_tiled", f"N={N} M={M} By=1", got, CR.chamfer(x, y), CR.chamfer(x, y, dtype=F32))


def test_running_cost_scores_rollouts_past_the_limit(ag, dev):
    B, H, N = 2, 2, 13500
    state, act, init, target = CR.reward_case(B, H, N)
    assert N + target.shape[0] > CR.CHAMFER_MAX_POINTS
    dev_err = partial(ag.chamfer_tiled, y=_g(target, dev)[None])
    dev_pen = partial(ag.rope_penalty, sim_real_ratio=10.0)
    got = ag.running_cost(_g(state, dev), _g(act, dev), _g(init, dev), error_func=dev_err, penalty_func=dev_pen, bbox=CR.BBOX)["reward_seqs"]
    refs = [CR.running_cost(state, act, init, partial(CR.chamfer, y=target[None], dtype=dt),
                            partial(CR.rope_penalty, sim_real_ratio=10.0, dtype=dt), CR.BBOX, dt) for dt in (F64, F32)]
    _check("reward", f"B={B} H={H} N={N} error=chamfer_tiled", got, refs[0], refs[1])


# --------------------------------------------------------------------------------------------------------------- 5. gradient
def _grads(fn, x, y, xm, ym, w, dev, **kw):
    xg = _g(x, dev).requires_grad_(True)
    out = fn(xg, _g(y, dev), _g(xm, dev), _g(ym, dev), **kw)
    (out * _g(w, dev)).sum().backward()
    return out, xg.grad


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("By", [1, 3])
@pytest.mark.parametrize("N,M", CR.CHAMFER_GRAD_SHAPES + [(2049, 5)])
def test_gradient_has_chamfer_diff_s_bits(ag, dev, N, M, By, masked):
    x, y, xm, ym = CR.chamfer_grad_case(N, M, By, masked)
    w = np.random.default_rng(N + M).uniform(0.5, 1.5, 3).astype(np.float32)
    out, grad = _grads(ag.chamfer_diff, x, y, xm, ym, w, dev)
    for tile in (2, 64):
        got, g = _grads(ag.chamfer_tiled_diff, x, y, xm, ym, w, dev, tile=tile)
        assert torch.equal(_bits(got), _bits(out)) and torch.equal(_bits(g), _bits(grad)), tile
    if masked and (~xm).any():
        assert torch.equal(_bits(g.cpu()[torch.from_numpy(~xm)]), torch.zeros((int((~xm).sum()), 3), dtype=torch.int32))


def test_exact_ties_route_to_the_lowest_index_across_tiles_and_owning_blocks(ag, dev):
    x, y = TC.tie_case()
    a, b, c = TC.TIE_ROWS
    w = np.float32([0.75, 1.25])
    out, grad = _grads(ag.chamfer_diff, x, y, None, None, w, dev)
    got, g = _grads(ag.chamfer_tiled_diff, x, y, None, None, w, dev, tile=64)
    assert torch.equal(_bits(got), _bits(out)) and torch.equal(_bits(g), _bits(grad))
    # the three copies share their own term (the same nearest y); the y-side share of TIE_Y reaches row `a` alone
    assert torch.equal(_bits(g[:, b]), _bits(g[:, c])) and not torch.equal(_bits(g[:, a]), _bits(g[:, b]))
    xs, ys = torch.from_numpy(x).to(F64), torch.from_numpy(y).to(F64)
    for r in range(2):
        j = int(torch.linalg.vector_norm(ys[r] - xs[r, a], dim=-1).argmin())
        assert j in TC.TIE_Y
        own = float(w[r]) / x.shape[1] * (xs[r, a] - ys[r, j]) / torch.linalg.vector_norm(xs[r, a] - ys[r, j])
        share = sum(float(w[r]) / y.shape[1] * (xs[r, a] - ys[r, k]) / torch.linalg.vector_norm(xs[r, a] - ys[r, k]) for k in TC.TIE_Y)
        assert torch.allclose(g[r, b].cpu().to(F64), own, rtol=1e-3, atol=1e-7)      # (the points lie ~1e-3 apart: fp32 directions)
        assert torch.allclose(g[r, a].cpu().to(F64), own + share, rtol=1e-3, atol=1e-7)


def test_dense_gradient_past_the_limit_vs_float64_autograd(ag, dev, dense):
    """Row by row against float64 autograd of the restatement, without the x rows a near-tie touches (their arg-min is a matter of
    fp32 rounding): at most 1 % of the rows - 38 and 33 of 6740 for this seed (tests/test_chamfer_tiled_host.py)."""
    x, y = dense
    N, M = TC.DENSE
    w = np.random.default_rng(N + M).uniform(0.5, 1.5, 2).astype(np.float32)
    out_rows = TC.near_tie_rows(x, y)
    assert float(out_rows.mean(1).max()) <= 0.01
    _, g = _grads(ag.chamfer_tiled_diff, x, y, None, None, w, dev)
    for r in range(2):
        refs = []
        for dt in (F64, F32):
            xr = torch.from_numpy(x[r:r + 1]).to(dt).requires_grad_(True)
            (CR.chamfer(xr, y[r:r + 1], dtype=dt) * float(w[r])).sum().backward()
            refs.append(xr.grad[0])
        keep = torch.from_numpy(~out_rows[r])
        _check("chamfer_tiled_grad", f"N={N} M={M} row {r} ({int((~keep).sum())} rows left out)", g[r].cpu()[keep], refs[0][keep], refs[1][keep])


# --------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_output_untouched(ag, dev):
    from adaptigraph_amd import _lib
    from adaptigraph_amd.context import default_engine, ptr, current_stream
    eng, cells = default_engine(dev), _lib.load_cells()
    x, y = torch.zeros((2, 9, 3), device=dev), torch.zeros((2, 7, 3), device=dev)
    out = torch.full((2,), -7.0, device=dev)
    gx, go = torch.full((2, 9, 3), -7.0, device=dev), torch.ones(2, device=dev)
    for tile in (3, -2, _lib.CHAMFER_TILED_MAX_TILE + 2):
        assert cells.ag_cost_chamfer_tiled(eng.ctx, current_stream(dev), ptr(x), ptr(y), None, None, 2, 9, 7, 2, tile, ptr(out)) == _lib.AG_ERR_INVALID
        assert cells.ag_cost_chamfer_tiled_backward(eng.ctx, current_stream(dev), ptr(x), ptr(y), None, None, 2, 9, 7, 2, tile, ptr(go),
                                                    ptr(gx)) == _lib.AG_ERR_INVALID
        with pytest.raises(AssertionError, match="tile_points"):
            ag.chamfer_tiled(x, y, tile=tile)
    # N = 1,048,577: refused before anything is read, so only y and the outputs need to exist
    big = _lib.CHAMFER_TILED_MAX_POINTS + 1
    assert big == 1048577
    for args in ((2, big, 7, 2), (2, 9, big, 2)):
        assert cells.ag_cost_chamfer_tiled(eng.ctx, current_stream(dev), ptr(x), ptr(y), None, None, *args, 0, ptr(out)) == _lib.AG_ERR_UNSUPPORTED
        assert b"exceed the tiled kernels' limit" in eng.lib.ag_last_error(eng.ctx)
        assert cells.ag_cost_chamfer_tiled_backward(eng.ctx, current_stream(dev), ptr(x), ptr(y), None, None, *args, 0, ptr(go),
                                                    ptr(gx)) == _lib.AG_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        eng.check(cells.ag_cost_chamfer_tiled(eng.ctx, current_stream(dev), ptr(x), ptr(y), None, None, 2, big, 7, 2, 0, ptr(out)))
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0, -7.0] and bool((gx == -7.0).all())
    assert torch.equal(ag.chamfer_tiled(x, y, tile=_lib.CHAMFER_TILED_MAX_TILE), torch.zeros(2, device=dev))     # the largest tile runs
    # chamfer() itself keeps its limit
    with pytest.raises(NotImplementedError, match="exceeds the LDS tile"):
        ag.chamfer(torch.zeros((1, 6740, 3), device=dev), torch.zeros((1, 6741, 3), device=dev))
