"""The training set-loss kernels (csrc/ag_setloss.hip: k_set_nn, k_set_final, k_step_loss_final, k_set_grad) where their fixtures
never take them (-m gpu): the ends of k_set_nn's 256-wide stride over N + M, exact ties through every layer of the arg-max, NaN and
inf coordinates, the LDS limit and one point past it, a part's share of the Chamfer mean, and the fused step with all three terms
at n_p = 257.

Yardstick: tests/set_loss_edges.py::set_rule in float64 on the same fp32 inputs (held against the reference's recordings, torch in
float64 and its own mutants by tests/test_set_loss_edges.py).  Bar, the project's convention (tests/test_gpu_costs_edges.py::_check):
err <= min(4 err32 + 1e-7 max|ref|, fixed), err32 = the same rule run in fp32 on the CPU, fixed = what tests/test_gpu_set_losses.py
applies (value 1e-5 relative; gradient 1e-4 max|g_ref| + 1e-7).  Arg-min tables and winners are integers and compared as such.
Every case prints both errors and ratio = err / (err32 + 0.25e-7 max|ref|), the quantity the bar holds to 4 (DESIGN.md section 3.19
records the largest seen).

No test hands a stale or out-of-range table to the backward: the clamp there guards an address."""
import functools

import numpy as np
import pytest
import torch

import backward_shapes as BS
import costs_restate as CR
import set_loss_edges as E
import train_restate as TR
from test_gpu_emd import _raw
from test_gpu_train import _model, _edge_list
from test_gpu_train_step import _t

pytestmark = pytest.mark.gpu

KIND = {"chamfer": 1, "hausdorff": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _check(kernel, case, got, ref64, ref32, fixed):
    """got, ref64 (the rule in float64), ref32 (in fp32): arrays or scalars, all finite"""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape and np.isfinite(ref64).all() and np.isfinite(got).all(), (kernel, case)
    err, err32, scale = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max()), float(np.abs(ref64).max())
    print(f"RATIO {kernel} {case}: err {err:.3e} fp32-restatement {err32:.3e} max|ref| {scale:.3e} ratio {E.ratio(err, err32, scale):.2f}")
    assert err <= min(4 * err32 + 1e-7 * scale, fixed(scale)), (kernel, case, err, err32)


VALUE_FIXED = lambda scale: 1e-5 * scale             # noqa: E731
GRAD_FIXED = lambda scale: 1e-4 * scale + 1e-7       # noqa: E731


def _module(name):
    import adaptigraph_amd as ag
    return {"chamfer": ag.ChamferLoss, "hausdorff": ag.HausdorffLoss}[name]()


def _tables(wk, B, N, M):
    t = wk[:B * (N + M)].view(B, N + M).cpu().numpy()
    return t[:, :N], t[:, N:], wk[B * (N + M):].cpu().tolist()


def _backward_raw(dev, x, y, kind, go, work, B_total=None):
    """ag_set_loss_backward at the boundary -> (return code, gradient)"""
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import ptr, current_stream
    eng = ag.default_engine(dev)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    g = torch.full_like(x, -7.0)
    got = torch.full((1,), float(go), device=dev)
    rc = eng.lib.ag_set_loss_backward(eng.ctx, current_stream(dev), ptr(x), ptr(y), B, N, M, B if B_total is None else B_total, kind,
                                      ptr(got), ptr(g), None if work is None else ptr(work))
    torch.cuda.synchronize()
    return rc, g


def _run(dev, xn, yn, name, grad_out=3.0):
    """the module forward and backward, and the boundary's tables -> (value, gradient tensor, nnx, nny, winners, work buffer)"""
    B, N, M = xn.shape[0], xn.shape[1], yn.shape[1]
    x, y = _t(xn, dev).requires_grad_(True), _t(yn, dev)
    v = _module(name)(x, y)
    assert v.dim() == 0 and v.is_cuda
    (grad_out * v).backward()
    rc, out, wk = _raw(dev, x.detach(), y, kind=KIND[name])
    assert rc == 0 and torch.equal(_bits(out), _bits(v))
    return float(v.detach()), x.grad, *_tables(wk, B, N, M), wk


def _same_decisions(case, name, r64, nnx, nny, win):
    assert np.array_equal(nnx, r64["nnx"]), (case, name, "x-side table", np.argwhere(nnx != r64["nnx"])[:5].tolist())
    assert np.array_equal(nny, r64["nny"]), (case, name, "y-side table", np.argwhere(nny != r64["nny"])[:5].tolist())
    assert win == r64["win"], (case, name, win, r64["win"])


# ------------------------------------------------------------------------------------------------ 1. where the loops end
@pytest.mark.parametrize("shape", E.BOUNDARY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loop_ends_against_float64(dev, shape):
    xn, yn, seed = E.boundary_case(*shape)
    case = "%dx%dx%d seed %d" % (*shape, seed)
    for name in ("chamfer", "hausdorff"):
        r64, r32 = (E.set_rule(xn, yn, dt, name, grad_out=3.0) for dt in (np.float64, np.float32))
        v, g, nnx, nny, win, _ = _run(dev, xn, yn, name)
        _same_decisions(case, name, r64, nnx, nny, win)
        _check("k_set_final " + name, case, v, r64["value"], r32["value"], VALUE_FIXED)
        _check("k_set_grad " + name, case, g.cpu().numpy(), r64["grad"], r32["grad"], GRAD_FIXED)


# ------------------------------------------------------------------------------------------------ 2. exact ties
@pytest.mark.parametrize("kind", E.TIE_KINDS)
def test_exact_ties_follow_the_documented_rule(dev, kind):
    c = E.tie_case(kind)
    xn, yn = c["x"], c["y"]
    for name in ("chamfer", "hausdorff"):
        r64, r32 = (E.set_rule(xn, yn, dt, name, grad_out=3.0) for dt in (np.float64, np.float32))
        v, g, nnx, nny, win, wk = _run(dev, xn, yn, name)
        _same_decisions("tie " + kind, name, r64, nnx, nny, win)
        _check("k_set_final " + name, "tie " + kind, v, r64["value"], r32["value"], VALUE_FIXED)
        _check("k_set_grad " + name, "tie " + kind, g.cpu().numpy(), r64["grad"], r32["grad"], GRAD_FIXED)
        if c["expect"].get("zero_grad"):
            assert v == 0.0 and torch.count_nonzero(g) == 0
        # the backward that is handed the forward's tables and the one that searches again write the same bits
        x, y = _t(xn, dev), _t(yn, dev)
        rc1, g1 = _backward_raw(dev, x, y, KIND[name], 3.0, wk)
        rc2, g2 = _backward_raw(dev, x, y, KIND[name], 3.0, None)
        assert rc1 == 0 and rc2 == 0 and torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(g1), _bits(g))
    # the planted decisions themselves (the Hausdorff run's tables)
    for b, i, j in c["expect"].get("nnx", []):
        assert nnx[b, i] == j
    for b, j, i in c["expect"].get("nny", []):
        assert nny[b, j] == i
    for k, w in c["expect"].get("win", []):
        assert win[k] == w


# ------------------------------------------------------------------------------------------------ 3. non-finite coordinates
@pytest.mark.parametrize("kind", E.NONFINITE_KINDS)
def test_non_finite_coordinates_propagate_as_documented(dev, kind):
    c = E.nonfinite_case(kind)
    xn, yn = c["x"], c["y"]
    case = "nonfinite " + kind
    for name in ("chamfer", "hausdorff"):
        r64, r32 = (E.set_rule(xn, yn, dt, name) for dt in (np.float64, np.float32))
        rc, out, wk = _raw(dev, _t(xn, dev), _t(yn, dev), kind=KIND[name])
        nnx, nny, win = _tables(wk, 3, 9, 7)
        print(f"{case} {name}: value {float(out)} rule {r32['value']}; winners {win} rule {r64['win']}")
        assert rc == 0 and E.same_float(float(out), r32["value"]) and not np.isfinite(float(out))
        assert np.isnan(float(out)) == (kind != "inf_x")
        _same_decisions(case, name, r64, nnx, nny, win)
    # the Chamfer gradient
    r64, r32 = (E.set_rule(xn, yn, dt, "chamfer", grad_out=3.0) for dt in (np.float64, np.float32))
    _, g, *_ = _run(dev, xn, yn, "chamfer")
    _, g_clean, *_ = _run(dev, c["x0"], c["y0"], "chamfer")
    good = [b for b in range(3) if b not in c["bad"]]
    assert torch.equal(_bits(g[good]), _bits(g_clean[good]))                  # a clean graph keeps the clean run's bits
    gn = g.cpu().numpy()
    for b, i in c["nan_rows"]:
        assert np.isnan(gn[b, i]).all(), (case, b, i, gn[b, i])              # the row of a NaN x point is NaN
    # the other rows of the graph: what the rule gives - its NaN pattern, and its numbers where it has numbers
    assert np.array_equal(np.isnan(gn), np.isnan(r64["grad"])), (case, np.argwhere(np.isnan(gn) != np.isnan(r64["grad"])).tolist())
    fin = np.isfinite(r64["grad"])
    _check("k_set_grad chamfer", case, gn[fin], r64["grad"][fin], r32["grad"][fin], GRAD_FIXED)


# ------------------------------------------------------------------------------------------------ 4. the LDS limit
def test_the_lds_limit_and_one_point_past_it(dev):
    """The largest accepted size: N + M == chamfer_max_points() (13,480: the host check that ag_set_loss shares with the planner's
    Chamfer; 6739 + 6741).  The value against the chunked float64 rule for both kinds; no gradient bar at this size - among 13k points
    gaps below 1e-5 are expected - and table entries only where the float64 gap exceeds 1e-4.  One point more (and 6739 + 6743, what
    the kernel's own 3 (N + M) floats of LDS would still hold) is refused with nothing written."""
    from adaptigraph_amd import _lib
    B, N = E.LDS_SHAPE
    M = CR.CHAMFER_MAX_POINTS - N
    assert N + M == CR.CHAMFER_MAX_POINTS and (N, M) == (6739, 6741)
    xn, yn = E.lds_case(M)
    r64 = E.set_rule(xn, yn, np.float64, want_gaps=True)
    r32 = E.set_rule(xn, yn, np.float32)
    x, y = _t(xn, dev), _t(yn, dev)
    for name in ("chamfer", "hausdorff"):
        rc, out, wk = _raw(dev, x, y, kind=KIND[name])
        assert rc == 0
        _check("k_set_final " + name, f"{B}x{N}x{M} (LDS limit)", float(out), r64["values"][name], r32["values"][name], VALUE_FIXED)
        nnx, nny, _ = _tables(wk, B, N, M)
        sure_x, sure_y = r64["gx"] > E.GAP_BAR, r64["gy"] > E.GAP_BAR
        print(f"  tables compared at {sure_x.mean():.4f} of the x points and {sure_y.mean():.4f} of the y points")
        assert sure_x.mean() > 0.99 and sure_y.mean() > 0.99
        assert np.array_equal(nnx[sure_x], r64["nnx"][sure_x]) and np.array_equal(nny[sure_y], r64["nny"][sure_y])
    for more_n, more_m in ((1, 0), (0, 1), (0, 2)):
        xb, yb = torch.zeros((B, N + more_n, 3), device=dev), torch.zeros((B, M + more_m, 3), device=dev)
        for name in ("chamfer", "hausdorff"):
            rc, out, wk = _raw(dev, xb, yb, kind=KIND[name])
            assert rc == _lib.AG_ERR_UNSUPPORTED and float(out) == -7.0 and bool((wk == -7).all())
            rc, g = _backward_raw(dev, xb, yb, KIND[name], 1.0, None)
            assert rc == _lib.AG_ERR_UNSUPPORTED and bool((g == -7.0).all())
        with pytest.raises(NotImplementedError, match="exceeds the set-loss LDS tile"):
            _module("chamfer")(xb, yb)


# ------------------------------------------------------------------------------------------------ 5. parts
def test_chamfer_parts_are_their_share_and_hausdorff_refuses(dev):
    from adaptigraph_amd import _lib
    Bt, N, M = E.PARTS
    xn, yn, seed = E.boundary_case(Bt, N, M)
    x, y = _t(xn, dev), _t(yn, dev)
    rc, whole, wk = _raw(dev, x, y, kind=1)
    rc_g, g_whole = _backward_raw(dev, x, y, 1, 3.0, wk)
    assert rc == 0 and rc_g == 0
    total, rows = 0.0, []
    for s in E.PART_SLICES:
        xs, ys = x[s].contiguous(), y[s].contiguous()
        r64, r32 = (E.set_rule(xn[s], yn[s], dt, "chamfer", grad_out=3.0, B_total=Bt) for dt in (np.float64, np.float32))
        rc, out, wk_p = _raw(dev, xs, ys, kind=1, B_total=Bt)
        assert rc == 0
        _check("k_set_final chamfer", f"part {s.start}:{s.stop} of {Bt}x{N}x{M} seed {seed}", float(out), r64["value"], r32["value"], VALUE_FIXED)
        for work in (wk_p, None):
            rc, g = _backward_raw(dev, xs, ys, 1, 3.0, work, B_total=Bt)
            assert rc == 0 and torch.equal(_bits(g), _bits(g_whole[s]))          # bit for bit the rows of the whole's
        total += float(out)
        rows.append(g)
    print("whole", float(whole), "parts sum", total)
    assert abs(total - float(whole)) <= 1e-6 * abs(float(whole))
    _check("k_set_grad chamfer", f"parts of {Bt}x{N}x{M}", torch.cat(rows).cpu().numpy(),
           *(E.set_rule(xn, yn, dt, "chamfer", grad_out=3.0)["grad"] for dt in (np.float64, np.float32)), GRAD_FIXED)
    s = E.PART_SLICES[0]
    rc, out, wk = _raw(dev, x[s].contiguous(), y[s].contiguous(), kind=2, B_total=Bt)
    assert rc == _lib.AG_ERR_UNSUPPORTED and float(out) == -7.0 and bool((wk == -7).all())
    rc, g = _backward_raw(dev, x[s].contiguous(), y[s].contiguous(), 2, 3.0, None, B_total=Bt)
    assert rc == _lib.AG_ERR_UNSUPPORTED and bool((g == -7.0).all())


# ------------------------------------------------------------------------------------------------ 6. the fused step
@functools.lru_cache(maxsize=None)
def _fused():
    bt = E.fused_batch(E.FUSED_SEED)
    W = TR.make_weights(5, E.FUSED["n_his"])
    g64, st64 = E.fused_restate(bt, W, torch.float64, "cuda:0")
    g32, st32 = E.fused_restate(bt, W, torch.float32, "cuda:0")
    return bt, W, g64, st64, g32, st32


def _fused_step(dev, bt, W, fut):
    import adaptigraph_amd as ag
    c = E.FUSED
    model = _model(dev, W, n_his=c["n_his"], pstep=c["pstep"])
    edges = _edge_list(bt["recv_l"], bt["send_l"], c["N"], dev)
    data = dict(state=_t(bt["state"], dev), attrs=_t(bt["attrs"], dev), p_instance=_t(bt["p_instance"], dev), action=_t(bt["action"], dev),
                edges=edges, phys_physics_param=_t(bt["phys"], dev), state_future=_t(fut, dev), eef_future=_t(bt["eef_future"], dev),
                action_future=_t(bt["action_future"], dev))
    ts = ag.TrainStep(model, lr=0.0, n_future=c["n_future"], losses=E.FUSED_LOSSES)
    loss = ts.step(data, max_edges=c["per_recv"] * c["N"])
    ts.check()
    torch.cuda.synchronize()
    return ts, loss


def test_fused_step_with_all_three_terms_at_n_p_257(dev):
    """k_set_nn on strided labels, k_step_loss_final, and k_set_grad with both weights adding into the chain's dpos, N = M = 257."""
    bt, W, g64, st64, g32, st32 = _fused()
    ts, loss = _fused_step(dev, bt, W, bt["state_future"])
    terms = ts.last_loss_terms.cpu().double().numpy()
    print("seed", E.FUSED_SEED, "loss_sum", float(loss), "float64", st64["loss"], "terms", terms.tolist(), "float64", st64["terms"].tolist())
    bad = []
    for fi in range(E.FUSED["n_future"]):
        for k, (name, _) in enumerate(E.FUSED_LOSSES):
            err, err32, ref = abs(terms[fi, k] - st64["terms"][fi, k]), abs(st32["terms"][fi, k] - st64["terms"][fi, k]), st64["terms"][fi, k]
            print(f"RATIO k_step_loss_final {name} step {fi}: err {err:.3e} fp32-restatement {err32:.3e} max|ref| {abs(ref):.3e} "
                  f"ratio {E.ratio(err, err32, abs(ref)):.2f} bar {BS.bar(np.array([ref]), err32):.3e}")
            if not err <= BS.bar(np.array([ref]), err32):
                bad.append((name, fi, err))
    for k, t in zip(TR.KEYS, ts.grad):
        ref = g64[k]
        assert np.abs(ref).max() > 0, k
        err, err32 = np.abs(t.double().cpu().numpy() - ref).max(), np.abs(g32[k] - ref).max()
        lim = BS.bar(ref, err32)
        print(f"RATIO fused {k}: err {err:.3e} fp32-restatement {err32:.3e} max|ref| {np.abs(ref).max():.3e} "
              f"ratio {E.ratio(err, err32, np.abs(ref).max()):.2f} bar {lim:.3e}")
        if not err <= lim:
            bad.append((k, float(err), float(err32)))
    assert not bad, bad


def test_fused_step_with_a_nan_label_at_step_1(dev):
    bt, W, *_ = _fused()
    clean, loss_clean = _fused_step(dev, bt, W, bt["state_future"])
    fut = bt["state_future"].copy()
    fut[1, 1, 4, 1] = np.nan
    ts, loss = _fused_step(dev, bt, W, fut)                                       # the call returns, check() included
    terms, terms_clean = ts.last_loss_terms, clean.last_loss_terms
    print("clean", terms_clean.tolist(), float(loss_clean), "NaN label at step 1", terms.tolist(), float(loss))
    assert bool(torch.isfinite(terms_clean).all()) and np.isfinite(float(loss_clean))
    assert torch.equal(_bits(terms[0]), _bits(terms_clean[0]))                     # step 0 never reads step 1's label
    assert torch.equal(_bits(ts._loss[:1]), _bits(clean._loss[:1]))
    assert bool(torch.isnan(terms[1, 1:]).all()) and np.isnan(float(loss)) and bool(torch.isnan(ts._loss[1:]).all())
