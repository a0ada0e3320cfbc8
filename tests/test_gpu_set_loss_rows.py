"""The training set losses over each graph's real rows (-m gpu): AG_LOSS_ROWS through ChamferLoss, HausdorffLoss, EarthMoverLoss,
earth_mover_assignment, the raw boundary and TrainStep(real_rows=True).  k_set_nn<true>, k_set_grad<true>, k_emd_assign<.., true>,
k_emd_grad<true>, the finalisers' ROWS branches and k_prefix_rows.

Yardstick: tests/set_loss_rows.py::rows_rule in float64 on the same fp32 inputs (held against the reference's recordings of the
sliced graphs, the plain rule at full counts and its own mutants by tests/test_set_loss_rows.py).  Measure and bar are those of
tests/test_gpu_set_loss_edges.py, restated here: err <= min(4 err32 + 1e-7 max|ref|, fixed), err32 = the same rule in fp32 on the
CPU, fixed = value 1e-5 relative, gradient 1e-4 max|g_ref| + 1e-7; every case prints RATIO = err / (err32 + 0.25e-7 max|ref|), the
quantity the bar holds to 4 (DESIGN.md section 3.22 records the largest seen).  Tables, winners and matches are integers and
compared as such: every case is built so that the float64 gaps exceed GAP_BAR (set_loss_rows.qualifies).  Every test here fails
on the parent commit, which has neither the flag nor the count arguments."""
import functools
import os

import numpy as np
import pytest
import torch

import set_loss_edges as SE
import set_loss_rows as RW
import train_restate as TR
from test_train import grad_tol
from test_gpu_train import _model, _fixture_edges, _graph
from test_gpu_train_step import _data, _train_step, _max_edges, _t

pytestmark = pytest.mark.gpu

KIND = {"chamfer": 1, "hausdorff": 2, "earth_mover": 3}
ROWS = 16
VALUE_FIXED = lambda scale: 1e-5 * scale             # noqa: E731
GRAD_FIXED = lambda scale: 1e-4 * scale + 1e-7       # noqa: E731
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _i32(a, dev):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(dev)


def _check(kernel, case, got, ref64, ref32, fixed):
    """tests/test_gpu_set_loss_edges.py::_check, restated"""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape and np.isfinite(ref64).all() and np.isfinite(got).all(), (kernel, case)
    err, err32, scale = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max()), float(np.abs(ref64).max())
    print(f"RATIO {kernel} {case}: err {err:.3e} fp32-restatement {err32:.3e} max|ref| {scale:.3e} ratio {SE.ratio(err, err32, scale):.2f}")
    assert err <= min(4 * err32 + 1e-7 * scale, fixed(scale)), (kernel, case, err, err32)


def _module(name):
    import adaptigraph_amd as ag
    return {"chamfer": ag.ChamferLoss, "hausdorff": ag.HausdorffLoss, "earth_mover": ag.EarthMoverLoss}[name]()


def _raw(dev, x, y, nx, ny, kind, B_total=None, work=True):
    """ag_set_loss with kind | AG_LOSS_ROWS at the boundary: (return code, out, work); the counts are the work buffer's last 2B words"""
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import ptr, current_stream
    eng = ag.default_engine(dev)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    out = torch.full((), -7.0, device=dev)
    wk = torch.full((B * (N + M) + 4 + 2 * B,), -7, device=dev, dtype=torch.int32)
    wk[B * (N + M) + 4:] = torch.cat([_i32(nx, dev), _i32(ny, dev)])
    rc = eng.lib.ag_set_loss(eng.ctx, current_stream(dev), ptr(x), ptr(y), B, N, M, B if B_total is None else B_total, kind | ROWS,
                             ptr(out), ptr(wk) if work else None)
    torch.cuda.synchronize()
    return rc, out, wk


def _backward_raw(dev, x, y, kind, go, wk, B_total=None):
    import adaptigraph_amd as ag
    from adaptigraph_amd.context import ptr, current_stream
    eng = ag.default_engine(dev)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    g = torch.full_like(x, -7.0)
    got = torch.full((1,), float(go), device=dev)
    rc = eng.lib.ag_set_loss_backward(eng.ctx, current_stream(dev), ptr(x), ptr(y), B, N, M, B if B_total is None else B_total,
                                      kind | ROWS, ptr(got), ptr(g), None if wk is None else ptr(wk))
    torch.cuda.synchronize()
    return rc, g


def _tables(wk, B, N, M):
    """-> dict(nnx, nny, win) of a Chamfer / Hausdorff buffer, dict(match, status) read the Earth-mover way"""
    t = wk[:B * (N + M)].view(B, N + M).cpu().numpy()
    return dict(nnx=t[:, :N], nny=t[:, N:], win=wk[B * (N + M):B * (N + M) + 4].cpu().tolist(),
                match=wk[:B * N].view(B, N).cpu().numpy(), status=wk[B * N:B * N + B].cpu().numpy())


def _run(dev, xn, yn, nx, ny, name, grad_out=3.0):
    """module forward and backward with counts, and the boundary's buffer -> (value, gradient tensor, tables, value tensor)"""
    B, N, M = xn.shape[0], xn.shape[1], yn.shape[1]
    x, y = _t(xn, dev).requires_grad_(True), _t(yn, dev)
    v = _module(name)(x, y, _i32(nx, dev), _i32(ny, dev))
    assert v.dim() == 0 and v.is_cuda
    (grad_out * v).backward()
    rc, out, wk = _raw(dev, x.detach(), y, nx, ny, KIND[name])
    assert rc == 0 and torch.equal(_bits(out), _bits(v))
    rc, g = _backward_raw(dev, x.detach(), y, KIND[name], grad_out, wk)
    assert rc == 0 and torch.equal(_bits(g), _bits(x.grad))                   # the boundary's backward is the module's
    return float(v.detach()), x.grad, _tables(wk, B, N, M), v.detach()


def _against_rule(dev, case, xn, yn, nx, ny, names=RW.KINDS):
    """every kind of a qualifying case: decisions exact, value and gradient inside the bar; padding rows exact zeros"""
    import adaptigraph_amd as ag
    N = xn.shape[1]
    out = {}
    for name in names:
        r64, r32 = (RW.rows_rule(xn, yn, nx, ny, dt, name, grad_out=3.0) for dt in (np.float64, np.float32))
        v, g, tb, vt = _run(dev, xn, yn, nx, ny, name)
        gn = g.cpu().numpy()
        if name == "earth_mover":
            assert np.array_equal(tb["match"], r64["match"]), (case, "match")
            assert not tb["status"].any()
            i1, i2 = ag.earth_mover_assignment(_t(xn, dev), _t(yn, dev), _i32(nx, dev), _i32(ny, dev))
            assert np.array_equal(i1.cpu().numpy(), r64["ind1"]) and np.array_equal(i2.cpu().numpy(), r64["ind2"]), (case, "assignment")
            kernels = ("k_emd_assign", "k_emd_grad")
        else:
            assert np.array_equal(tb["nnx"], r64["nnx"]) and np.array_equal(tb["nny"], r64["nny"]), (case, name, "tables")
            if name == "hausdorff":
                assert tb["win"] == r64["win"], (case, tb["win"], r64["win"])
            kernels = ("k_set_final " + name, "k_set_grad " + name)
        _check(kernels[0], case, v, r64["value"], r32["value"], VALUE_FIXED)
        _check(kernels[1], case, gn, r64["grad"], r32["grad"], GRAD_FIXED)
        for b in range(len(xn)):
            assert (gn[b, r64["nx"][b]:] == 0).all(), (case, name, b)
        out[name] = (vt, g, tb)
    return out


# ------------------------------------------------------------------------------------------------ 1. fixture and rule
def _fixture(tag):
    f = np.load(os.path.join(HERE, "golden", "set_losses_rows.npz"))
    return {k.split("::", 1)[1]: f[k] for k in f.files if k.startswith(tag + "::")}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_modules_against_the_fixture_and_the_rule(dev, tag):
    c = _fixture(tag)
    got = _against_rule(dev, "fixture " + tag, c["x"], c["y"], c["nx"], c["ny"])
    B, rec = len(c["nx"]), c["recorded"]
    # the reference's own numbers: the mean over graphs of its modules on the slices (an empty graph adds 0 and counts in B)
    for name, key in (("chamfer", "chamfer"), ("earth_mover", "emd")):
        v, g, _ = got[name]
        ref, g_ref = float(c[key][rec].astype(np.float64).sum() / B), 3.0 * c["g_" + key] / B
        err = np.abs(g.cpu().numpy() - g_ref).max()
        print(f"fixture {tag} {name}: {float(v):.8g} reference {ref:.8g}; gradient error {err:.3e}, max|g_ref| {np.abs(g_ref).max():.3e}")
        assert abs(float(v) - ref) <= 1e-5 * abs(ref) and err <= 1e-4 * np.abs(g_ref).max() + 1e-7
    assert abs(float(got["chamfer"][0]) - c["mean_chamfer"][rec].sum() / B) <= 1e-5 * float(got["chamfer"][0])
    # Hausdorff graph by graph (a batch of one is the reference's module on the slice)
    for b in np.nonzero(rec)[0]:
        x = _t(c["x"][b:b + 1], dev).requires_grad_(True)
        v = _module("hausdorff")(x, _t(c["y"][b:b + 1], dev), _i32(c["nx"][b:b + 1], dev), _i32(c["ny"][b:b + 1], dev))
        v.backward()
        assert abs(float(v.detach()) - float(c["hausdorff"][b])) <= 1e-5 * float(c["hausdorff"][b])
        assert np.abs(x.grad[0].cpu().numpy() - c["g_hausdorff"][b]).max() <= 1e-4 * np.abs(c["g_hausdorff"][b]).max() + 1e-7


# ------------------------------------------------------------------------------------------------ 2. shapes
SHAPES = {
    "1x1x1": (1, 1, 1, [1], [1]),
    "strides 255 256 257 in 600": (3, 300, 300, [100, 156, 200], [155, 100, 57]),      # nx + ny; nx < ny and nx > ny
    "K_b = 1": (2, 5, 4, [1, 5], [4, 1]),
    "empty first middle last": (5, 6, 5, [0, 3, 6, 4, 2], [3, 5, 0, 4, 0]),
}
# (the third graph of the last case is empty through its y side alone; the first through x, the last through y)


@functools.lru_cache(maxsize=None)
def _shape_case(name):
    B, N, M, nx, ny = SHAPES[name]
    x, y, seed = RW.case(B, N, M, nx, ny)
    return x, y, np.array(nx), np.array(ny), seed


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_against_float64(dev, name):
    x, y, nx, ny, seed = _shape_case(name)
    _against_rule(dev, f"{name} seed {seed}", x, y, nx, ny)


def test_all_graphs_empty(dev):
    x, y = RW.cloud(3, 3, 6, 5)
    for name in RW.KINDS:
        v, g, tb, _ = _run(dev, x, y, [0, 4, 0], [3, 0, 0], name)
        assert v == 0.0 and bool((g == 0).all())
        if name == "earth_mover":
            assert (tb["match"] == -1).all() and not tb["status"].any()
        else:
            assert not tb["nnx"].any() and not tb["nny"].any() and tb["win"] == [-1, -1, -1, -1]


def test_counts_out_of_range_give_the_clamped_bits(dev):
    x, y, nx, ny, _ = _shape_case("empty first middle last")
    wild_x, wild_y = np.array([-4, 3, 600, 4, 2]), np.array([3, 2 ** 30, -1, 4, -(2 ** 31)])
    assert np.array_equal(np.clip(wild_x, 0, 6), nx) and np.array_equal(np.clip(wild_y, 0, 5), ny)
    for name in RW.KINDS:
        v0, g0, t0, _ = _run(dev, x, y, nx, ny, name)
        v1, g1, t1, _ = _run(dev, x, y, wild_x, wild_y, name)
        assert np.float32(v0).tobytes() == np.float32(v1).tobytes() and torch.equal(_bits(g0), _bits(g1))
        assert all(np.array_equal(t0[k], t1[k]) for k in ("nnx", "nny", "match")) and t0["win"] == t1["win"]
    # one side given: the other is full
    full = _module("chamfer")(_t(x, dev), _t(y, dev), None, _i32([5] * 5, dev))
    both = _module("chamfer")(_t(x, dev), _t(y, dev), _i32([6] * 5, dev), _i32([5] * 5, dev))
    assert torch.equal(_bits(full), _bits(both))


# ------------------------------------------------------------------------------------------------ 3. padding is inert
def test_padding_is_inert_and_runs_repeat(dev):
    c = _fixture("a")
    for name in RW.KINDS:
        v0, g0, t0, _ = _run(dev, c["x"], c["y"], c["nx"], c["ny"], name)
        for fill in (np.nan, np.inf, 1e30, 0.0):                             # 0.0: the same run again gives the same bits
            x, y = RW.with_padding(c["x"], c["y"], c["nx"], c["ny"], fill)
            v, g, t, _ = _run(dev, x, y, c["nx"], c["ny"], name)
            assert np.float32(v).tobytes() == np.float32(v0).tobytes(), (name, fill, v, v0)
            assert torch.equal(_bits(g), _bits(g0)), (name, fill)
            assert all(np.array_equal(t[k], t0[k]) for k in ("nnx", "nny", "match")) and t["win"] == t0["win"], (name, fill)
            gn = g.cpu().numpy()
            for b in range(len(x)):
                n = 0 if c["ny"][b] == 0 else c["nx"][b]
                assert (gn[b, n:] == 0).all(), (name, fill, b)


# ------------------------------------------------------------------------------------------------ 4. Hausdorff
def test_hausdorff_padding_cannot_win_and_ties_take_the_lowest(dev):
    import adaptigraph_amd as ag
    c = _fixture("a")
    x, y, nx, ny = c["x"].copy(), c["y"].copy(), c["nx"], c["ny"]
    x[1, 7] = SE.FAR_P                                                        # nx[1] = 5: a padding row that would win the plain max
    y[2, 5] = SE.FAR_R                                                        # ny[2] = 2: likewise on the y side
    plain = float(ag.HausdorffLoss()(_t(x, dev), _t(y, dev)))
    v, g, tb, _ = _run(dev, x, y, nx, ny, "hausdorff")
    v0, g0, tb0, _ = _run(dev, c["x"], c["y"], nx, ny, "hausdorff")
    print("plain", plain, "rows", v, "rows without the far padding", v0, "winners", tb["win"])
    assert plain > 20 and v == v0 and tb["win"] == tb0["win"] and torch.equal(_bits(g), _bits(g0))
    # equal real maxima: the same far pair in graphs 4 (y side empty: no candidate), 1 and 5 - the lowest real (b, i) wins
    x, y = c["x"].copy(), c["y"].copy()
    for b, i, j in ((4, 0, 0), (1, 3, 2), (5, 1, 2), (1, 4, 6)):
        x[b, i], y[b, j] = SE.FAR_P, SE.FAR_Q
    v, g, tb, _ = _run(dev, x, y, nx, ny, "hausdorff")
    r64 = RW.rows_rule(x, y, nx, ny, np.float64, "hausdorff", grad_out=3.0)
    assert tb["win"] == r64["win"] and tb["win"][:2] == [1, 3] and tb["win"][2] == 1, tb["win"]
    gn = g.cpu().numpy()
    assert np.abs(gn[1, 3]).max() > 0 and not gn[4].any() and not gn[5].any() and not gn[1, 4].any()


@pytest.mark.parametrize("shape", [(3, 7, 5), (2, 257, 300)], ids=lambda s: "x".join(map(str, s)))
def test_hausdorff_full_counts_are_kind_2_bits(dev, shape):
    import adaptigraph_amd as ag
    B, N, M = shape
    xn, yn = RW.cloud(11, B, N, M)
    x0, x1, y = _t(xn, dev).requires_grad_(True), _t(xn, dev).requires_grad_(True), _t(yn, dev)
    a = ag.HausdorffLoss()(x0, y)
    b = ag.HausdorffLoss()(x1, y, _i32([N] * B, dev), _i32([M] * B, dev))
    a.backward()
    b.backward()
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(x0.grad), _bits(x1.grad))
    # Chamfer and Earth-mover at full counts: the plain kinds up to the last place (the division happens per graph)
    for mod in (ag.ChamferLoss(), ag.EarthMoverLoss()):
        p, r = float(mod(x0.detach(), y)), float(mod(x0.detach(), y, _i32([N] * B, dev), _i32([M] * B, dev)))
        assert abs(p - r) <= float(np.spacing(np.float32(abs(p)))), (type(mod).__name__, p, r)   # one fp32 place: both round one fp64 sum


# ------------------------------------------------------------------------------------------------ 5. parts
def test_chamfer_and_earth_mover_parts_add_up_and_hausdorff_refuses(dev):
    from adaptigraph_amd import _lib
    c = _fixture("a")
    xn, yn, nx, ny = c["x"], c["y"], c["nx"], c["ny"]
    Bt = len(nx)
    x, y = _t(xn, dev), _t(yn, dev)
    for name in ("chamfer", "earth_mover"):
        rc, whole, wk = _raw(dev, x, y, nx, ny, KIND[name])
        rc_g, g_whole = _backward_raw(dev, x, y, KIND[name], 3.0, wk)
        assert rc == 0 and rc_g == 0
        total = 0.0
        for s in (slice(0, 4), slice(4, 6)):
            xs, ys = x[s].contiguous(), y[s].contiguous()
            r64, r32 = (RW.rows_rule(xn[s], yn[s], nx[s], ny[s], dt, name, grad_out=3.0, B_total=Bt) for dt in (np.float64, np.float32))
            rc, out, wk_p = _raw(dev, xs, ys, nx[s], ny[s], KIND[name], B_total=Bt)
            assert rc == 0
            _check("k_set_final " + name, f"part {s.start}:{s.stop} of fixture a", float(out), r64["value"], r32["value"], VALUE_FIXED)
            rc, g = _backward_raw(dev, xs, ys, KIND[name], 3.0, wk_p, B_total=Bt)
            assert rc == 0 and torch.equal(_bits(g), _bits(g_whole[s]))       # bit for bit the rows of the whole's
            total += float(out)
        print(name, "whole", float(whole), "parts sum", total)
        assert abs(total - float(whole)) <= 1e-6 * abs(float(whole))
    s = slice(0, 4)
    rc, out, wk = _raw(dev, x[s].contiguous(), y[s].contiguous(), nx[s], ny[s], 2, B_total=Bt)
    assert rc == _lib.AG_ERR_UNSUPPORTED and float(out) == -7.0 and bool((wk[:4 * 16 + 4] == -7).all())
    rc, g = _backward_raw(dev, x[s].contiguous(), y[s].contiguous(), 2, 3.0, wk, B_total=Bt)
    assert rc == _lib.AG_ERR_UNSUPPORTED and bool((g == -7.0).all())


# ------------------------------------------------------------------------------------------------ 6. non-finite in a real row
def test_non_finite_in_a_real_row(dev):
    c = _fixture("a")
    x0, y, nx, ny = c["x"], c["y"], c["nx"], c["ny"]
    x = x0.copy()
    x[1, 2, 1] = np.nan                                                       # nx[1] = 5: a real row
    good = [0, 2, 3, 4, 5]
    for name in RW.KINDS:
        v0, g0, _, _ = _run(dev, x0, y, nx, ny, name)
        v, g, tb, _ = _run(dev, x, y, nx, ny, name)
        gn = g.cpu().numpy()
        assert np.isfinite(v0) and np.isnan(v), (name, v)
        assert np.isnan(gn[1, 2]).all() and (gn[1, 5:] == 0).all(), name
        if name == "hausdorff":                                               # both winners move to the NaN row: nothing is left elsewhere
            assert tb["win"][0] == 1 and tb["win"][2] == 1 and not gn[good].any()
        else:                                                                 # the other graphs keep the clean run's bits
            assert torch.equal(_bits(g[good]), _bits(g0[good])), name
        r64 = RW.rows_rule(x, y, nx, ny, np.float64, name, grad_out=3.0)
        assert np.array_equal(np.isnan(gn), np.isnan(r64["grad"])), name
        if name == "earth_mover":                                             # the graph fails alone
            assert tb["status"].tolist() == [0, 1, 0, 0, 0, 0] and (tb["match"][1] == -1).all() and np.isnan(gn[1, :5]).all()
            assert np.array_equal(tb["match"][good], RW.rows_rule(x0, y, nx, ny, kind=name)["match"][good])


# ------------------------------------------------------------------------------------------------ 7. the fused step
LIVE = [40, 23, 1]
N_FUTURE = 2


@functools.lru_cache(maxsize=None)
def _padded_fixture():
    """train_losses_rope.npz (B = 3, n_p = 40) as a padded batch: graph b's live rows are its first LIVE[b]; attrs[b, i, 0] = 0 and
    state_future zero behind them, as the device data set writes padding"""
    f = TR.load_fixture("train_losses_rope.npz")
    f = {k: np.array(f[k]) for k in f.keys()}
    n_p = f["p_instance"].shape[1]
    assert n_p == 40 and f["attrs"].shape[0] == 3
    for b, n in enumerate(LIVE):
        f["attrs"][b, n:n_p, 0] = 0
        f["state_future"][b, :, n:] = 0
    f["n_future"] = np.int32(N_FUTURE)
    return f


def _rows_modules(counts):
    import adaptigraph_amd as ag
    wrap = lambda m: (lambda p, g: m(p, g, counts, counts))   # noqa: E731
    return {"mse": torch.nn.MSELoss(), "chamfer": wrap(ag.ChamferLoss()), "hausdorff": wrap(ag.HausdorffLoss()),
            "earth_mover": wrap(ag.EarthMoverLoss())}


def _autograd_chain(model, f, dev, names_weights, counts):
    """tests/test_gpu_set_losses.py::_autograd_chain with the new modules fed by prefix_counts -> (loss_sum, terms (n_future, k))"""
    mods = _rows_modules(counts)
    edges = _fixture_edges(f, dev)
    state, action = _t(f["state"], dev), _t(f["action"], dev)
    fut, eef, act_f = _t(f["state_future"], dev), _t(f["eef_future"], dev), _t(f["action_future"], dev)
    n_p = f["p_instance"].shape[1]
    loss_sum, table = 0, []
    for fi in range(N_FUTURE):
        gt = fut[:, fi].clone()
        pred, _ = model(**_graph(f, dev, state=state, action=action, edges=edges))
        pred_p = pred[:, :gt.shape[1], :3].clone()
        vals = [mods[n](pred_p, gt) for n, _ in names_weights]
        loss_sum = loss_sum + sum([w * v for (_, w), v in zip(names_weights, vals)])
        table.append([float(v.detach()) for v in vals])
        if fi < N_FUTURE - 1:
            nxt = eef[:, fi].clone().unsqueeze(1)
            nxt[:, -1, :n_p] = pred_p
            state = torch.cat([state[:, 1:], nxt], 1)
            action = act_f[:, fi]
    return loss_sum, np.array(table)


FUSED_LISTS = {"mse chamfer hausdorff": [("mse", 1.0), ("chamfer", 0.5), ("hausdorff", 0.25)],
               "mse earth_mover": [("mse", 1.0), ("earth_mover", 0.5)]}


def _terms(names_weights):
    import adaptigraph_amd as ag
    return [((ag.EarthMoverLoss() if n == "earth_mover" else n), w) for n, w in names_weights]


@pytest.mark.parametrize("which", list(FUSED_LISTS))
def test_fused_step_equals_the_autograd_path(dev, which):
    """Bars restated from tests/test_gpu_set_losses.py::test_autograd_path_with_the_modules_equals_fused and its twin in
    tests/test_gpu_emd.py: |fused - autograd| <= 1e-5 |fused| for the loss (here also for every term), and for each of the 22
    weight gradients err <= 1e-4 max|g| + 1e-7."""
    import adaptigraph_amd as ag
    f, lst = _padded_fixture(), FUSED_LISTS[which]
    ts, _ = _train_step(dev, f, lr=0.0, losses=_terms(lst), real_rows=True, n_future=N_FUTURE)
    data = _data(f, dev)
    fused = float(ts.step(data, max_edges=_max_edges(data)))
    ts.check()
    counts = ag.prefix_counts(data["attrs"][:, :40, 0] > 0)
    assert counts.tolist() == LIVE and counts.dtype == torch.int32
    model = _model(dev, TR.fixture_weights(f), n_his=f["state"].shape[1], pstep=int(f["pstep"])).train()
    loss, table = _autograd_chain(model, f, dev, lst, counts)
    loss.backward()
    terms = ts.last_loss_terms.cpu().double().numpy()
    print("fused", fused, "autograd", loss.item(), "terms", terms.tolist(), "autograd", table.tolist())
    assert abs(fused - loss.item()) <= 1e-5 * abs(fused)
    assert terms.shape == table.shape and (np.abs(terms - table) <= 1e-5 * np.abs(table)).all()
    bad = []
    for k, p, g in zip(TR.KEYS, model.ordered_parameters(), ts.grad):
        ref = p.grad.detach()
        err, top = float((g - ref).abs().max()), float(ref.abs().max())
        print(f"  {k}: fused vs autograd {err:.3e}, max|g| {top:.3e}")
        if not err <= 1e-4 * top + 1e-7:
            bad.append((k, err, top))
    assert not bad, bad
    # the flag matters on this batch, and without it the step is the one it always was
    plain, _ = _train_step(dev, f, lr=0.0, losses=_terms(lst), n_future=N_FUTURE)
    off, _ = _train_step(dev, f, lr=0.0, losses=_terms(lst), real_rows=False, n_future=N_FUTURE)
    lp, lo = plain.step(data, max_edges=_max_edges(data)), off.step(data, max_edges=_max_edges(data))
    assert torch.equal(_bits(lp), _bits(lo)) and torch.equal(_bits(plain.last_loss_terms), _bits(off.last_loss_terms))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(plain.grad, off.grad))
    assert torch.equal(_bits(plain.last_loss_terms[:, 0]), _bits(ts.last_loss_terms[:, 0]))      # MSE runs over all rows either way
    assert not torch.equal(_bits(plain.last_loss_terms[:, 1]), _bits(ts.last_loss_terms[:, 1]))
    # evaluate gives the bits of step
    ev = ts.evaluate(data, max_edges=_max_edges(data))
    assert torch.equal(_bits(ev), _bits(torch.as_tensor(fused)))


def test_fused_two_parts_equal_one_step_and_hausdorff_refuses(dev):
    """bars of tests/test_gpu_set_losses.py::test_mse_chamfer_in_two_parts_equals_one_step, restated"""
    f = _padded_fixture()
    lst = [("mse", 1.0), ("chamfer", 0.5), ("earth_mover", 0.25)]
    whole, _ = _train_step(dev, f, lr=0.0, losses=_terms(lst), real_rows=True, n_future=N_FUTURE)
    data = _data(f, dev)
    l1 = float(whole.step(data, max_edges=_max_edges(data)))
    whole.check()
    parts, _ = _train_step(dev, f, lr=0.0, losses=_terms(lst), real_rows=True, n_future=N_FUTURE)
    for idx in ([0, 1], [2]):
        d = _data(f, dev, idx=idx)
        parts.accumulate(d, max_edges=_max_edges(d), total=3)
    l2 = float(parts.apply())
    parts.check()
    print("one step", l1, "two parts", l2, "terms", whole.last_loss_terms.tolist(), parts.last_loss_terms.tolist())
    assert abs(l1 - l2) <= 1e-6 * abs(l1)
    assert torch.allclose(whole.last_loss_terms, parts.last_loss_terms, rtol=1e-6, atol=0)
    bad = []
    for k, a, b in zip(TR.KEYS, whole.grad, parts.grad):
        err = float((a - b).abs().max())
        print(f"  {k}: parts vs whole {err:.3e} (bar {grad_tol(f, k):.3e})")
        if not err <= grad_tol(f, k):
            bad.append((k, err))
    assert not bad, bad
    hd, _ = _train_step(dev, f, lr=0.0, losses=[("mse", 1.0), ("hausdorff", 0.25)], real_rows=True, n_future=N_FUTURE)
    with pytest.raises(ValueError, match="does not split"):
        hd.accumulate(data, max_edges=_max_edges(data), total=6)


# ------------------------------------------------------------------------------------------------ 8. the raw boundary
def test_raw_boundary_refusals_enqueue_nothing(dev):
    import ctypes as C
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    from adaptigraph_amd.context import ptr, current_stream
    x, y = torch.zeros(2, 4, 3, device=dev), torch.zeros(2, 5, 3, device=dev)
    for kind in (1, 2, 3):
        rc, out, _ = _raw(dev, x, y, [4, 4], [5, 5], kind, work=False)        # a flagged kind needs d_work
        assert rc == _lib.AG_ERR_INVALID and float(out) == -7.0
        rc, g = _backward_raw(dev, x, y, kind, 1.0, None)
        assert rc == _lib.AG_ERR_INVALID and bool((g == -7.0).all())
    for kind in (_lib.AG_LOSS_MSE, 4, 8):                                     # AG_LOSS_MSE | AG_LOSS_ROWS and other non-kinds
        rc, out, wk = _raw(dev, x, y, [4, 4], [5, 5], kind)
        assert rc == _lib.AG_ERR_INVALID and float(out) == -7.0 and bool((wk[:2 * 9 + 4] == -7).all())
    # ag_train_step_losses: MSE | ROWS is no kind - TrainStep never builds it, so the spec is patched by hand
    f = _padded_fixture()
    ts, _ = _train_step(dev, f, lr=0.0, losses=[("mse", 1.0), ("chamfer", 0.5)], real_rows=True, n_future=N_FUTURE)
    assert list(ts._spec.kind)[:2] == [0, 1 | ROWS]
    ts._spec.kind[0] = _lib.AG_LOSS_MSE | _lib.AG_LOSS_ROWS
    data = _data(f, dev)
    with pytest.raises(Exception, match="unknown kind"):
        ts.step(data, max_edges=_max_edges(data))
    # host-side argument checks of the modules: before anything is enqueued
    mod = ag.ChamferLoss()
    with pytest.raises(AssertionError, match="shape"):
        mod(x, y, torch.zeros(3, dtype=torch.int32, device=dev), None)
    with pytest.raises(TypeError, match="integer"):
        mod(x, y, torch.zeros(2, device=dev), None)
    with pytest.raises(TypeError, match="integer"):
        mod(x, y, [4, 4], None)
    with pytest.raises(AssertionError, match="lives on"):
        mod(x, y, torch.zeros(2, dtype=torch.int32), None)
    assert ptr and current_stream and C
