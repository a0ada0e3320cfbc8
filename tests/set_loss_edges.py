"""The training set losses (csrc/ag_setloss.hip) where their fixtures never take them: exact ties, non-finite coordinates, the ends of
k_set_nn's 256-wide stride over N + M, the LDS limit, a part's share of a mean.  No GPU, no library: numpy only.

set_rule is a restatement of the RULE the kernel header documents, not of torch: distance sqrt((dx*dx + dy*dy) + dz*dz); the arg-min
is the first index of the smallest distance, a NaN taken at its first occurrence and kept; per-graph sums and maxima; the Hausdorff
winner is the lowest (b, index) among equals, the first NaN beating every number; chamfer = Sx / (B_total N) + Sy / (B_total M),
hausdorff = max_x + max_y; the gradient of x_i is its own nearest y, then every y_j whose arg-min is i in ascending j, zero at zero
distance (and NaN at a NaN distance, as torch's norm has it); the Hausdorff gradient goes to the two winning pairs alone.  In float64 it
is the yardstick, in float32 the error scale of the bar.  tests/test_set_loss_edges.py holds it against the reference's recordings,
against torch in float64, and against the MUTANTS below; tests/test_gpu_set_loss_edges.py holds the kernels against it.

One known difference from torch: torch.max() over the whole batch splits its gradient evenly among equal maxima, the rule gives the
whole weight to the lowest (b, index).  Only exact ties (duplicated points) show it."""
from __future__ import annotations

import numpy as np

MUTANTS = ("argmin_last", "max_last", "later_graph", "nan_min_ignored", "nan_max_ignored", "denominator_B", "pull_every_duplicate",
           "swap_NM")
BOUNDARY_SHAPES = [(1, 1, 1), (1, 1, 300), (1, 300, 1), (2, 100, 156), (2, 100, 157), (3, 255, 257), (2, 256, 256), (2, 257, 255),
                   (5, 3, 2), (300, 3, 2)]
TIE_KINDS = ("dup_y", "dup_x", "max_same_graph", "max_two_graphs", "both_graph0", "both_middle", "same_xi", "single_coincident")
NONFINITE_KINDS = ("nan_x", "nan_y", "inf_x", "inf_minus_inf", "all_nan_graph")
GAP_BAR = 1e-4
CHUNK_ELEMS = 1 << 16              # the (rows, M) block of distances held at once: half a MiB in float64, so it stays in cache


# ------------------------------------------------------------------------------------------------------------ the rule
def _dist(a, b):
    """a (n,3), b (m,3) -> (n,m), every operation rounded on its own in the arrays' dtype"""
    acc = None
    for k in range(3):
        d = a[:, None, k] - b[None, :, k]
        d *= d
        acc = d if acc is None else np.add(acc, d, out=acc)                 # (dx*dx + dy*dy) + dz*dz
    return np.sqrt(acc, out=acc)


def _nearest(a, b, mutant=None, want_gap=False):
    """For every row of a the nearest row of b: (distance, index[, gap to the second nearest]), chunked over a's rows."""
    n, m = len(a), len(b)
    rows = max(1, CHUNK_ELEMS // m)
    val, arg, gap = np.empty(n, a.dtype), np.empty(n, np.int64), np.full(n, np.inf)
    for i0 in range(0, n, rows):
        d = _dist(a[i0:i0 + rows], b)
        nan = np.isnan(d)
        fin = np.where(nan, np.inf, d)
        first = fin.argmin(1)                                            # all +inf: index 0
        if mutant == "argmin_last":
            first = m - 1 - fin[:, ::-1].argmin(1)
        if mutant != "nan_min_ignored":
            first = np.where(nan.any(1), nan.argmax(1), first)
            fin = d
        arg[i0:i0 + rows] = first
        val[i0:i0 + rows] = fin[np.arange(len(d)), first]
        if want_gap and m > 1:                                               # the smallest of the rest (d is this chunk's own)
            d[np.arange(len(d)), first] = np.inf
            gap[i0:i0 + rows] = d.min(1) - val[i0:i0 + rows]
    return (val, arg, gap) if want_gap else (val, arg)


def _argmax_first(v, mutant=None):
    """(value, index) of the largest entry: the lowest index among equals, the first NaN beating every number"""
    nan = np.isnan(v)
    if nan.any() and mutant != "nan_max_ignored":
        i = int(nan.argmax())
        return v[i], i
    w = np.where(nan, -np.inf, v)
    i = len(w) - 1 - int(w[::-1].argmax()) if mutant == "max_last" else int(w.argmax())
    return w[i], i


def _beats(ov, v, mutant):
    """does a later graph's maximum ov replace v?"""
    if mutant == "nan_max_ignored":
        return (not np.isnan(ov)) and (np.isnan(v) or ov > v)
    if np.isnan(ov):
        return not np.isnan(v)
    if np.isnan(v):
        return False
    return ov >= v if mutant == "later_graph" else ov > v


def _pull(xi, yj, s):
    """s * d|x_i - y_j| / dx_i, rows of (n,3) arrays; zero at zero distance, NaN at a NaN distance"""
    d = xi - yj
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    q = np.divide(s, dist, out=np.zeros_like(dist), where=dist != 0)
    return np.where((dist == 0)[:, None], 0, d * q[:, None]).astype(xi.dtype)


def set_rule(x, y, dtype=np.float64, kind="chamfer", grad_out=1.0, B_total=None, mutant=None, want_gaps=False):
    """x (B,N,3), y (B,M,3) -> dict(value, grad (B,N,3), nnx (B,N), nny (B,M), win [b, i, b, j]) of `kind` in `dtype` (values: both kinds'); with
    want_gaps also gx (B,N), gy (B,M): every point's gap between its nearest and second-nearest distance."""
    assert kind in ("chamfer", "hausdorff") and (mutant is None or mutant in MUTANTS)
    dt = np.dtype(dtype).type
    x, y = np.asarray(x).astype(dt), np.asarray(y).astype(dt)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    B_total = B if B_total is None else B_total
    den = B if mutant == "denominator_B" else B_total
    dN, dM = (M, N) if mutant == "swap_NM" else (N, M)
    nnx, nny = np.zeros((B, N), np.int64), np.zeros((B, M), np.int64)
    gx, gy = np.full((B, N), np.inf), np.full((B, M), np.inf)
    sx = sy = 0.0
    mx = my = None
    win = [0, 0, 0, 0]
    with np.errstate(all="ignore"):
        for b in range(B):
            rx, ry = _nearest(x[b], y[b], mutant, want_gaps), _nearest(y[b], x[b], mutant, want_gaps)
            nnx[b], nny[b] = rx[1], ry[1]
            if want_gaps:
                gx[b], gy[b] = rx[2], ry[2]
            sx, sy = sx + float(rx[0].astype(np.float64).sum()), sy + float(ry[0].astype(np.float64).sum())
            (vx, ix), (vy, iy) = _argmax_first(rx[0].astype(np.float64), mutant), _argmax_first(ry[0].astype(np.float64), mutant)
            if b == 0 or _beats(vx, mx, mutant):
                mx, win[0], win[1] = vx, b, ix
            if b == 0 or _beats(vy, my, mutant):
                my, win[2], win[3] = vy, b, iy
        values = {"chamfer": float(dt(sx / (float(den) * dN) + sy / (float(den) * dM))), "hausdorff": float(dt(mx + my))}
        grad = np.zeros((B, N, 3), dt)
        if kind == "chamfer":
            cx, cy = dt(float(grad_out) / (float(den) * dN)), dt(float(grad_out) / (float(den) * dM))
            for b in range(B):
                grad[b] = _pull(x[b], y[b][nnx[b]], cx)
                if mutant == "pull_every_duplicate":
                    d = _dist(x[b], y[b])
                    ii, jj = np.nonzero(d == d.min(0)[None, :])
                    order = np.argsort(jj, kind="stable")
                    ii, jj = ii[order], jj[order]
                else:
                    ii, jj = nny[b], np.arange(M)
                np.add.at(grad[b], ii, _pull(x[b][ii], y[b][jj], cy))      # unbuffered: ascending j
        else:
            wh = dt(grad_out)
            bx, i, by, j = win
            grad[bx, i] += _pull(x[bx, i][None], y[bx, nnx[bx, i]][None], wh)[0]
            grad[by, nny[by, j]] += _pull(x[by, nny[by, j]][None], y[by, j][None], wh)[0]
    out = dict(kind=kind, value=values[kind], values=values, grad=grad, nnx=nnx, nny=nny, win=[int(w) for w in win])
    if want_gaps:
        out.update(gx=gx, gy=gy)
    return out


# ------------------------------------------------------------------------------------------------------------ the bar
def value_bar(ref, err32):
    """the project's convention (tests/test_gpu_costs_edges.py::_check) under the bar tests/test_gpu_set_losses.py applies"""
    return min(4 * err32 + 1e-7 * abs(ref), 1e-5 * abs(ref))


def grad_bar(g_ref, err32):
    top = float(np.abs(g_ref).max())
    return min(4 * err32 + 1e-7 * top, 1e-4 * top + 1e-7)


def ratio(err, err32, scale):
    return err / (err32 + 0.25e-7 * scale + 1e-300)


# ------------------------------------------------------------------------------------------------------------ the cases
def _cloud(rng, B, N, M):
    return rng.uniform(-1, 1, (B, N, 3)).astype(np.float32), rng.uniform(-1, 1, (B, M, 3)).astype(np.float32)


def boundary_case(B, N, M, max_seed=2000):
    """Generic clouds at a shape where a loop of k_set_nn ends: the first seed of 0, 1, 2 ... whose float64 gaps
    (set_loss_restate.gaps) are >= GAP_BAR in all four entries.  -> (x, y, seed)"""
    import set_loss_restate as SR
    for seed in range(max_seed):
        x, y = _cloud(np.random.default_rng([seed, B, N, M]), B, N, M)
        if (SR.gaps(x, y) >= GAP_BAR).all():
            return x, y, seed
    raise AssertionError(f"no seed below {max_seed} meets the gap condition at {(B, N, M)}")


# the clouds lie in [-1, 1]^3, where no nearest distance exceeds the diagonal 3.47: a point out here is its side's maximum, and the
# pair P, Q (4 apart, 15 from the cube) is each other's nearest
FAR_P = np.array([10.0, 10.0, 10.0], np.float32)
FAR_Q = np.array([10.0, 10.0, 14.0], np.float32)
FAR_R = np.array([-10.0, -10.0, -10.0], np.float32)


def tie_case(kind):
    """Exact ties out of DUPLICATED points: exact in fp32 and float64 alike.  -> dict(x, y, note, tied: rows of x that share a
    maximum (the even split of torch.max() shows there), expect: what the rule has to give at the planted places)"""
    rng = np.random.default_rng([TIE_KINDS.index(kind), 77])
    off = np.array([0.01, 0.02, -0.01], np.float32)
    tied, expect = [], {}
    if kind == "dup_y":                  # y_2 = y_6 (graph 0) and y_0 = y_1 = y_7 (graph 1), each the nearest of a planted x
        x, y = _cloud(rng, 2, 9, 8)
        y[0, 6] = y[0, 2]
        x[0, 3] = y[0, 2] + off
        y[1, 1] = y[1, 7] = y[1, 0]
        x[1, 8] = y[1, 0] - off
        expect = {"nnx": [(0, 3, 2), (1, 8, 0)]}
    elif kind == "dup_x":                # x_1 = x_5 (graph 0), x_0 = x_4 = x_8 (graph 1): the lowest alone takes the y-side pull
        x, y = _cloud(rng, 2, 9, 8)
        x[0, 5] = x[0, 1]
        y[0, 4] = x[0, 1] + off
        x[1, 4] = x[1, 8] = x[1, 0]
        y[1, 7] = x[1, 0] - off
        expect = {"nny": [(0, 4, 1), (1, 7, 0)]}
    elif kind == "max_same_graph":       # N + M = 400: thread 5 owns points 5 and 261, threads 70 and 200 sit in waves 1 and 3
        x, y = _cloud(rng, 1, 300, 100)
        for i in (5, 70, 200, 261):
            x[0, i] = FAR_P
        tied, expect = [(0, 5), (0, 70), (0, 200), (0, 261)], {"win": [(0, 0), (1, 5)]}
    elif kind == "max_two_graphs":       # graphs 1 and 3 of five hold the same far pair, at a LOWER index in graph 3
        x, y = _cloud(rng, 5, 9, 7)
        x[1, 2], y[1, 6] = FAR_P, FAR_Q
        x[3, 0], y[3, 1] = FAR_P, FAR_Q
        tied, expect = [(1, 2), (3, 0)], {"win": [(0, 1), (1, 2), (2, 1), (3, 6)]}
    elif kind in ("both_graph0", "both_middle"):     # an x far from every y and a y far from every x, in one graph
        x, y = _cloud(rng, 3, 9, 7)
        b = 0 if kind == "both_graph0" else 1
        x[b, 7], y[b, 3] = FAR_P, FAR_R
        expect = {"win": [(0, b), (1, 7), (2, b), (3, 3)]}
    elif kind == "same_xi":              # the far pair: x_4 is the x-side winner and the nearest x of the y-side winner
        x, y = _cloud(rng, 3, 9, 7)
        x[2, 4], y[2, 5] = FAR_P, FAR_Q
        expect = {"win": [(0, 2), (1, 4), (2, 2), (3, 5)], "nny": [(2, 5, 4)], "nnx": [(2, 4, 5)]}
    elif kind == "single_coincident":
        x = rng.uniform(-1, 1, (1, 1, 3)).astype(np.float32)
        y = x.copy()
        expect = {"value": 0.0, "zero_grad": True}
    else:
        raise ValueError(kind)
    return dict(x=x, y=y, tied=tied, expect=expect)


def nonfinite_case(kind):
    """B = 3, N = 9, M = 7.  -> dict(x, y: with the non-finite entries; x0, y0: the clean clouds; bad: graphs that hold one;
    nan_rows: (b, i) of x points with a NaN coordinate)"""
    x0, y0 = _cloud(np.random.default_rng(909), 3, 9, 7)
    x, y = x0.copy(), y0.copy()
    nan_rows = []
    if kind == "nan_x":
        x[1, 4, 1] = np.nan
        bad, nan_rows = [1], [(1, 4)]
    elif kind == "nan_y":
        y[2, 0, 0] = np.nan
        bad = [2]
    elif kind == "inf_x":
        x[0, 3, 0] = np.inf
        bad = [0]
    elif kind == "inf_minus_inf":
        x[1, 2, 2] = np.inf
        y[1, 5, 2] = np.inf
        bad = [1]
    elif kind == "all_nan_graph":
        x[1], y[1] = np.nan, np.nan
        bad, nan_rows = [1], [(1, i) for i in range(9)]
    else:
        raise ValueError(kind)
    return dict(x=x, y=y, x0=x0, y0=y0, bad=bad, nan_rows=nan_rows)


PARTS = (5, 3, 2)                        # B_total = 5 graphs of the boundary case (5, 3, 2), in parts of 3 + 2
PART_SLICES = (slice(0, 3), slice(3, 5))
LDS_SHAPE = (2, 6739)                    # B, N of the largest accepted size: M = CHAMFER_MAX_POINTS - N


def lds_case(M):
    return _cloud(np.random.default_rng(6739), 2, LDS_SHAPE[1], M)


def named_cases():
    """name -> (x, y, B_total) of every case a mutant may be caught by"""
    out = {}
    for s in BOUNDARY_SHAPES:
        x, y, _ = boundary_case(*s)
        out["boundary %dx%dx%d" % s] = (x, y, None)
    for k in TIE_KINDS:
        c = tie_case(k)
        out["tie " + k] = (c["x"], c["y"], None)
    for k in NONFINITE_KINDS:
        c = nonfinite_case(k)
        out["nonfinite " + k] = (c["x"], c["y"], None)
    x, y, _ = boundary_case(*PARTS)
    for n, s in enumerate(PART_SLICES):
        out["part %d of 5x3x2" % n] = (x[s], y[s], PARTS[0])
    return out


def same_float(a, b):
    """equal, NaN = NaN and inf = inf"""
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def told_apart(rule64, rule32, mut):
    """Is a mutant's result on one case and kind told apart from the rule's: a differing table or winner (the winners count for the
    Hausdorff kind only: Chamfer never reads them), a differing non-finite pattern, or a value / gradient more than ten times the bar
    away?  -> the reason, or None"""
    if not (np.array_equal(rule64["nnx"], mut["nnx"]) and np.array_equal(rule64["nny"], mut["nny"])):
        return "table"
    if mut["kind"] == "hausdorff" and rule64["win"] != mut["win"]:
        return "winner"
    v, m = rule64["value"], mut["value"]
    fin_g = np.isfinite(rule64["grad"])
    if np.isfinite(v) != np.isfinite(m) or not np.array_equal(fin_g, np.isfinite(mut["grad"])):
        return "non-finite pattern"
    if np.isfinite(v) and abs(m - v) > 10 * value_bar(v, abs(rule32["value"] - v)):
        return "value"
    if fin_g.all() and np.abs(rule64["grad"]).max() > 0:
        err32 = float(np.abs(rule32["grad"].astype(np.float64) - rule64["grad"]).max())
        if np.abs(mut["grad"] - rule64["grad"]).max() > 10 * grad_bar(rule64["grad"], err32):
            return "gradient"
    return None


# ------------------------------------------------------------------------------------------------------------ the fused step
# TrainStep with all three terms on a synthetic batch: n_p = 257 puts N + M = 514 two strides and two points into k_set_nn, the
# labels are strided views of state_future (y_bstride = n_future * n_p * 3), and k_set_grad adds both weights into the chain's dpos.
FUSED = dict(N=258, n_p=257, n_his=4, B=3, per_recv=4, pstep=1, n_future=2)
FUSED_LOSSES = [("mse", 1.0), ("chamfer", 0.5), ("hausdorff", 0.25)]
FUSED_SEED = 0                           # the first seed fused_qualifies admits (tests/test_set_loss_edges.py walks them again)
FUSED_SENSITIVITY = 1e-6


def _chain(bt, W, dtype, device, losses, backward):
    import backward_shapes as BS
    import set_loss_restate as SR
    import torch
    stash = {}

    def loss(step, state, action, t):
        inp = dict(state=state, action=action, n_p=bt["n_p"], state_future=t(bt["state_future"]), eef_future=t(bt["eef_future"]),
                   action_future=t(bt["action_future"]))
        with torch.set_grad_enabled(backward):
            total, terms, preds = SR.chain_loss_terms(step, inp, FUSED["n_future"], losses)
        if backward:
            total.backward()
        stash.update(loss=float(total.detach()), terms=terms, preds=[p.double().cpu().numpy() for p in preds])
        return preds[0], preds[0]
    g, _, _ = BS.restate(bt, W, FUSED["pstep"], dtype, device, loss=loss)
    return g, stash


def fused_batch(seed):
    """backward_shapes.dense_batch plus the chain's inputs: eef_future and action_future (B, n_future - 1, N, 3), and the labels
    state_future (B, n_future, n_p, 3).  A step's prediction does not depend on the labels, so they are drawn AROUND the float64
    chain's own predictions (sigma 0.01, a fifth of the clouds' spacing): every predicted point then has one label far nearer than
    the next, which is what makes gaps of 1e-4 reachable with 2 x 771 points per step."""
    import torch
    import backward_shapes as BS
    import train_restate as TR
    c = FUSED
    bt = BS.dense_batch(c["N"], c["n_p"], c["n_his"], c["B"], c["per_recv"], seed)
    rng = np.random.default_rng(seed + 2)
    last = bt["state"][:, -1]
    bt["eef_future"] = np.stack([last + rng.normal(0, 0.01, last.shape) for _ in range(c["n_future"] - 1)], 1).astype(np.float32)
    act = np.zeros((c["B"], c["n_future"] - 1, c["N"], 3), np.float32)
    act[:, :, c["n_p"]:] = rng.normal(0, 0.05, (c["B"], c["n_future"] - 1, c["N"] - c["n_p"], 3))
    bt["action_future"] = act
    bt["state_future"] = np.zeros((c["B"], c["n_future"], c["n_p"], 3), np.float32)
    _, st = _chain(bt, TR.make_weights(5, c["n_his"]), torch.float64, "cpu", [("mse", 1.0)], backward=False)
    bt["state_future"] = np.stack([p + rng.normal(0, 0.01, p.shape) for p in st["preds"]], 1).astype(np.float32)
    return bt


def fused_restate(bt, W, dtype, device="cpu"):
    """The chain with FUSED_LOSSES under torch autograd in `dtype` -> ({name: gradient}, dict(loss, terms (n_future, 3), preds))."""
    return _chain(bt, W, dtype, device, FUSED_LOSSES, backward=True)


def fused_qualifies(seed):
    """-> (admitted, the chain's float64 gaps per step (n_future, 4), rounding sensitivity or None if the gaps already refuse)"""
    import torch
    import backward_shapes as BS
    import set_loss_restate as SR
    import train_restate as TR
    bt = fused_batch(seed)
    W = TR.make_weights(5, FUSED["n_his"])
    _, st = fused_restate(bt, W, torch.float64)
    gaps = np.array([SR.gaps(p, bt["state_future"][:, fi].astype(np.float64)) for fi, p in enumerate(st["preds"])])
    if not (gaps >= GAP_BAR).all():
        return False, gaps, None
    g64, _, _ = BS.restate(bt, W, FUSED["pstep"], torch.float64)
    sens = BS.rounding_sensitivity(bt, W, FUSED["pstep"], g64, BS.NAMES)
    return sens <= FUSED_SENSITIVITY, gaps, sens
