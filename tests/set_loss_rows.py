"""The training set losses over each graph's REAL ROWS (AG_LOSS_ROWS; csrc/ag_setloss.hip, ag_emd.hip): the rule in numpy.  No GPU, no
library.

rows_rule restates what include/adaptigraph_amd.h documents for kind | AG_LOSS_ROWS, built from the primitives of
tests/set_loss_edges.py (_nearest, _argmax_first, _pull, ratio) and, for the Earth-mover kind, the solver of tests/emd_restate.py:
  * counts are clamped into [0, N] / [0, M]; graph b's clouds are x[b, :nx_b], y[b, :ny_b]; a graph with an empty side is empty;
  * chamfer     = (1/B_total) sum_b [ mean_{i<nx_b} min_{j<ny_b} d + mean_{j<ny_b} min_{i<nx_b} d ]
  * hausdorff   = max_{b, i<nx_b} mx + max_{b, j<ny_b} my; winner the lowest (b, index) among equals, the first NaN beats every number
  * earth_mover = (1/B_total) sum_b (1/K_b) sum of the optimal assignment of the real rows, K_b = min(nx_b, ny_b)
  * an empty graph adds 0, has no Hausdorff candidate (none at all: value 0, winners -1), zero gradient rows, and counts in B_total;
  * gradient rows i >= nx_b are 0; scales g/(B_total nx_b), g/(B_total ny_b), g/(B_total K_b);
  * arg-min entries of padding rows are 0, match entries of padding or unmatched rows -1.
In float64 it is the yardstick, in float32 the error scale of the bar (set_loss_edges.ratio).  tests/test_set_loss_rows.py holds it
against the reference's recordings (tests/golden/set_losses_rows.npz), against set_rule / emd_restate at full counts and against the
MUTANTS below; tests/test_gpu_set_loss_rows.py holds the kernels against it."""
from __future__ import annotations

import numpy as np

import emd_restate as ER
import set_loss_edges as SE

MUTANTS = ("denominator_padded", "pooled_mean", "pad_rows_searched", "pad_grad_nonzero", "counts_swapped", "empty_is_nan",
           "emd_K_padded", "hausdorff_pad_wins")
KINDS = ("chamfer", "hausdorff", "earth_mover")
GAP_BAR = SE.GAP_BAR

# the fixture's batches (tests/golden/make_golden_set_losses_rows.py)
BATCH_A = dict(B=6, N=9, M=7, nx=[9, 5, 1, 0, 9, 3], ny=[7, 7, 2, 4, 0, 3])
BATCH_B = dict(B=3, N=40, M=40, nx=[40, 23, 1], ny=[40, 23, 1])


def clamp_counts(nx, ny, N, M, mutant=None):
    """-> (nx, ny) int64 (B,), clamped into range, both 0 where either is"""
    nx, ny = np.clip(np.asarray(nx, np.int64), 0, N), np.clip(np.asarray(ny, np.int64), 0, M)
    if mutant == "counts_swapped":
        nx, ny = np.clip(ny, 0, N), np.clip(nx, 0, M)
    empty = (nx == 0) | (ny == 0)
    return np.where(empty, 0, nx), np.where(empty, 0, ny)


def _emd_graph(xb, yb, dt):
    """the optimal assignment of two non-empty clouds on their distances in dtype `dt`: (ind1, ind2, matched distances in dt)"""
    c = ER.cost_matrix(xb, yb, dt)
    i1, i2, _ = ER.solve(c)
    return i1, i2, c[i1, i2]


def rows_rule(x, y, nx, ny, dtype=np.float64, kind="chamfer", grad_out=1.0, B_total=None, mutant=None, want_gaps=False):
    """x (B,N,3), y (B,M,3), counts (B,) -> dict(kind, value, grad (B,N,3), nnx (B,N), nny (B,M), win [b, i, b, j]; earth_mover:
    match (B,N), ind1 / ind2 (B, min(N,M)) with -1 beyond K_b, failed (B,)).  want_gaps: gx (B,N), gy (B,M) nearest-neighbour gaps
    of the real rows (inf elsewhere)."""
    assert kind in KINDS and (mutant is None or mutant in MUTANTS)
    dt = np.dtype(dtype).type
    x, y = np.asarray(x).astype(dt), np.asarray(y).astype(dt)
    B, N, M = x.shape[0], x.shape[1], y.shape[1]
    B_total = B if B_total is None else B_total
    nxs, nys = clamp_counts(nx, ny, N, M, mutant)
    g = float(grad_out)
    grad = np.zeros((B, N, 3), dt)
    out = dict(kind=kind, nx=nxs, ny=nys)
    with np.errstate(all="ignore"):
        if kind == "earth_mover":
            Kp = min(N, M)
            match = np.full((B, N), -1, np.int64)
            ind1, ind2 = np.full((B, Kp), -1, np.int64), np.full((B, Kp), -1, np.int64)
            failed = np.zeros(B, bool)
            total = 0.0
            for b in range(B):
                n, m = int(nxs[b]), int(nys[b])
                if n == 0:
                    if mutant == "empty_is_nan":
                        total = np.nan
                    continue
                K = Kp if mutant == "emd_K_padded" else min(n, m)
                if not (np.isfinite(x[b, :n]).all() and np.isfinite(y[b, :m]).all()):
                    failed[b], total = True, np.nan
                    grad[b, :n] = np.nan
                    continue
                i1, i2, d = _emd_graph(x[b, :n], y[b, :m], dt)
                match[b, i1] = i2
                ind1[b, :len(i1)], ind2[b, :len(i1)] = i1, i2
                s = 0.0
                for v in d:                                                  # ascending i
                    s += float(v)
                total = total + s / K
                grad[b, i1] = SE._pull(x[b, i1], y[b, i2], dt(g / (float(B_total) * K)))
                if mutant == "pad_grad_nonzero" and n < N:
                    grad[b, n:] = SE._pull(x[b, n:], np.repeat(y[b, :1], N - n, 0), dt(g / (float(B_total) * K)))
            out.update(value=float(dt(total / float(B_total))), grad=grad, match=match, ind1=ind1, ind2=ind2, failed=failed,
                       nnx=np.zeros((B, N), np.int64), nny=np.zeros((B, M), np.int64), win=[-1, -1, -1, -1])
            return out

        nnx, nny = np.zeros((B, N), np.int64), np.zeros((B, M), np.int64)
        gx, gy = np.full((B, N), np.inf), np.full((B, M), np.inf)
        mean_sum_x = mean_sum_y = 0.0                                        # the sums of the per-graph means
        pool_x = pool_y = 0.0
        mx = my = None
        win = [-1, -1, -1, -1]
        for b in range(B):
            n, m = int(nxs[b]), int(nys[b])
            if n == 0:
                if mutant == "empty_is_nan":
                    mean_sum_x = np.nan
                continue
            ycand = y[b] if mutant == "pad_rows_searched" else y[b, :m]      # the candidates of an x row
            xcand = x[b] if mutant == "pad_rows_searched" else x[b, :n]
            xq = x[b] if mutant == "hausdorff_pad_wins" else x[b, :n]        # the rows that search
            yq = y[b] if mutant == "hausdorff_pad_wins" else y[b, :m]
            rx, ry = SE._nearest(xq, ycand, None, want_gaps), SE._nearest(yq, xcand, None, want_gaps)
            nnx[b, :n], nny[b, :m] = rx[1][:n], ry[1][:m]
            if want_gaps:
                gx[b, :n], gy[b, :m] = rx[2][:n], ry[2][:m]
            sx, sy = float(rx[0][:n].astype(np.float64).sum()), float(ry[0][:m].astype(np.float64).sum())
            dn, dm = (N, M) if mutant == "denominator_padded" else (n, m)
            mean_sum_x, mean_sum_y = mean_sum_x + sx / dn, mean_sum_y + sy / dm
            pool_x, pool_y = pool_x + sx, pool_y + sy
            (vx, ix), (vy, iy) = SE._argmax_first(rx[0].astype(np.float64)), SE._argmax_first(ry[0].astype(np.float64))
            if mx is None or SE._beats(vx, mx, None):
                mx, win[0], win[1] = vx, b, ix
            if my is None or SE._beats(vy, my, None):
                my, win[2], win[3] = vy, b, iy
        if mutant == "pooled_mean":
            chamfer = pool_x / max(1, int(nxs.sum())) + pool_y / max(1, int(nys.sum()))
        else:
            chamfer = mean_sum_x / float(B_total) + mean_sum_y / float(B_total)
        hausdorff = (0.0 if mx is None else mx) + (0.0 if my is None else my)
        values = {"chamfer": float(dt(chamfer)), "hausdorff": float(dt(hausdorff))}
        if kind == "chamfer":
            for b in range(B):
                n, m = int(nxs[b]), int(nys[b])
                if n == 0:
                    continue
                if mutant == "pooled_mean":
                    cx, cy = dt(g / max(1, int(nxs.sum()))), dt(g / max(1, int(nys.sum())))
                else:
                    dn, dm = (N, M) if mutant == "denominator_padded" else (n, m)
                    cx, cy = dt(g / (float(B_total) * dn)), dt(g / (float(B_total) * dm))
                grad[b, :n] = SE._pull(x[b, :n], y[b][nnx[b, :n]], cx)
                np.add.at(grad[b], nny[b, :m], SE._pull(x[b][nny[b, :m]], y[b, :m], cy))      # unbuffered: ascending j
                if mutant == "pad_grad_nonzero" and n < N:
                    grad[b, n:] = SE._pull(x[b, n:], np.repeat(y[b, :1], N - n, 0), cx)
        elif win[0] >= 0:
            wh = dt(g)
            bx, i, by, j = win
            grad[bx, i] += SE._pull(x[bx, i][None], y[bx, nnx[bx, i]][None], wh)[0]
            grad[by, nny[by, j]] += SE._pull(x[by, nny[by, j]][None], y[by, j][None], wh)[0]
            if mutant == "pad_grad_nonzero":
                for b in range(B):
                    n = int(nxs[b])
                    if 0 < n < N:
                        grad[b, n:] = SE._pull(x[b, n:], np.repeat(y[b, :1], N - n, 0), wh)
    out.update(value=values[kind], values=values, grad=grad, nnx=nnx, nny=nny, win=[int(w) for w in win])
    if want_gaps:
        out.update(gx=gx, gy=gy)
    return out


def emd_gaps(x, y, nx, ny):
    """uniqueness gap of every graph's assignment over its real rows in float64; inf for an empty graph"""
    nxs, nys = clamp_counts(nx, ny, np.shape(x)[1], np.shape(y)[1])
    return np.array([ER.gap(ER.cost_matrix(a[:n], b[:m])) if n else np.inf for a, b, n, m in zip(np.asarray(x), np.asarray(y), nxs, nys)])


def told_apart(rule64, rule32, mut):
    """Is a mutant's result told apart from the rule's: a differing table, winner or match, a differing non-finite pattern, or a
    value / gradient more than ten times the bar away (set_loss_edges.value_bar / grad_bar)?  -> the reason, or None"""
    if not (np.array_equal(rule64["nnx"], mut["nnx"]) and np.array_equal(rule64["nny"], mut["nny"])):
        return "table"
    if mut["kind"] == "hausdorff" and rule64["win"] != mut["win"]:
        return "winner"
    if mut["kind"] == "earth_mover" and not np.array_equal(rule64["match"], mut["match"]):
        return "match"
    v, m = rule64["value"], mut["value"]
    fin_g = np.isfinite(rule64["grad"])
    if np.isfinite(v) != np.isfinite(m) or not np.array_equal(fin_g, np.isfinite(mut["grad"])):
        return "non-finite pattern"
    if np.isfinite(v) and abs(m - v) > 10 * SE.value_bar(v, abs(rule32["value"] - v)) + 1e-300:
        return "value"
    if fin_g.all():
        err32 = float(np.abs(rule32["grad"].astype(np.float64) - rule64["grad"]).max())
        if np.abs(mut["grad"] - rule64["grad"]).max() > 10 * SE.grad_bar(rule64["grad"], err32):
            return "gradient"
    return None


# ------------------------------------------------------------------------------------------------------------ the cases
def cloud(seed, B, N, M):
    """generic clouds in [-1, 1]^3; the label sits near the prediction's points so that assignments are unique by a margin"""
    rng = np.random.default_rng([seed, B, N, M])
    x = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    y = (x[:, rng.integers(0, N, M)] + rng.normal(0, 0.15, (B, M, 3))).astype(np.float32)
    return x, y


def qualifies(x, y, nx, ny):
    """every real row's nearest-neighbour gap, the gap between the two largest minima per side and every graph's assignment gap are
    >= GAP_BAR in float64: two correct implementations then pick the same tables, winners and matches"""
    r = rows_rule(x, y, nx, ny, np.float64, "hausdorff", want_gaps=True)
    if min(r["gx"].min(), r["gy"].min()) < GAP_BAR:
        return False
    for side, cnt in (("x", r["nx"]), ("y", r["ny"])):
        mins = []
        for b in range(len(cnt)):
            a, c = (x[b, :r["nx"][b]], y[b, :r["ny"][b]]) if side == "x" else (y[b, :r["ny"][b]], x[b, :r["nx"][b]])
            if len(a):
                mins.append(SE._nearest(a.astype(np.float64), c.astype(np.float64))[0])
        if mins:
            top = np.sort(np.concatenate(mins))[::-1]
            if len(top) > 1 and top[0] - top[1] < GAP_BAR:
                return False
    return bool((emd_gaps(x, y, nx, ny) >= GAP_BAR).all())


def case(B, N, M, nx, ny, max_seed=400):
    """the first seed whose clouds qualify -> (x, y, seed)"""
    for seed in range(max_seed):
        x, y = cloud(seed, B, N, M)
        if qualifies(x, y, nx, ny):
            return x, y, seed
    raise AssertionError(f"no seed below {max_seed} qualifies at {(B, N, M)}")


def with_padding(x, y, nx, ny, fill):
    """the rows behind the (clamped) counts set to `fill`"""
    x, y = x.copy(), y.copy()
    nxs, nys = np.clip(nx, 0, x.shape[1]), np.clip(ny, 0, y.shape[1])
    for b in range(len(x)):
        x[b, nxs[b]:], y[b, nys[b]:] = fill, fill
    return x, y
