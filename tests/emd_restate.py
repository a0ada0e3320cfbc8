"""Restatement of the Earth-mover loss (reference src/dynamics/gnn/loss.py: EarthMoverLoss :25-60) in numpy float64: the
assignment solver (rectangular shortest augmenting paths with dual variables - Jonker & Volgenant 1987, Crouse 2016 - written from
the papers' description, with the tie rule the engine states: among equal path costs a free column wins, then the lowest column
index), the uniqueness gap of an assignment, and the loss value and its gradient.  Independent of the engine and of scipy: it is
the CPU yardstick of tests/test_emd.py, held there against scipy.optimize.linear_sum_assignment and against the reference's own
values and gradients in tests/golden/emd.npz and train_emd_rope.npz, and the oracle of the seeded GPU cases."""
from __future__ import annotations

import numpy as np
import torch

import set_loss_restate as SR
import train_restate as TR


def cost_matrix(x, y, dtype=np.float64):
    """x (N,3), y (M,3) -> (N,M) Euclidean distances computed in `dtype` (float32: the engine's and the reference's costs)."""
    d = np.asarray(x, dtype)[:, None, :] - np.asarray(y, dtype)[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _augment(c, u, v, col4row, row4col, cur):
    """One augmentation: the Dijkstra search from the free row `cur` over the columns in reduced costs, the dual update and the
    path flip, in place.  Returns the number of search steps.  Raises ValueError when no finite path exists."""
    K, L = c.shape
    sp = np.full(L, np.inf)
    scanned = np.zeros(L, bool)
    path = np.zeros(L, np.int64)
    minv, i, sink, steps = 0.0, cur, -1, 0
    for _ in range(L):
        steps += 1
        r = ((minv + c[i]) - u[i]) - v
        better = ~scanned & (r < sp)
        sp[better], path[better] = r[better], i
        cand = np.where(~scanned & (sp < np.inf))[0]
        if cand.size == 0:
            break
        # smallest path cost; among equals a free column, then the lowest index
        key = cand + np.where(row4col[cand] >= 0, L, 0)
        best = cand[np.lexsort((key, sp[cand]))[0]]
        minv = sp[best]
        scanned[best] = True
        if row4col[best] < 0:
            sink = best
            break
        i = row4col[best]
    if sink < 0:
        raise ValueError("cost matrix is infeasible")
    d = minv - sp[scanned]
    rows = row4col[scanned]
    u[rows[rows >= 0]] += d[rows >= 0]
    v[scanned] -= d
    u[cur] += minv
    j = sink
    while True:
        r = path[j]
        row4col[j] = r
        col4row[r], j = j, col4row[r]
        if r == cur:
            break
    return steps


def _solve_state(c):
    """c (K, L), K <= L -> (u, v, col4row, row4col, steps)."""
    K, L = c.shape
    u, v = np.zeros(K), np.zeros(L)
    col4row, row4col = np.full(K, -1), np.full(L, -1)
    steps = np.array([_augment(c, u, v, col4row, row4col, cur) for cur in range(K)], np.int64).reshape(K)
    return u, v, col4row, row4col, steps


def solve(cost):
    """Linear sum assignment of a cost matrix (n, m), any n and m: (ind1, ind2, steps) with ind1 ascending, len min(n, m), in the
    layout of scipy.optimize.linear_sum_assignment; steps[r] = search steps the augmentation of row r took (rows of the
    transposed problem when n > m).  Raises ValueError when no finite assignment exists."""
    c = np.array(cost, np.float64)
    transposed = c.shape[0] > c.shape[1]
    if transposed:
        c = c.T
    _, _, col4row, _, steps = _solve_state(c)
    rows, cols = np.arange(c.shape[0]), col4row.copy()
    if transposed:
        order = np.argsort(cols)
        rows, cols = cols[order], rows[order]
    return rows.astype(np.int64), cols.astype(np.int64), steps


def total(cost, ind1, ind2):
    return float(np.asarray(cost, np.float64)[ind1, ind2].sum())


def gap(cost):
    """float64 cost of the second-best assignment minus the best: every matched pair forbidden in turn, the problem solved again.
    inf where no other assignment exists.  Solving again starts from the optimum's duals: with the pair's cost at +inf they stay
    feasible and the other K - 1 matches stay tight, so one augmentation of the freed row gives the new optimum."""
    c = np.array(cost, np.float64)
    if c.shape[0] > c.shape[1]:
        c = c.T.copy()
    u, v, col4row, row4col, _ = _solve_state(c)
    rows = np.arange(c.shape[0])
    best, second = float(c[rows, col4row].sum()), np.inf
    for i in rows:
        j = col4row[i]
        u2, v2, c4r, r4c = u.copy(), v.copy(), col4row.copy(), row4col.copy()
        keep, c[i, j] = c[i, j], np.inf
        c4r[i], r4c[j] = -1, -1
        try:
            _augment(c, u2, v2, c4r, r4c, i)
            second = min(second, float(c[rows, c4r].sum()))
        except ValueError:
            pass
        c[i, j] = keep
    return second - best


def batch_gaps(x, y):
    """gap of every graph of a batch, on float64 costs of the given coordinates."""
    return np.array([gap(cost_matrix(a, b)) for a, b in zip(np.asarray(x), np.asarray(y))], np.float64)


def assignment(x, y, dtype=np.float64):
    """(ind1, ind2) of every graph, (B, K) int64, costs computed in `dtype`."""
    out = [solve(cost_matrix(a, b, dtype))[:2] for a, b in zip(np.asarray(x), np.asarray(y))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def greedy(cost):
    """The row-order greedy matching (every row of the smaller side takes its cheapest free column): a shortcut that must fail."""
    c = np.asarray(cost, np.float64)
    c = c.T if c.shape[0] > c.shape[1] else c
    taken, out = np.zeros(c.shape[1], bool), []
    for row in c:
        j = int(np.argmin(np.where(taken, np.inf, row)))
        taken[j] = True
        out.append(j)
    return np.array(out)


def shortcuts_fail(cost):
    """Greedy differs from the optimum, and the nearest-neighbour table of the row side is not one-to-one."""
    c = np.asarray(cost, np.float64)
    c = c.T if c.shape[0] > c.shape[1] else c
    _, opt, _ = solve(c)
    nn = c.argmin(1)
    return (not np.array_equal(greedy(c), opt)) and len(set(nn.tolist())) < len(nn)


def emd(x, y, ind1=None, ind2=None):
    """The loss as a torch expression over (B,N,3), (B,M,3) tensors (autograd reaches x): mean over the (B, K) matched norms,
    loss.py:54.  The assignment is data: given, or solved on the float64 costs of the detached clouds."""
    if ind1 is None:
        ind1, ind2 = assignment(x.detach().numpy(), y.detach().numpy())
    i1, i2 = torch.as_tensor(ind1), torch.as_tensor(ind2)
    b = torch.arange(x.shape[0])[:, None]
    return torch.linalg.vector_norm(x[b, i1] - y[b, i2], dim=2).mean()


def value_and_grad(x, y, ind1=None, ind2=None):
    xt = torch.as_tensor(np.asarray(x, np.float64)).clone().requires_grad_(True)
    v = emd(xt, torch.as_tensor(np.asarray(y, np.float64)), ind1, ind2)
    v.backward()
    return v.item(), xt.grad.numpy()


def term_value(name, pred, gt):
    return emd(pred, gt) if name == "earth_mover" else SR.term_value(name, pred, gt)


def restated_chain(f, losses, dtype=torch.float64):
    """SR.restated_chain with the Earth-mover term known: (loss_sum, terms, predictions, 22 gradients, dstate0)."""
    inp = TR.fixture_inputs(f, dtype)
    B, N = inp["attrs"].shape[:2]
    recv, send = TR.fixture_edges(f, B, N)
    W = TR.weights(f, dtype)
    inp["state"].requires_grad_(True)
    state, action, n_p, n_future = inp["state"], inp["action"], inp["n_p"], int(f["n_future"])
    loss, table, preds = 0, [], []
    for fi in range(n_future):
        gt = inp["state_future"][:, fi]
        pred, _ = TR.forward(W, state, inp["attrs"], action, inp["phys"], inp["group"], recv, send, n_p, int(f["pstep"]))
        p = pred[:, :gt.shape[1], :3]
        vals = [term_value(name, p, gt) for name, _ in losses]
        loss = loss + sum(w * v for (_, w), v in zip(losses, vals))
        table.append([float(v.detach()) for v in vals])
        preds.append(p.detach())
        if fi < n_future - 1:
            nxt = inp["eef_future"][:, fi].clone().unsqueeze(1)
            nxt[:, -1, :n_p] = pred[:, :n_p]
            state = torch.cat([state[:, 1:], nxt], 1)
            action = inp["action_future"][:, fi]
    loss.backward()
    return loss.item(), np.array(table, np.float64), preds, {k: W[k].grad.numpy() for k in TR.KEYS}, inp["state"].grad.numpy()
