"""numpy restatement of the cell-list edge builder's grid (adaptigraph_amd/csrc/ag_cells.hip) - TEST INFRASTRUCTURE ONLY.

The property everything rests on: a pair that passes the reference's exact test, (dis - thr2) < 0 in fp32, lies within one cell
of each other on every axis, so a receiver that looks at the 27 cells around its own misses no sender.  cull_radius, make_grid
and cell_axis follow k_cells_bounds / cell_axis operation by operation, in np.float32 (IEEE, round to nearest, like the
kernel's __fsub_rn / __fmul_rn); build_edges is the whole builder on top of them - candidates only from neighbouring cells - so
that a hole in the grid shows as a missing edge against the oracle, on the CPU.
"""
import numpy as np

F32 = np.float32
AXIS_MAX = 1024            # CELLS_AXIS_MAX
FMAX = np.finfo(np.float32).max
EDGE_MARGIN = F32(1.001)   # cell edge over the culling radius (k_cells_bounds); the tests lower it to show that their attack can fail


def cells_cap_for(N):
    c = 64
    while c < N and c < (1 << 20):
        c <<= 1
    return c


def cull_radius(thr2):
    """r with fl(r*r) >= thr2: every pair that passes the test has |fl(x_i - x_j)| < r on each axis."""
    with np.errstate(invalid="ignore", over="ignore"):
        return F32(np.sqrt(F32(thr2)) * F32(1.0001))


def make_grid(pts, thr2, cells_cap):
    """pts (M,3) float32: the finite coordinates of the valid particles.  -> dict(lo (3,), inv_h, n (3,), ncells)."""
    thr2 = F32(thr2)
    g = dict(lo=np.zeros(3, F32), inv_h=F32(0), n=np.ones(3, np.int64), ncells=0, thr2=thr2)
    if not (thr2 > 0) or len(pts) == 0:
        return g
    lo, hi = pts.min(0).astype(F32), pts.max(0).astype(F32)
    g["lo"], g["ncells"] = lo, 1
    r = cull_radius(thr2)
    if not (r < FMAX):
        return g
    with np.errstate(over="ignore"):
        E = (hi - lo).astype(F32)
    on = E < FMAX
    h = F32(r * EDGE_MARGIN)
    for c in range(3):
        if on[c]:
            h = max(h, F32(F32(E[c] / F32(AXIS_MAX)) * F32(1.001)))
    for _ in range(256):
        inv = F32(F32(1) / h)
        n = np.array([int(F32(E[c] * inv)) + 1 if on[c] else 1 for c in range(3)], np.int64)
        if (n < AXIS_MAX).all() and int(n.prod()) <= cells_cap:
            g["inv_h"], g["n"], g["ncells"] = inv, n, int(n.prod())
            return g
        h = F32(h * F32(1.26))
    return g                                               # one cell: correct, only slower


def cell_axis(x, lo, inv_h, n):
    """Cell of coordinate(s) x on an axis of n cells from lo: monotone non-decreasing in x."""
    x = np.asarray(x, F32)
    if n == 1:
        return np.zeros(x.shape, np.int64)
    u = ((x - F32(lo)).astype(F32) * F32(inv_h)).astype(F32)
    return np.where(u >= F32(n - 1), n - 1, u.astype(np.int64)).astype(np.int64)


def cells_of(pts, g):
    return np.stack([cell_axis(pts[:, c], g["lo"][c], g["inv_h"], int(g["n"][c])) for c in range(3)], 1)


def pair_passes(pi, pj, thr2):
    """The reference's test on one pair, fp32, no FMA."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(pi, F32) - np.asarray(pj, F32)).astype(F32)
        sq = (d * d).astype(F32)
        dis = F32(F32(sq[0] + sq[1]) + sq[2])
        return bool(F32(dis - F32(thr2)) < 0)


def build_edges(pos, thr2, mask, tool, topk, rule, cells_cap=None):
    """The cell builder on the CPU: rule 0 none, 1 batch (flag, tool<->tool stays), 2 single graph.  -> (recv, send) int32."""
    pos = np.ascontiguousarray(pos, F32)
    N = pos.shape[0]
    mask, tool = np.asarray(mask, bool), np.asarray(tool, bool)
    thr2 = F32(thr2)
    binned = mask & np.isfinite(pos).all(1)
    g = make_grid(pos[binned], thr2, cells_cap or cells_cap_for(N))
    k = min(N, int(topk))
    adj = np.zeros((N, N), bool)
    if g["ncells"]:
        idx = np.nonzero(binned)[0]
        cells = cells_of(pos[idx], g)
        for a, i in enumerate(idx):
            near = (np.abs(cells - cells[a]) <= 1).all(1)
            js = idx[near]
            d = (pos[i][None] - pos[js]).astype(F32)
            sq = (d * d).astype(F32)
            dis = ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)
            within = ((dis - thr2).astype(F32) < 0) & ~(tool[i] & tool[js])
            js, dis = js[within], dis[within]
            order = np.lexsort((js, dis))[:k]             # (dis, sender index)
            adj[i, js[order]] = True
    if rule:
        flag = True if rule == 2 else bool(adj[tool[:, None] & ~tool[None, :]].any())
        adj[tool[:, None] & mask[None, :]] = False
        adj[tool[None, :] & mask[:, None]] = flag
        if rule == 2:
            adj[tool[:, None] & tool[None, :]] = False
    recv, send = np.nonzero(adj)
    return recv.astype(np.int32), send.astype(np.int32)
