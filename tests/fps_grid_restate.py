"""The cell-pruned farthest-point sampler (adaptigraph_amd/csrc/ag_fps_grid.hip) restated in plain numpy, for both stages, with its
`cells` knob: what the kernel is read against.  Pinned on tests/dataset_restate.py's brute-force sweeps by
tests/test_fps_grid_restate.py.

The cloud is binned into cells; a cell keeps its tight box and the largest running minimum among its members (with the lowest
original index that has it).  After a new centre c only the cells with NOT (bound >= cellmax) are visited, where bound is the
sampler's own fp32 distance arithmetic applied to the per-axis gaps max(lo - c, c - hi, 0).  Rounding to nearest is monotone, so
the bound is <= every member's computed distance and a skipped cell is one the brute-force sweep would have left unchanged
(DESIGN.md section 3.27).  The partition never enters the result, so the binning below need not - and does not try to - reproduce
the kernel's cell of every point.
"""
import numpy as np

F32 = np.float32
CELL_POINTS, MAX_CELLS = 64, 16384           # the default policy: about 64 points per cell, a power-of-two cell count


def sq_dist(p, c):
    """fp32 ((dx*dx + dy*dy) + dz*dz), separate products and sums (dataset_restate.sq_dist)."""
    d = p - c
    s = d * d
    return (s[..., 0] + s[..., 1]) + s[..., 2]


def cell_bound(lo, hi, c, stage2):
    """The fp32 bound of boxes lo, hi (C, 3) against centre c: the distance arithmetic on the gaps.  fmax drops a NaN operand, as
    the device's fmaxf does: a NaN gap counts as 0, which can only make a cell visited."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.fmax(np.fmax(lo - c, c - hi), F32(0))
        b = sq_dist(g, F32(0))
        return np.sqrt(b) if stage2 else b


def default_cells(n):
    c = 1
    while c < MAX_CELLS and c * CELL_POINTS < n:
        c *= 2
    return c


def bin_points(p, cells=None):
    """(members, lo, hi): members[c] = ascending original indices of cell c, the last cell holding the points with a non-finite
    coordinate (box (-inf, +inf): never pruned while its maximum is positive); lo, hi (C + 1, 3) the tight boxes (0 where empty)."""
    p = np.ascontiguousarray(p, F32)
    n = len(p)
    fin = np.isfinite(p).all(1)
    nax = np.ones(3, np.int64)
    cid = np.zeros(n, np.int64)
    if fin.any():
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            lo, hi = p[fin].min(0), p[fin].max(0)
            ext = hi - lo
            want = default_cells(n) if cells is None else int(cells)
            c = 1
            while c < want:                  # halve the axis whose cells are longest; a zero extent keeps one cell
                ln = np.where((ext > 0) & np.isfinite(ext), ext / nax.astype(F32), F32(0))
                if not (ln > 0).any():
                    break
                nax[int(np.argmax(ln))] *= 2
                c *= 2
            inv = np.where(nax > 1, nax.astype(F32) / np.where(ext > 0, ext, F32(1)), F32(0)).astype(F32)
            u = (p - lo) * inv
            u = np.where(np.isnan(u), 0, u)
            ax = np.clip(u, 0, nax - 1).astype(np.int64)
        cid = (ax[:, 2] * nax[1] + ax[:, 1]) * nax[0] + ax[:, 0]
    ncells = int(nax.prod())
    cid = np.where(fin, cid, ncells)
    order = np.argsort(cid, kind="stable")
    start = np.searchsorted(cid[order], np.arange(ncells + 2))
    members = [order[start[c]:start[c + 1]] for c in range(ncells + 1)]
    lo = np.zeros((ncells + 1, 3), F32)
    hi = np.zeros((ncells + 1, 3), F32)
    for c in range(ncells):
        if len(members[c]):
            lo[c], hi[c] = p[members[c]].min(0), p[members[c]].max(0)
    lo[ncells], hi[ncells] = -np.inf, np.inf
    return members, lo, hi


def _select(p, cells, stage2, start, n_pick, radius, stats):
    """Both stages' loop.  Stage 1: exactly n_pick picks from `start`.  Stage 2: from `start` while the maximum is > radius and
    points are left."""
    p = np.ascontiguousarray(p, F32)
    n = len(p)
    members, lo, hi = bin_points(p, cells)
    md0 = F32(np.inf) if stage2 else F32(1e10)
    md = np.full(n, md0)
    cellmax = np.array([md0 if len(m) else F32(0) for m in members], F32)
    cellarg = np.array([m[0] if len(m) else n for m in members], np.int64)
    live = np.array([len(m) > 0 for m in members])
    picks = [int(start)]
    r = F32(radius)
    while True:
        if not stage2 and len(picks) >= n_pick:
            break
        c = p[picks[-1]]
        with np.errstate(invalid="ignore", over="ignore"):
            visit = ~(cell_bound(lo, hi, c, stage2) >= cellmax) & live          # a NaN bound visits
            for k in np.nonzero(visit)[0]:
                m = members[k]
                d = sq_dist(p[m], c)
                if stage2:
                    d = np.sqrt(d)
                new = np.where(md[m] > d, d, md[m])                             # the kernel's md > d ? d : md: a NaN d changes nothing
                md[m] = new
                a = int(np.argmax(new))                                         # members ascend: the lowest index among equals
                cellmax[k], cellarg[k] = new[a], m[a]
                if stats is not None:
                    stats["evals"] = stats.get("evals", 0) + len(m)
        mx = cellmax.max()
        if stage2 and (not (mx > r) or len(picks) >= n):
            break
        picks.append(int(cellarg[cellmax == mx].min()))                         # the largest packed key
    return np.array(picks, np.int64)


def fps_stage1(points, n_sample, start, cells=None, stats=None):
    return _select(points, cells, False, start, n_sample, 0.0, stats)


def fps_stage2(points, radius, start, cells=None, stats=None):
    return _select(points, cells, True, start, 0, radius, stats)


def fps_indices(cloud, max_nobj, fps_start, fps_radius, rad_start, cells=None, stats=None):
    """dataset_restate.fps_indices by the pruned selection: stage1[stage2], in selection order."""
    cloud = np.ascontiguousarray(cloud, F32)
    i1 = fps_stage1(cloud, min(max_nobj, len(cloud)), fps_start, cells, stats)
    return i1[fps_stage2(cloud[i1], fps_radius, rad_start, cells, stats)]
