"""Seeded inputs of tests/test_gpu_chamfer_tiled.py beyond those of tests/costs_restate.py; tests/test_chamfer_tiled_host.py checks
their preconditions on the CPU."""
from __future__ import annotations

import numpy as np
import torch

import costs_restate as CR

F32 = np.float32
EXTRA_SHAPES = [(2049, 5), (5, 2049)]                         # three owning blocks of 1024 points on one side
PREFIX = (257, 255, 7000, 7000)                               # compact N, M; slots of the embedding: 14,000 > CR.CHAMFER_MAX_POINTS
DENSE = (6740, 6741)                                          # one point past the LDS limit
NEAR_TIE = 1e-4
TIE_ROWS = (3, 3 + 64, 3 + 1024)                              # the same x point: across a 64-point tile boundary, and in the next owning block
TIE_Y = (2, 5, 11, 30)                                        # y points placed next to it


def prefix_embedding(By, fill=0.0):
    """-> (x, y) compact, (X, Y, Xm, Ym) the same clouds as the first rows of `fill`-filled clouds, masks true on the prefix only."""
    n, m, N, M = PREFIX
    x, y, _, _ = CR.chamfer_case(n, m, By, "none")
    X, Y = np.full((x.shape[0], N, 3), fill, F32), np.full((By, M, 3), fill, F32)
    X[:, :n], Y[:, :m] = x, y
    Xm, Ym = np.zeros((x.shape[0], N), bool), np.zeros((By, M), bool)
    Xm[:, :n], Ym[:, :m] = True, True
    return (x, y), (X, Y, Xm, Ym)


def tie_case(N=1100, M=40, R=2):
    """x holds one point three times (TIE_ROWS); the y points TIE_Y sit within 2e-3 of it, so their three candidate distances are
    equal bit for bit and every one of them is nearest to that point."""
    rng = np.random.default_rng([26, N, M])
    x = rng.normal(0.0, 1.0, (R, N, 3)).astype(F32)
    y = rng.normal(0.2, 1.0, (R, M, 3)).astype(F32)
    x[:, 3] = F32([0.25, -0.5, 0.125])                        # (a fixed point inside the cloud)
    for i in TIE_ROWS[1:]:
        x[:, i] = x[:, 3]
    for k, j in enumerate(TIE_Y):
        y[:, j] = x[:, 3] + (rng.uniform(-1e-3, 1e-3, (R, 3)) + 1e-4 * (k + 1)).astype(F32)
    return x, y


def dense_case():
    N, M = DENSE
    x, y, _, _ = CR.chamfer_case(N, M, 2, "none", R=2)
    return x, y


def _two_smallest(a, b):
    """Element-wise the two smallest of the (n,2) candidates a and b, ascending."""
    return torch.topk(torch.cat([a, b], 1), 2, dim=1, largest=False).values


def near_tie_rows(x, y, gap=NEAR_TIE, chunk=512):
    """x (R,N,3), y (R,M,3) -> (R,N) bool: the x rows whose gradient a near-tie touches, in float64 - an x whose own two nearest y
    are closer than `gap` to each other in distance, and the two nearest x of any y with such a gap."""
    x, y = CR.T(x), CR.T(y)
    out = np.zeros(x.shape[:2], bool)
    for r in range(x.shape[0]):
        best = torch.full((x.shape[1], 2), float("inf"), dtype=CR.F64)
        for j0 in range(0, y.shape[1], chunk):
            d = CR._dist(x[r], y[r, j0:j0 + chunk])           # (m, N)
            if d.shape[0] >= 2:
                best = _two_smallest(best, torch.topk(d, 2, dim=0, largest=False).values.T)
            else:
                best = _two_smallest(best, torch.cat([d.T, torch.full((x.shape[1], 1), float("inf"), dtype=CR.F64)], 1))
            if d.shape[1] >= 2:
                two = torch.topk(d, 2, dim=1, largest=False)
                close = (two.values[:, 1] - two.values[:, 0]) < gap
                out[r, two.indices[close].reshape(-1).numpy()] = True
        out[r] |= ((best[:, 1] - best[:, 0]) < gap).numpy()
    return out
