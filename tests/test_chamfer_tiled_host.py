"""CPU checks of the tiled Chamfer cost (csrc/ag_chamfer_tiled.hip): where its two exports live, what the package exports, and the
preconditions of the cases tests/test_gpu_chamfer_tiled.py runs (tests/chamfer_tiled_cases.py)."""
import os
import re

import numpy as np
import pytest
import torch

import chamfer_tiled_cases as TC
import costs_restate as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ag_cost_chamfer_tiled", "ag_cost_chamfer_tiled_backward")


def test_the_two_exports_belong_to_the_cells_library():
    from adaptigraph_amd import _lib
    raw = open(os.path.join(ROOT, "include", "adaptigraph_amd_cells.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in NAMES:
        assert name in _lib.CELLS_EXPORTS and name not in _lib.EXPORTS
        assert re.search(r"\bint " + name + r"\s*\(", src), name
    assert "empty valid set" in raw and "tile_points" in src
    assert "ag_cost_chamfer_tiled" not in open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()


def test_the_package_exports_the_three_functions_and_they_have_no_cpu_fallback():
    import adaptigraph_amd as ag
    x, y = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    for name in ("chamfer_tiled", "chamfer_tiled_diff", "mean_chamfer_tiled"):
        assert callable(getattr(ag, name)) and name in ag.__all__
    for call in (lambda: ag.chamfer_tiled(x, y), lambda: ag.chamfer_tiled(x, y, tile=64), lambda: ag.chamfer_tiled_diff(x, y),
                 lambda: ag.mean_chamfer_tiled(x, y, torch.ones(1, 4, dtype=torch.bool), torch.ones(1, 5, dtype=torch.bool))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_dense_case_leaves_out_at_most_one_percent_of_its_rows():
    x, y = TC.dense_case()
    assert x.shape == (2, 6740, 3) and y.shape == (2, 6741, 3) and x.shape[1] + y.shape[1] == CR.CHAMFER_MAX_POINTS + 1
    out = TC.near_tie_rows(x, y)
    share = out.mean(1)
    print("left out:", out.sum(1).tolist(), "of", x.shape[1], "rows:", share.tolist())
    assert out.sum(1).tolist() == [38, 33] and float(share.max()) <= 0.01
    # the helper agrees with the plain definition on a small case
    xs, ys = x[:1, :300], y[:1, :200]
    d = CR._dist(CR.T(xs[0]), CR.T(ys[0]))                    # (200, 300)
    want = np.zeros(300, bool)
    tx = torch.topk(d, 2, dim=0, largest=False).values
    want |= ((tx[1] - tx[0]) < 5e-3).numpy()
    ty = torch.topk(d, 2, dim=1, largest=False)
    want[ty.indices[(ty.values[:, 1] - ty.values[:, 0]) < 5e-3].reshape(-1).numpy()] = True
    assert want.any() and np.array_equal(TC.near_tie_rows(xs, ys, gap=5e-3, chunk=64)[0], want)


def test_the_tie_case_has_its_duplicates_where_the_gpu_test_says():
    x, y = TC.tie_case()
    a, b, c = TC.TIE_ROWS
    assert (a, b, c) == (3, 67, 1027) and a // 64 != b // 64 and a // 1024 != c // 1024 and c < x.shape[1]
    assert np.array_equal(x[:, a], x[:, b]) and np.array_equal(x[:, a], x[:, c])
    assert x.shape[1] + y.shape[1] <= CR.CHAMFER_MAX_POINTS                      # chamfer_diff applies
    for r in range(x.shape[0]):
        d32 = ((x[r][None, :, :] - y[r][:, None, :]).astype(np.float32) ** 2).sum(-1)      # (M, N)
        d = CR._dist(CR.T(x[r]), CR.T(y[r]))
        for j in TC.TIE_Y:                                    # nearest to the tripled point, by a wide margin over every other x
            others = np.delete(np.arange(x.shape[1]), [a, b, c])
            assert float(d[j, a]) < 0.25 * float(d[j, others].min()) and float(d[j, a]) > 0
            assert d32[j, a] == d32[j, b] == d32[j, c]
        near = np.sort(d[list(TC.TIE_Y), a].numpy())          # which of them is nearest to the point is no matter of fp32 rounding
        assert np.diff(near).min() > 1e-6 and near.max() < 4e-3
        rest = np.delete(np.arange(y.shape[1]), TC.TIE_Y)     # no other y is nearest to it: the share is exactly TIE_Y's
        assert not np.isin(d[rest].argmin(1).numpy(), [a, b, c]).any()


@pytest.mark.parametrize("By", [1, 3])
def test_the_prefix_embedding_has_the_compact_case_s_value_in_float64(By):
    (x, y), (X, Y, Xm, Ym) = TC.prefix_embedding(By)
    n, m, N, M = TC.PREFIX
    assert X.shape == (3, N, 3) and Y.shape == (By, M, 3) and N + M > CR.CHAMFER_MAX_POINTS and n + m <= CR.CHAMFER_MAX_POINTS
    assert Xm[:, :n].all() and not Xm[:, n:].any() and Ym[:, :m].all() and not Ym[:, m:].any()
    # the same selected points through the same row-by-row path: equal; the unmasked call batches its rows (another sum order)
    compact = CR.chamfer(x, y, np.ones(x.shape[:2], bool), np.ones(y.shape[:2], bool))
    assert torch.equal(CR.chamfer(X, Y, Xm, Ym), compact)
    assert torch.allclose(compact, CR.chamfer(x, y), rtol=1e-14, atol=0)
    (_, _), (Xn, Yn, _, _) = TC.prefix_embedding(By, fill=np.nan)
    assert np.isnan(Xn[:, n:]).all() and np.isnan(Yn[:, m:]).all() and np.array_equal(Xn[:, :n], x)
    assert torch.equal(CR.chamfer(Xn, Yn, Xm, Ym), compact)
