"""CPU checks of the cell-pruned farthest-point sampler: its numpy restatement (tests/fps_grid_restate.py) against the brute-force
sweeps of tests/dataset_restate.py - integer indices only, no tolerance -, the proof obligation of DESIGN.md section 3.27 on fp32
directly, and the host side of ag_fps_cloud_grid: exports, header, package names, refusals without a device."""
import os
import re

import numpy as np
import pytest
import torch

import dataset_restate as DR
import fps_grid_restate as GR
from adaptigraph_amd import perception as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _sheet(n, rng):
    return (rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]).astype(F32)


def _lattice(n, pitch):
    side = int(round(n ** 0.5))
    assert side * side == n
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)
    return np.stack([g[:, 0] * pitch, np.zeros(n), g[:, 1] * pitch], 1).astype(F32)


def _cloud(kind, n, rng):
    if kind == "sheet":
        return _sheet(n, rng)
    if kind == "flat":                                       # zero y extent
        c = _sheet(n, rng)
        c[:, 1] = F32(0.25)
        return c
    if kind == "line":
        return (np.linspace(0, 1, n)[:, None] * [1.0, 0.0, 0.0] + [0.5, 2.0, -1.0]).astype(F32)
    if kind == "repeat":
        return np.repeat(rng.normal(size=(1, 3)), n, 0).astype(F32)
    if kind == "lattice":
        return _lattice(n, 0.05)
    if kind == "dup4":                                       # every point four times
        return np.tile(_sheet(n // 4, rng), (4, 1))
    raise KeyError(kind)


CASES = [("sheet", 3000, 1025, 0.05), ("sheet", 1025, 1025, 0.0), ("sheet", 700, 1025, 0.02), ("sheet", 20000, 4097, 0.02),
         ("sheet", 4000, 1025, 100.0), ("flat", 5000, 2049, 0.03), ("line", 2500, 1100, 0.001), ("repeat", 1500, 1025, 0.2),
         ("repeat", 1500, 1025, 0.0), ("lattice", 4900, 2049, 0.05), ("lattice", 4900, 2049, 0.0500001), ("dup4", 6000, 1500, 0.01),
         ("sheet", 1, 1025, 0.1), ("sheet", 2, 1025, 0.1)]


@pytest.mark.parametrize("kind,n,max_nobj,radius", CASES)
def test_pruned_selection_equals_the_brute_force_sweep(kind, n, max_nobj, radius):
    rng = np.random.default_rng(n + max_nobj)
    c = _cloud(kind, n, rng)
    fps_start, rad_start = int(rng.integers(n)), int(rng.integers(min(n, max_nobj)))
    want = DR.fps_indices(c, max_nobj, fps_start, radius, rad_start)
    stats = {}
    got = GR.fps_indices(c, max_nobj, fps_start, radius, rad_start, stats=stats)
    assert np.array_equal(got, want), (kind, n, max_nobj, radius, len(got), len(want))
    if n <= 5000:                                            # and the partition never enters the result
        for cells in (1, 2, 64):
            assert np.array_equal(GR.fps_indices(c, max_nobj, fps_start, radius, rad_start, cells=cells), want), cells
    if kind == "sheet" and n == 20000:                       # the point of it: far fewer distance evaluations than the sweeps' n per pick
        assert stats["evals"] * 8 < (4097 + len(want)) * n


def test_the_bound_never_exceeds_a_member_s_fp32_distance():
    """The proof obligation, on the numbers: for cells of random members at several scales and offsets, and centres outside, inside,
    on a box face and equal to a member, the fp32 bound is <= the fp32 distance of EVERY member, squared and after the square root."""
    rng = np.random.default_rng(0)
    for trial in range(400):
        scale, shift = 10.0 ** rng.integers(-6, 7), 10.0 ** rng.integers(-3, 6) * rng.normal(size=3)
        m = (rng.normal(size=(int(rng.integers(1, 40)), 3)) * scale + shift).astype(F32)
        lo, hi = m.min(0), m.max(0)
        far = (shift + rng.normal(size=3) * scale * 10.0 ** rng.integers(-2, 4)).astype(F32)
        face = far.copy()
        face[trial % 3] = lo[trial % 3] if trial & 1 else hi[trial % 3]
        nudged = np.nextafter(lo, F32(-np.inf)) if trial & 2 else np.nextafter(hi, F32(np.inf))
        for c in (far, face, m[trial % len(m)].copy(), nudged.astype(F32), ((lo + hi) * F32(0.5)).astype(F32)):
            for stage2 in (False, True):
                b = GR.cell_bound(lo[None], hi[None], c, stage2)[0]
                d = GR.sq_dist(m, c)
                d = np.sqrt(d) if stage2 else d
                assert (b <= d).all(), (trial, stage2, b, d.min())
    # a centre that is a member has bound 0; a NaN or infinite centre never yields a bound above a comparable distance
    m = rng.normal(size=(9, 3)).astype(F32)
    assert GR.cell_bound(m.min(0)[None], m.max(0)[None], m[3], False)[0] == 0
    for bad in (np.nan, np.inf, -np.inf):
        c = np.array([bad, 0.1, 0.2], F32)
        with np.errstate(invalid="ignore", over="ignore"):
            b, d = GR.cell_bound(m.min(0)[None], m.max(0)[None], c, False)[0], GR.sq_dist(m, c)
        assert (np.isnan(d) | (b <= d)).all()


def test_non_finite_points_are_swept_like_the_brute_force_sweep():
    """A NaN or infinite coordinate: the brute-force kernel's `md > d ? d : md` never lowers such a point's minimum, so it keeps
    1e10 and is picked again and again from the moment the lowest such index is reached; the pruned selection does the same for
    every cell count."""
    rng = np.random.default_rng(5)
    c = _sheet(600, rng)
    c[77, 1] = np.nan
    c[300, 0] = np.inf
    outs = [GR.fps_indices(c, 50, 3, 0.0, 0, cells=k) for k in (1, 8, None)]
    assert all(np.array_equal(o, outs[0]) for o in outs)
    assert (GR.fps_stage1(c, 50, 3, cells=8)[1:] == 77).all()


# ------------------------------------------------------------------------------------------------ host side
def test_export_header_and_package_names():
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    assert "ag_fps_cloud_grid" in _lib.CELLS_EXPORTS and "ag_fps_cloud_grid" not in _lib.EXPORTS
    h = open(os.path.join(ROOT, "include", "adaptigraph_amd_cells.h")).read()
    assert re.search(r"\bint ag_fps_cloud_grid\s*\(", h) and "65,536" in h and "1,048,576" in h
    for name in ("fps_cloud_grid", "construct_graph_grid", "state_cur_from_points_grid"):
        assert name in ag.__all__ and callable(getattr(ag, name))
    assert P.GRID_MAX_NOBJ == 65536 and (P.GRID_CELL_POINTS, P.GRID_MAX_CELLS) == (GR.CELL_POINTS, GR.MAX_CELLS)
    src = open(os.path.join(ROOT, "adaptigraph_amd", "csrc", "ag_fps_grid.h")).read()
    for name, value in (("FPS_GRID_MAX_NOBJ", "1 << 16"), ("FPS_GRID_MAX_POINTS", "1 << 20"), ("FPS_GRID_CELL_POINTS", "64"),
                        ("FPS_GRID_MAX_CELLS", "1 << 14")):
        assert re.search(rf"\b{name} = {re.escape(value)}\b", src), name


class _Shape:                                                # a shape is all a refusal may look at
    def __init__(self, *shape):
        self.shape = shape


def test_refusals_come_from_shapes_alone():
    z = _Shape(4, 3)
    with pytest.raises(NotImplementedError, match="65536"):
        P.fps_cloud_grid(z, z, z, z, z, z, 65537, 4)
    with pytest.raises(NotImplementedError, match="1048576"):
        P.fps_cloud_grid(z, z, z, z, z, z, 100, (1 << 20) + 1)
    with pytest.raises(ValueError, match="cells"):
        P.fps_cloud_grid(z, z, z, z, z, z, 100, 4, cells=3)
    with pytest.raises(NotImplementedError, match="65536"):
        P.construct_graph_grid(_Shape(70000, 3), 0.1, max_nobj=65537, device="cuda:0", draws=[(0, 0)])
    with pytest.raises(NotImplementedError, match="1048576"):
        P.construct_graph_grid(_Shape((1 << 20) + 1, 3), 0.1, max_nobj=2000, device="cuda:0", draws=[(0, 0)])
    with pytest.raises(NotImplementedError, match="1048576"):
        P.state_cur_from_points_grid(_Shape((1 << 20) + 1, 3), 10, max_nobj=4097, device="cuda:0")
    with pytest.raises(NotImplementedError, match="65536"):
        P.state_cur_from_points_grid(_Shape(5000, 3), 10, max_nobj=65537, device="cuda:0")
    with pytest.raises(NotImplementedError, match="1024"):   # the old entries keep their limit and message
        P.construct_graph(_Shape(5000, 3), 0.1, max_nobj=1025, device="cuda:0", draws=[(0, 0)])


def test_cpu_tensors_get_the_no_cpu_fallback_error():
    z = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.fps_cloud_grid(torch.zeros(4, 3), z, z, z.int(), z.float(), z.int(), 2000, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.construct_graph_grid(np.zeros((4, 3), np.float32), 0.1, max_nobj=2000, device="cpu", draws=[(0, 0)])
