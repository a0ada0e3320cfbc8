"""CPU checks of the cell-list edge builder's grid (tests/cells_restate.py restates ag_cells.hip's index formula): every pair
that passes the reference's exact fp32 test lies within one cell on each axis - attacked with pairs next to cell boundaries and
with distances one ulp around the threshold, at extents from 1e-3 to 1e7 - and the builder restated on that grid equals the
oracle.  Also: the two fixtures of tests/test_gpu_cells.py equal the oracle."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import cells_restate as R
from conftest import GOLDEN
from oracle import adaptigraph_oracle as O

F32 = np.float32
THRS = (0.4, 0.5, 0.75)
SIGNS = [s for s in itertools.product((-1, 0, 1), repeat=3) if any(s)]      # the axes and every diagonal


def thr2_of(thr, single):
    return F32(thr * thr) if single else F32(F32(thr) * F32(thr))            # double product rounded | fp32 product


def nudge(x, k):
    """x moved by k ulps (elementwise)."""
    x = np.array(x, F32)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


def passes(pi, pj, thr2):
    d = (pi - pj).astype(F32)
    sq = (d * d).astype(F32)
    dis = ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)
    return (dis - F32(thr2)).astype(F32) < 0


def adversarial_pairs(rng, lo, hi, thr2, cap, n):
    """Receivers on (and a few ulps around) cell boundaries or anywhere in the box; senders along every axis and diagonal at a
    distance whose dis is within a few ulps of thr2, or anywhere inside the radius.  All inside the box, so the grid of the box
    corners is the grid of the whole set."""
    corners = np.stack([lo, hi]).astype(F32)
    g = R.make_grid(corners, thr2, cap)
    h = 1.0 / float(g["inv_h"]) if g["inv_h"] > 0 else float((hi - lo).max())
    m = np.stack([rng.integers(0, int(g["n"][c]) + 1, n) for c in range(3)], 1)
    on_edge = (lo[None].astype(np.float64) + m * h).astype(F32)
    for k in (-2, -1, 1, 2):
        sel = rng.random(n) < 0.2
        on_edge[sel] = nudge(on_edge[sel], k)
    anywhere = (lo[None] + rng.random((n, 3)) * (hi - lo)[None]).astype(F32)
    pi = np.where(rng.random((n, 1)) < 0.6, on_edge, anywhere)
    pi = np.clip(pi, lo[None], hi[None]).astype(F32)
    s = np.array(SIGNS, np.float64)[rng.integers(0, len(SIGNS), n)]
    d = np.sqrt(float(thr2) / (s != 0).sum(1))
    d = np.where(rng.random(n) < 0.7, nudge(d.astype(F32), 0).astype(np.float64), d * rng.random(n))
    step = d.astype(F32)
    for k in range(-3, 4):
        sel = rng.integers(-3, 4, n) == k
        step[sel] = nudge(step[sel], k)
    pj = (pi + (s * step[:, None]).astype(F32)).astype(F32)
    pj = np.clip(pj, lo[None], hi[None]).astype(F32)
    return g, pi, pj


CONFIGS = [(e, thr, single, cap, neg) for e in (1e-3, 0.05, 1.0, 30.0, 1e3, 1e5, 1e7) for thr in THRS for single in (False, True)
           for cap, neg in ((64, True), (1 << 12, False), (1 << 20, True))]


def test_passing_pairs_are_within_one_cell():
    rng = np.random.default_rng(24)
    n_pass = n_straddle = 0
    for e, thr, single, cap, neg in CONFIGS:
        thr2 = thr2_of(thr, single)
        ext = np.array([e, e * 0.37, e * 1e-3 if e > 1 else e], np.float64)
        lo = (-ext * 0.61 if neg else ext * 0.13).astype(F32)               # negative coordinates | an offset origin
        hi = (lo + ext).astype(F32)
        g, pi, pj = adversarial_pairs(rng, lo, hi, thr2, cap, 4000)
        assert g["ncells"] <= cap and (g["n"] < R.AXIS_MAX).all()
        ci, cj = R.cells_of(pi, g), R.cells_of(pj, g)
        assert ci.min() >= 0 and (ci < g["n"][None]).all() and (cj < g["n"][None]).all()
        ok = passes(pi, pj, thr2)
        apart = np.abs(ci - cj).max(1)
        assert (apart[ok] <= 1).all(), (e, thr, single, cap, int(apart[ok].max()))
        n_pass += int(ok.sum())
        n_straddle += int((ok & (apart == 1)).sum())
    assert n_pass > 50000 and n_straddle > 5000                              # the attack reached what it aims at


def test_the_attack_catches_a_cell_edge_below_the_radius(monkeypatch):
    """Negative control: with the cell edge at 0.999 of the culling radius a passing pair two cells apart is found."""
    monkeypatch.setattr(R, "EDGE_MARGIN", F32(0.999))
    with pytest.raises(AssertionError):
        test_passing_pairs_are_within_one_cell()


@settings(derandomize=True, database=None, deadline=None, max_examples=300)
@given(loge=st.floats(-3, 7), thr=st.sampled_from(THRS), single=st.booleans(), cap=st.sampled_from((64, 1 << 12, 1 << 20)),
       origin=st.floats(-1.0, 0.5), u=st.tuples(*[st.floats(0, 1)] * 3), sign=st.sampled_from(SIGNS), frac=st.floats(0.0, 1.0),
       near=st.booleans(), ulps=st.integers(-4, 4), edge_ulps=st.integers(-2, 2), snap=st.booleans())
def test_pair_within_one_cell_hypothesis(loge, thr, single, cap, origin, u, sign, frac, near, ulps, edge_ulps, snap):
    thr2 = thr2_of(thr, single)
    e = 10.0 ** loge
    lo = np.full(3, origin * e, np.float64).astype(F32)
    hi = (lo + np.array([e, e * 0.5, e * 0.01])).astype(F32)
    g = R.make_grid(np.stack([lo, hi]), thr2, cap)
    pi = (lo + np.array(u) * (hi - lo)).astype(F32)
    if snap and g["inv_h"] > 0:                                              # onto a cell boundary, a few ulps around it
        h = 1.0 / float(g["inv_h"])
        pi = nudge((lo + np.floor((pi - lo) / h) * h).astype(F32), edge_ulps)
    pi = np.clip(pi, lo, hi).astype(F32)
    s = np.array(sign, np.float64)
    d = np.sqrt(float(thr2) / (s != 0).sum())
    d = nudge(F32(d), ulps) if near else F32(d * frac)
    pj = np.clip((pi + (s * d).astype(F32)).astype(F32), lo, hi).astype(F32)
    ci, cj = R.cells_of(pi[None], g)[0], R.cells_of(pj[None], g)[0]
    assert (ci >= 0).all() and (ci < g["n"]).all() and (cj >= 0).all() and (cj < g["n"]).all()
    if R.pair_passes(pi, pj, thr2):
        assert np.abs(ci - cj).max() <= 1


def test_cell_axis_is_monotone_and_in_range():
    rng = np.random.default_rng(5)
    for e in (1e-3, 1.0, 1e4, 1e7):
        lo, hi = F32(-0.3 * e), F32(0.7 * e)
        g = R.make_grid(np.array([[lo] * 3, [hi] * 3], F32), thr2_of(0.5, False), 1 << 20)
        x = np.sort(np.concatenate([rng.uniform(lo, hi, 20000).astype(F32), [lo, hi]]).astype(F32))
        c = R.cell_axis(x, g["lo"][0], g["inv_h"], int(g["n"][0]))
        assert (np.diff(c) >= 0).all() and c[0] == 0 and c[-1] <= g["n"][0] - 1


def test_cull_radius_squares_to_at_least_the_threshold():
    for thr, single in itertools.product(THRS + (1e-20, 3e18), (False, True)):
        thr2 = thr2_of(thr, single)
        r = R.cull_radius(thr2)
        assert F32(r * r) >= thr2


def test_degenerate_thresholds_and_clouds_get_no_grid_or_one_cell():
    pts = np.random.default_rng(1).normal(0, 1, (50, 3)).astype(F32)
    for bad in (0.0, -1.0, np.nan):
        assert R.make_grid(pts, bad, 64)["ncells"] == 0                      # (dis - thr2) < 0 never holds
    assert R.make_grid(pts[:0], 0.25, 64)["ncells"] == 0
    assert R.make_grid(pts, np.inf, 64)["ncells"] == 1                       # every finite pair passes: one cell
    far = np.array([[-3e38, 0, 0], [3e38, 1, 1]], F32)                       # an extent that overflows fp32
    g = R.make_grid(far, 0.25, 1 << 20)
    assert g["n"][0] == 1 and g["ncells"] >= 1


def cloud(rng, N, spread=1.5):
    pos = rng.uniform(-spread, spread, (N, 3)).astype(F32)
    mask = np.ones(N, bool)
    mask[N // 3:N // 3 + N // 10] = False                                    # a masked stretch in the middle
    tool = np.zeros(N, bool)
    tool[[N // 7, N // 2, N - 2]] = True                                     # tools not at the end of the index range
    return pos, mask, tool


@pytest.mark.parametrize("topk", [5, 400])
@pytest.mark.parametrize("cta", [False, True])
def test_restated_builder_equals_the_oracle(topk, cta):
    rng = np.random.default_rng(300 + topk)
    pos, mask, tool = cloud(rng, 300)
    for thr in THRS:
        want = O.construct_edges_single(pos, thr, mask, tool, topk, cta)
        for cap in (None, 64):                                               # the default budget | one that forces larger cells
            got = R.build_edges(pos, thr2_of(thr, False), mask, tool, topk, 1 if cta else 0, cap)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (thr, cap)
        want = O.construct_edges_from_states(pos, thr, mask, tool, topk, cta)
        got = R.build_edges(pos, thr2_of(thr, True), mask, tool, topk, 2 if cta else 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), thr


@pytest.mark.parametrize("topk", [5, 400])
@pytest.mark.parametrize("cta", [False, True])
def test_restated_builder_with_non_finite_coordinates(topk, cta):
    """A valid particle with a NaN / +Inf / -Inf coordinate, in object, masked and tool rows: no radius edge, no self-loop, still
    valid for the connect_tools_all rules - the oracle's (= the reference's) own arithmetic."""
    rng = np.random.default_rng(77)
    pos, mask, tool = cloud(rng, 300, spread=1.0)
    N = len(pos)
    for row, col, v in ((3, 0, np.nan), (40, 1, np.inf), (41, 2, -np.inf), (N // 3 + 2, 0, np.nan), (N // 2, 1, np.inf), (N // 7, 2, np.nan),
                        (200, 0, np.inf), (201, 0, np.inf)):
        pos[row, col] = v
    with np.errstate(invalid="ignore"):
        want = O.construct_edges_single(pos, 0.5, mask, tool, topk, cta)
        got = R.build_edges(pos, thr2_of(0.5, False), mask, tool, topk, 1 if cta else 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert not ((got[0] == 3) & (got[1] == 3)).any()
        want = O.construct_edges_from_states(pos, 0.5, mask, tool, topk, cta)
        got = R.build_edges(pos, thr2_of(0.5, True), mask, tool, topk, 2 if cta else 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name", ["cells_cloth64", "cells_pile"])
def test_fixture_equals_the_oracle(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert g["pos"].shape[0] > 4096 and g["recv"].dtype == np.int32 and g["send"].dtype == np.int32
    recv, send = O.construct_edges_single(g["pos"], float(g["thr"]), g["mask"], g["tool"], int(g["topk"]), bool(g["cta"]), check_ties=True)
    assert np.array_equal(recv, g["recv"]) and np.array_equal(send, g["send"])


def test_cells_library_exports_exactly_its_header():
    """The builder is a library of its own beside the engine's, whose export list stays as it is (tests/test_abi.py)."""
    from adaptigraph_amd import _lib
    root = os.path.dirname(GOLDEN.rstrip(os.sep).rsplit(os.sep, 1)[0])
    raw = open(os.path.join(root, "include", "adaptigraph_amd_cells.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(ag_[a-z_]+)\s*\(", src))) == sorted(_lib.CELLS_EXPORTS)
    assert not set(_lib.CELLS_EXPORTS) & set(_lib.EXPORTS)
    for limit in ("1,048,576", "topk <= 128", "INT32_MAX"):
        assert limit in raw
    if not os.path.exists(_lib.CELLS_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load_cells()
    for name in _lib.CELLS_EXPORTS:
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.CELLS_LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (ag_[a-z_]+)$", out, flags=re.M))) == sorted(_lib.CELLS_EXPORTS)
    assert lib.ag_build_edges_cells(None, None, None, 0, None, None, 1, 1, 0.5, None, None, 5, 0, 10, None, None, None, None) == _lib.AG_ERR_INVALID
