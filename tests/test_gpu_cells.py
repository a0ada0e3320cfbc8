"""GPU checks of the cell-list edge builder (-m gpu): ag_build_edges_cells / construct_edges_cells against the LDS-resident
builder and the numpy oracle where both apply, against lists the reference itself produced above 4096 particles
(tests/golden/make_golden_cells.py), at degenerate geometry, at pairs one ulp around the threshold on cell boundaries, with
non-finite coordinates, at the edge_cap overflow, for determinism, through DynamicsPredictor.forward, and its refusals.
Integer outputs: equal means equal."""
import itertools
import os

import numpy as np
import pytest
import torch

import cells_restate as R
from conftest import GOLDEN
from test_gpu_parity import POS_TOL, _cfg

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ag():
    import adaptigraph_amd
    return adaptigraph_amd


@pytest.fixture(scope="module")
def O():
    from oracle import adaptigraph_oracle
    return adaptigraph_oracle


def t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def cells(ag, dev, pos, thr, mask, tool, topk, cta, single=False, edge_cap=None):
    thr = t(np.asarray(thr, np.float64), dev) if np.ndim(thr) else thr
    return ag.construct_edges_cells(t(pos, dev), thr, t(mask, dev), t(tool, dev), topk, cta, edge_cap=edge_cap, single=single)


def raw_cells(ag, dev, pos, thr_vec, mask, tool, topk, rule, edge_cap):
    """ag_build_edges_cells on outputs filled with a sentinel -> EdgeList of whole tensors."""
    from adaptigraph_amd import _lib
    from adaptigraph_amd.context import default_engine, ptr, current_stream
    from adaptigraph_amd.graph import EdgeList
    eng = default_engine(dev)
    B, N, _ = pos.shape
    out = [torch.full(s, SENTINEL, device=dev, dtype=torch.int32) for s in ((B, edge_cap), (B, edge_cap), (B, N + 1), (B,))]
    p, m, tl, tv = t(pos, dev), t(mask, dev).view(torch.uint8), t(tool, dev).view(torch.uint8), t(np.asarray(thr_vec, F32), dev)
    rc = _lib.load_cells().ag_build_edges_cells(eng.ctx, current_stream(dev), ptr(p), 0, ptr(m), ptr(tl), B, N, 0.0, ptr(tv), None, topk, rule,
                                                edge_cap, *[ptr(o) for o in out])
    assert rc == 0, eng.lib.ag_last_error(eng.ctx)
    torch.cuda.synchronize()
    return EdgeList(*out, N)


def lists(el):
    n = el.n_edges.cpu().numpy()
    r, s = el.recv.cpu().numpy(), el.send.cpu().numpy()
    return [(r[b, :n[b]], s[b, :n[b]]) for b in range(len(n))]


def assert_lists(el, want, what=""):
    """EdgeList against per-graph (recv, send): the lists, the counts, and row_ptr as the receivers imply it."""
    got = lists(el)
    rp = el.row_ptr.cpu().numpy()
    for b, ((gr, gs), (wr, ws)) in enumerate(zip(got, want)):
        assert len(gr) == len(wr), (what, b, len(gr), len(wr))
        assert np.array_equal(gr, wr) and np.array_equal(gs, ws), (what, b)
        assert np.array_equal(rp[b], np.concatenate([[0], np.cumsum(np.bincount(wr, minlength=el.N))])), (what, b)


def batch_cloud(rng, B, N):
    """B graphs: different valid counts, a masked stretch in the middle, tools not at the end of the index range."""
    side = max(0.5, (N / 30.0) ** (1.0 / 3.0))
    pos = rng.uniform(0, side, (B, N, 3)).astype(F32)
    mask = np.ones((B, N), bool)
    tool = np.zeros((B, N), bool)
    for b in range(B):
        mask[b, N // 3:N // 3 + N // 10] = False
        if b:
            mask[b, N - (b * N) // 5:] = False
        for j in {N // 7, N // 2, (2 * N) // 3 + b}:
            if N >= 3 and j < N:
                tool[b, j] = True
    return pos, mask, tool


THR_VEC = np.array([0.4, 0.5, 0.75])


@pytest.mark.parametrize("rule", ["none", "batch", "single"])
@pytest.mark.parametrize("topk", [1, 5, 20, 128])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 301, 1029])
def test_equal_to_the_lds_builder_and_the_oracle(ag, dev, O, N, topk, rule):
    rng = np.random.default_rng(1000 * N + topk)
    B = 3
    pos, mask, tool = batch_cloud(rng, B, N)
    cta, single = rule != "none", rule == "single"
    el = cells(ag, dev, pos, THR_VEC, mask, tool, topk, cta, single=single)
    if single:
        want = [O.construct_edges_from_states(pos[b], THR_VEC[b], mask[b], tool[b], topk, cta) for b in range(B)]
        thr2 = t(np.array([F32(x * x) for x in THR_VEC], F32), dev)
        cull = t(np.nextafter(THR_VEC.astype(F32), F32(np.inf)), dev)
        lds = ag.construct_edges_graphs(t(pos, dev), 0, t(mask, dev).view(torch.uint8), t(tool, dev).view(torch.uint8), thr2, cull, topk, cta,
                                        edge_cap=el.edge_cap)
    else:
        want = O.construct_edges_batch(pos, THR_VEC, mask, tool, topk, cta)
        lds = ag.construct_edges_index(t(pos, dev), t(THR_VEC, dev), t(mask, dev), t(tool, dev), topk, cta, edge_cap=el.edge_cap)
    assert_lists(el, want, "oracle")
    assert torch.equal(el.n_edges, lds.n_edges) and torch.equal(el.row_ptr, lds.row_ptr)
    for (gr, gs), (lr, ls) in zip(lists(el), lists(lds)):
        assert np.array_equal(gr, lr) and np.array_equal(gs, ls)


@pytest.fixture(scope="module")
def cloth64():
    return dict(np.load(os.path.join(GOLDEN, "cells_cloth64.npz")))


@pytest.mark.parametrize("name", ["cells_cloth64", "cells_pile"])
def test_above_the_old_limit_against_the_reference(ag, dev, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert g["pos"].shape[0] > 4096
    el = cells(ag, dev, g["pos"][None], float(g["thr"]), g["mask"][None], g["tool"][None], int(g["topk"]), bool(g["cta"]))
    assert_lists(el, [(g["recv"], g["send"])], name)
    with pytest.raises(NotImplementedError):                                 # and the LDS builder still refuses such a graph
        ag.construct_edges_index(t(g["pos"][None], dev), float(g["thr"]), t(g["mask"][None], dev), t(g["tool"][None], dev),
                                 int(g["topk"]), bool(g["cta"]))


def _degenerate(name):
    rng = np.random.default_rng(31)
    if name == "coincident":                                                 # one cell holds everything; every row is a tie
        N = 5000
        pos = np.tile(np.array([[0.3, -1.2, 2.0]], F32), (N, 1))
    elif name == "line_1e6":                                                 # the cell budget forces a larger cell
        N = 5000
        i = np.arange(N)
        pos = np.stack([1000.0 * (i // 5) + 0.1 * (i % 5), np.zeros(N), np.zeros(N)], 1).astype(F32)
    elif name == "clusters_1e7":
        N = 600
        pos = rng.normal(0, 0.4, (N, 3))
        pos[N // 2:, 0] += 1e7
        pos = pos.astype(F32)
    elif name in ("sheet", "all_masked", "no_tools", "only_tools"):
        n = 40
        ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        pos = np.stack([-5.0 + 0.2 * ii.ravel(), np.zeros(n * n), 0.2 * jj.ravel()], 1)
        pos[:, [0, 2]] += rng.normal(0, 0.01, (n * n, 2))
        pos = pos.astype(F32)
        N = n * n
    mask = np.ones(N, bool)
    tool = np.zeros(N, bool)
    if name == "all_masked":
        mask[:] = False
    if name == "only_tools":
        tool[:] = True
    elif name != "no_tools":
        tool[[N // 5, N // 2]] = True
    return pos, mask, tool


@pytest.mark.parametrize("name", ["coincident", "line_1e6", "clusters_1e7", "sheet", "all_masked", "no_tools", "only_tools"])
def test_degenerate_geometry_against_the_oracle(ag, dev, O, name):
    pos, mask, tool = _degenerate(name)
    want = O.construct_edges_single(pos, 0.5, mask, tool, 5, True)
    assert_lists(cells(ag, dev, pos[None], 0.5, mask[None], tool[None], 5, True), [want], (name, "batch"))
    if len(pos) > 2000:                                                      # (the oracle is dense: one rule at 5000 points)
        return
    want = O.construct_edges_single(pos, 0.5, mask, tool, 5, False)
    assert_lists(cells(ag, dev, pos[None], 0.5, mask[None], tool[None], 5, False), [want], (name, "none"))
    want = O.construct_edges_from_states(pos, 0.5, mask, tool, 5, True)
    assert_lists(cells(ag, dev, pos[None], 0.5, mask[None], tool[None], 5, True, single=True), [want], (name, "single"))


def _straddle(pi, s, thr2):
    """Senders from pi along direction s around the radius: the last two positions (stepping every moving coordinate by one ulp)
    that pass the exact test and the first two that fail it."""
    s = np.array(s, F32)
    d = F32(np.sqrt(float(thr2) / np.abs(s).sum()))
    p = (pi + s * d).astype(F32)
    out = np.where(s > 0, F32(np.inf), F32(-np.inf)).astype(F32)

    def step(q, outward):
        n = np.nextafter(q, out if outward else pi)
        return np.where(s != 0, n, q).astype(F32)
    for _ in range(4096):                                                    # to the last passing position
        if not R.pair_passes(pi, p, thr2):
            p = step(p, False)
        elif R.pair_passes(pi, step(p, True), thr2):
            p = step(p, True)
        else:
            break
    assert R.pair_passes(pi, p, thr2) and not R.pair_passes(pi, step(p, True), thr2)
    return [step(p, False), p, step(p, True), step(step(p, True), True)]


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("thr", [0.4, 0.5, 0.75])
def test_boundary_pairs_against_the_oracle(ag, dev, O, thr, single):
    """Receivers on cell boundaries (tests/cells_restate.py restates the grid); senders along every axis and diagonal one ulp of
    their coordinates below, at and above the distance at which the exact test flips."""
    thr2 = F32(thr * thr) if single else F32(F32(thr) * F32(thr))
    lo = np.array([-3.0, -1.0, 0.5], F32)
    hi = (lo + np.array([6.0, 3.0, 3.0], F32)).astype(F32)
    g = R.make_grid(np.stack([lo, hi]), thr2, 1024)
    assert (g["n"] >= 4).all() and g["ncells"] <= 1024
    h = 1.0 / float(g["inv_h"])
    rng = np.random.default_rng(4)
    signs = [s for s in itertools.product((-1, 0, 1), repeat=3) if any(s)]
    pts = [lo, hi]
    for _ in range(6):
        m = np.array([rng.integers(2, int(g["n"][c]) - 1) for c in range(3)])    # senders stay inside the box: the grid is the box's
        pi = (lo.astype(np.float64) + m * h).astype(F32)
        pts.append(pi)
        for s in signs:
            pts.extend(_straddle(pi, s, thr2))
    pos = np.stack(pts).astype(F32)
    N = len(pos)
    assert R.cells_cap_for(N) == 1024 and (pos >= lo).all() and (pos <= hi).all()
    mask, tool = np.ones(N, bool), np.zeros(N, bool)
    if single:
        want = O.construct_edges_from_states(pos, thr, mask, tool, 128, False)
    else:
        want = O.construct_edges_single(pos, thr, mask, tool, 128, False)
    assert_lists(cells(ag, dev, pos[None], thr, mask[None], tool[None], 128, False, single=single), [want])


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("N,topk", [(300, 5), (120, 128)])
def test_non_finite_coordinates(ag, dev, O, N, topk, single):
    """NaN / +Inf / -Inf in object, masked and tool rows, with top-k active and without: such a particle is in no radius edge and
    stays valid for the connect_tools_all rules; the call returns AG_OK (the wrapper raises otherwise)."""
    rng = np.random.default_rng(77)
    pos = rng.uniform(-1, 1, (N, 3)).astype(F32)
    mask = np.ones(N, bool)
    mask[N // 3:N // 3 + N // 10] = False
    tool = np.zeros(N, bool)
    tool[[N // 7, N // 2, N - 2]] = True
    bad = [(3, 0, np.nan), (40, 1, np.inf), (41, 2, -np.inf), (N // 3 + 2, 0, np.nan), (N // 2, 1, np.inf), (N // 7, 2, np.nan),
           (90, 0, np.inf), (91, 0, np.inf)]
    for row, col, v in bad:
        pos[row, col] = v
    with np.errstate(invalid="ignore"):
        for cta in (False, True):
            want = (O.construct_edges_from_states if single else O.construct_edges_single)(pos, 0.5, mask, tool, topk, cta)
            el = cells(ag, dev, pos[None], 0.5, mask[None], tool[None], topk, cta, single=single)
            assert_lists(el, [want], cta)
            if not cta:
                r, s = lists(el)[0]
                assert len(r) > N and not np.isin(r, [b[0] for b in bad]).any() and not np.isin(s, [b[0] for b in bad]).any()


def test_edge_cap_one_below_the_true_count(ag, dev, O):
    rng = np.random.default_rng(6)
    pos, mask, tool = batch_cloud(rng, 3, 301)
    mask[1] = True                                                           # graph 1 is the densest
    thr = np.array([0.5, 0.5, 0.5])
    want = O.construct_edges_batch(pos, thr, mask, tool, 5, True)
    counts = [len(w[0]) for w in want]
    cap = counts[1] - 1
    assert counts[0] <= cap and counts[2] <= cap
    el = raw_cells(ag, dev, pos, thr, mask, tool, 5, 1, cap)
    assert el.n_edges.cpu().tolist() == counts                               # the true count
    assert (el.recv[1] == SENTINEL).all() and (el.send[1] == SENTINEL).all() and (el.row_ptr[1] == SENTINEL).all()
    for b in (0, 2):
        r, s = el.recv[b].cpu().numpy(), el.send[b].cpu().numpy()
        assert np.array_equal(r[:counts[b]], want[b][0]) and np.array_equal(s[:counts[b]], want[b][1])
        assert (r[counts[b]:] == SENTINEL).all()
        assert el.row_ptr[b, -1].item() == counts[b]


def test_determinism(ag, dev):
    rng = np.random.default_rng(8)
    pos, mask, tool = batch_cloud(rng, 3, 1029)
    other = batch_cloud(rng, 2, 4500)
    thr = np.array([0.4, 0.5, 0.75])
    cap = 1029 * 23
    a = raw_cells(ag, dev, pos, thr, mask, tool, 20, 1, cap)
    b = raw_cells(ag, dev, pos, thr, mask, tool, 20, 1, cap)
    raw_cells(ag, dev, other[0], thr[:2], other[1], other[2], 7, 2, 4500 * 10)   # the workspace is carved for another shape
    c = raw_cells(ag, dev, pos, thr, mask, tool, 20, 1, cap)
    assert int(a.n_edges.min()) > 0
    for x in (b, c):
        assert torch.equal(a.recv, x.recv) and torch.equal(a.send, x.send) and torch.equal(a.row_ptr, x.row_ptr) and \
            torch.equal(a.n_edges, x.n_edges)


def test_forward_on_a_graph_above_the_old_limit(ag, dev, O, cloth64):
    g = cloth64
    rng = np.random.default_rng(3)
    W = O.random_weights(24)
    m = ag.DynamicsPredictor(*_cfg("rope", 3), dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})
    B, N = 2, g["pos"].shape[0]
    N_o = N - 1
    state = np.tile(g["pos"][None, None], (B, 4, 1, 1)).astype(F32)
    state[:, :3] += rng.normal(0, 0.01, (B, 3, N, 3)).astype(F32)           # both graphs end on the fixture's frame
    attrs = np.zeros((B, N, 2), F32)
    attrs[:, :N_o, 0] = 1
    attrs[:, N_o:, 1] = 1
    action = np.zeros((B, N, 3), F32)
    action[:, N_o:] = [[0.05, 0.0, -0.03]]
    p_inst = np.ones((B, N_o, 1), F32)
    phys = np.array([[0.3], [0.7]], F32)
    mask, tool = np.tile(g["mask"][None], (B, 1)), np.tile(g["tool"][None], (B, 1))
    el = cells(ag, dev, state[:, -1], float(g["thr"]), mask, tool, int(g["topk"]), bool(g["cta"]))
    assert_lists(el, [(g["recv"], g["send"])] * B)
    E = len(g["recv"])
    recv = torch.zeros((B, el.edge_cap), device=dev, dtype=torch.int32)
    send = torch.zeros((B, el.edge_cap), device=dev, dtype=torch.int32)
    recv[:, :E], send[:, :E] = t(g["recv"], dev), t(g["send"], dev)
    rp = np.concatenate([[0], np.cumsum(np.bincount(g["recv"], minlength=N))]).astype(np.int32)
    fix = ag.EdgeList(recv, send, t(np.tile(rp[None], (B, 1)), dev), torch.full((B,), E, device=dev, dtype=torch.int32), N)
    kw = dict(state=t(state, dev), attrs=t(attrs, dev), p_instance=t(p_inst, dev), action=t(action, dev), rope_physics_param=t(phys, dev))
    pos, mot = m(edges=el, **kw)
    pos2, mot2 = m(edges=fix, **kw)
    assert torch.equal(pos, pos2) and torch.equal(mot, mot2)
    want_pos, want_mot = O.model_forward(W, state, attrs, [(g["recv"], g["send"])] * B, p_inst, action, phys, 3)
    assert np.abs(pos.cpu().numpy() - want_pos).max() <= POS_TOL
    assert np.abs(mot.cpu().numpy() - want_mot).max() <= POS_TOL


def test_refusals(ag, dev):
    pos = torch.zeros((1, 200, 3), device=dev)
    ones, zeros = torch.ones((1, 200), device=dev, dtype=torch.bool), torch.zeros((1, 200), device=dev, dtype=torch.bool)
    with pytest.raises(NotImplementedError, match="128"):
        ag.construct_edges_cells(pos, 0.5, ones, zeros, topk=129)
    big = 1048577
    with pytest.raises(NotImplementedError, match="1048576"):
        ag.construct_edges_cells(torch.zeros((1, big, 3), device=dev), 0.5, torch.ones((1, big), device=dev, dtype=torch.bool),
                                 torch.zeros((1, big), device=dev, dtype=torch.bool), topk=5, edge_cap=16)
    with pytest.raises(NotImplementedError, match="int32"):
        ag.construct_edges_cells(torch.zeros((1, 1 << 20, 3), device=dev), 0.5, torch.ones((1, 1 << 20), device=dev, dtype=torch.bool),
                                 torch.ones((1, 1 << 20), device=dev, dtype=torch.bool), topk=5)
    with pytest.raises(NotImplementedError):                                 # the LDS builder keeps its limit
        ag.construct_edges_index(torch.zeros((1, 5000, 3), device=dev), 0.5, torch.ones((1, 5000), device=dev, dtype=torch.bool),
                                 torch.zeros((1, 5000), device=dev, dtype=torch.bool), topk=5)


def test_forward_refuses_a_graph_beyond_its_row_offsets(ag, dev, O):
    """ag_forward addresses activation rows with 32-bit element offsets: a single graph whose edge_cap (rounded up to 256)
    exceeds 2^32 / 160 - 512 = 26,843,033 slots is refused before anything is enqueued (the arrays are never read)."""
    from adaptigraph_amd import _lib
    from adaptigraph_amd.context import ptr, current_stream
    m = ag.DynamicsPredictor(*_cfg("rope", 3), dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_weights(1).items()})
    eng = m.engine()                                                         # the model's context, weights uploaded
    x = torch.zeros(256, device=dev)
    i = torch.zeros(64, device=dev, dtype=torch.int32)
    call = lambda cap: eng.lib.ag_forward(eng.ctx, current_stream(dev), ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), 1, ptr(i), ptr(i),   # noqa: E731
                                          ptr(i), ptr(i), cap, 1, 4, 3, ptr(x), ptr(x))
    assert call(26843034) == _lib.AG_ERR_UNSUPPORTED
    assert b"26843033" in eng.lib.ag_last_error(eng.ctx)
    assert call(2 ** 31 - 1) == _lib.AG_ERR_UNSUPPORTED
