"""GPU checks (-m gpu) of the batched two-closest-planes rule: ag_edges_surface_rule_graphs against the one-graph path
(construct_edges_from_states with connect_tools_surface and all six bounds), its guards, and rollout_eval_batch on a surface config
against the reference's own rollouts (tests/golden/eval_batch_surface.npz), against the graph-by-graph path, and - for the configs
without the rule - against the fixtures that pinned them before."""
import os

import numpy as np
import pytest
import torch

import surface_restate as SR

pytestmark = pytest.mark.gpu

F32 = np.float32
TOPK = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the kernel against the one-graph path
def host_bounds(rows, padded, ratio, order):
    """The six bounds as the package's own host functions form them (rollout.surface_bounds: the step loop's order;
    dataset.start_graph_bounds: construct_graph's); no row at all: NaN (the device's empty subset)."""
    from adaptigraph_amd.dataset import start_graph_bounds
    from adaptigraph_amd.rollout import surface_bounds
    if padded:
        rows = np.concatenate([rows, np.zeros((1, 3), F32)])
    if len(rows) == 0:
        return {k: F32(np.nan) for k in SR.BOUND_KEYS}
    with np.errstate(invalid="ignore"):
        b = (start_graph_bounds if order else surface_bounds)(rows, ratio)
    assert all(isinstance(b[k], np.float32) for k in SR.BOUND_KEYS)
    return b


def make_batch(No, M, B, ratio, padded, order, chained, seed, nan_graph=None):
    """B graphs of No object rows + M tool rows (the tools behind the objects) with ragged n_obj, jittered clouds in a box of
    1 x 0.5 x 1 with its low corner at (0.5, 0.5, 0.5), the tools inside it.  Kinds: b % 5 == 1 no tool contact (the tool rows are
    masked out); 2 the bounds rows lie 10 above the positions on every axis (ratio 0.8: the max planes are the closest and nothing
    reaches them, S empty; ratio 1.0: the min planes are, S = every valid particle); 3 the bounds rows lie 10 below (S = every valid
    particle, the tools included).  kNN (used when chained) cycles through 1.0, 0.5 and 0.7.  nan_graph: that graph's first
    bounds row has a NaN x."""
    rng = np.random.default_rng(seed)
    N = No + M
    pos = np.zeros((B, N, 3), F32)
    mask = np.zeros((B, N), bool)
    tool = np.zeros((B, N), bool)
    tool[:, No:] = True
    n_obj = np.zeros(B, np.int32)
    bnd = np.zeros((B * No + 1, 3), F32)
    first = np.arange(B, dtype=np.int64) * No
    adj, kNN, bounds = np.zeros(B), np.ones(B), []
    for b in range(B):
        kind = b % 5
        n = No if b == 0 else int(rng.integers(0, No + 1))
        cloud = F32(0.5) + rng.uniform(0, 1, (No, 3)).astype(F32) * F32([1.0, 0.5, 1.0])
        pos[b, :n] = cloud[:n]
        pos[b, No:] = F32(0.5) + rng.uniform(0.3, 0.7, (M, 3)).astype(F32) * F32([1.0, 0.5, 1.0])
        rows = cloud[:n].copy()
        if kind == 2:
            rows += F32(10.0)
        if kind == 3:
            rows -= F32(10.0)
        if nan_graph == b and n:
            rows[0, 0] = np.nan
        bnd[first[b]:first[b] + n] = rows
        mask[b, :n] = True
        mask[b, No:] = kind != 1
        n_obj[b] = n
        adj[b] = rng.uniform(0.25, 0.45)
        kNN[b] = [1.0, 0.5, 0.7][b % 3] if chained else 1.0
        bounds.append(host_bounds(rows, padded and No > n, ratio, order))
    return dict(No=No, M=M, B=B, N=N, pos=pos, mask=mask, tool=tool, n_obj=n_obj, bnd=bnd, first=first, adj=adj, kNN=kNN, bounds=bounds,
                ratio=ratio, pad_rows=No if padded else 0, order=order, chained=chained)


def upload(c, dev, sel=None):
    o = np.arange(c["B"]) if sel is None else np.asarray(sel)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[o])).to(dev)   # noqa: E731
    adj = c["adj"][o]
    return dict(pos=t(c["pos"]), mask=t(c["mask"]).view(torch.uint8), tool=t(c["tool"]).view(torch.uint8), kNN=t(c["kNN"]),
                first=t(c["first"]), n=t(c["n_obj"]), thr2=torch.from_numpy((adj * adj).astype(F32)).to(dev),
                cull=torch.from_numpy(np.nextafter(np.abs(adj).astype(F32), F32(np.inf))).to(dev), bnd=torch.from_numpy(c["bnd"]).to(dev))


def run_rule(ag, c, d, edge_cap=None, n_tools=None, sentinel=None):
    """base build -> (the non-fixed rule when chained) -> the surface launch.  -> (input EdgeList, out, d_bounds, d_planes)."""
    B, N, M = d["mask"].shape[0], c["N"], c["M"]
    dev = d["pos"].device
    wide = max(1, N * (min(TOPK, N) + M))
    el = ag.construct_edges_graphs(d["pos"], 0, d["mask"], d["tool"], d["thr2"], d["cull"], TOPK, False, edge_cap=wide)
    if c["chained"]:
        el = ag.nonfixed_rule_graphs(d["pos"], 0, d["mask"], d["tool"], el, M, d["kNN"], d["bnd"], d["first"], None, d["n"], c["pad_rows"],
                                     c["ratio"], wide)
    cap = wide if edge_cap is None else edge_cap
    out = None
    if sentinel is not None:
        full = lambda *s: torch.full(s, sentinel, dtype=torch.int32, device=dev)   # noqa: E731
        out = ag.EdgeList(full(B, cap), full(B, cap), full(B, N + 1), full(B), N)
    bd = torch.full((B, 6), 7.0, dtype=torch.float32, device=dev)
    pl = torch.full((B, 2), 7, dtype=torch.int32, device=dev)
    out = ag.surface_rule_graphs(d["pos"], 0, d["mask"], d["tool"], el, M if n_tools is None else n_tools, d["bnd"], d["first"], None,
                                 d["n"], c["pad_rows"], c["ratio"], c["order"], cap, out=out, bounds_out=bd, planes_out=pl)
    return el, out, bd, pl


def lists(el):
    return el.n_edges.cpu().numpy(), el.recv.cpu().numpy(), el.send.cpu().numpy(), el.row_ptr.cpu().numpy()


def partner(ag, c, dev, b):
    el = ag.construct_edges_from_states(torch.from_numpy(c["pos"][b]).to(dev), float(c["adj"][b]), torch.from_numpy(c["mask"][b]).to(dev),
                                        torch.from_numpy(c["tool"][b]).to(dev), topk=TOPK, connect_tools_all=False,
                                        connect_tools_surface=True, connect_tool_all_non_fixed=c["chained"], kNN=float(c["kNN"][b]),
                                        as_index=True, **c["bounds"][b])
    n, r, s, rp = lists(el)
    return int(n[0]), r[0, :n[0]], s[0, :n[0]], rp[0]


def restated(c, b):
    """tests/surface_restate.py on graph b: the host's planes, subset and contact count."""
    n = int(c["n_obj"][b])
    rows = c["bnd"][c["first"][b]:c["first"][b] + n]
    return SR.chained(c["pos"][b], float(c["adj"][b]), c["mask"][b], c["tool"][b], TOPK, False, c["chained"], float(c["kNN"][b]), rows,
                      c["pad_rows"], c["ratio"], c["order"])


SIZES = [(2, 1), (24, 2), (300, 5)]
MODES = [(1.0, True, 0, False), (0.8, False, 1, True), (0.8, True, 0, True), (1.0, False, 1, False), (0.8, True, 1, False),
         (0.8, False, 0, False)]                                          # ratio, padded, bounds order, chained behind the non-fixed rule
CASES = [(si, mi) for si in range(len(SIZES)) for mi in range(len(MODES))]


def test_the_cases_cover_every_kind_of_graph():
    """By the restatement the B = 5 batches hold, with tool contact: an empty subset, a subset of every valid particle, one that adds
    and one that removes an edge; without contact: a copied graph.  Both ratios, padded and unpadded, both orders, chained and not."""
    assert {m[0] for m in MODES} == {1.0, 0.8} and {m[1] for m in MODES} == {True, False} and {m[2] for m in MODES} == {0, 1}
    assert {m[3] for m in MODES} == {True, False}
    seen = set()
    for si, mi in CASES:
        c = make_batch(*SIZES[si], 5, *MODES[mi], seed=100 * si + mi)
        for b in range(5):
            g = restated(c, b)
            if g["check"] == 0:
                seen.add("copied")
                continue
            before, after = set(zip(*map(np.ndarray.tolist, g["mid"]))), set(zip(g["recv"].tolist(), g["send"].tolist()))
            seen |= {"empty"} if not g["S"].any() else set()
            seen |= {"all"} if (g["S"] == c["mask"][b]).all() and g["S"].any() else set()
            seen |= {"adds"} if after - before else set()
            seen |= {"removes"} if before - after else set()
    assert seen == {"copied", "empty", "all", "adds", "removes"}, seen


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("si,mi", CASES, ids=[f"{SIZES[s][0]}+{SIZES[s][1]}-r{MODES[m][0]}-pad{int(MODES[m][1])}-o{MODES[m][2]}-ch{int(MODES[m][3])}"
                                              for s, m in CASES])
def test_the_batched_surface_rule_equals_the_one_graph_path(dev, si, mi, B):
    """recv, send, row_ptr and n_edges of every graph bit-equal to construct_edges_from_states(..., as_index=True,
    connect_tools_surface=True, six bounds); d_bounds equal to the host's six bounds, d_planes to the host's choice; a permuted batch
    and B = 1 slices bit-equal to the batch."""
    import adaptigraph_amd as ag
    c = make_batch(*SIZES[si], B, *MODES[mi], seed=100 * si + mi)
    d = upload(c, dev)
    _, out, bd, pl = run_rule(ag, c, d)
    n, r, s, rp = lists(out)
    bd, pl = bd.cpu().numpy(), pl.cpu().numpy()
    for b in range(B):
        want_bd = np.array([c["bounds"][b][k] for k in SR.BOUND_KEYS], F32)
        assert np.array_equal(bd[b], want_bd, equal_nan=True), (b, bd[b], want_bd)
        g = restated(c, b)
        assert tuple(pl[b]) == tuple(g["planes"]), (b, pl[b], g["planes"])
        wn, wr, ws, wrp = partner(ag, c, dev, b)
        assert n[b] == wn, (b, n[b], wn)
        assert np.array_equal(r[b, :wn], wr) and np.array_equal(s[b, :wn], ws) and np.array_equal(rp[b], wrp), b
        assert np.array_equal(wr, g["recv"]) and np.array_equal(ws, g["send"]), b          # (the restatement agrees too)
    if B > 1:
        perm = np.random.default_rng(si).permutation(B)
        _, outp, bdp, plp = run_rule(ag, c, upload(c, dev, perm))
        n2, r2, s2, rp2 = lists(outp)
        assert np.array_equal(n2, n[perm]) and np.array_equal(rp2, rp[perm]) and np.array_equal(plp.cpu().numpy(), pl[perm])
        assert np.array_equal(bdp.cpu().numpy(), bd[perm], equal_nan=True)
        for j, b in enumerate(perm):
            assert np.array_equal(r2[j, :n[b]], r[b, :n[b]]) and np.array_equal(s2[j, :n[b]], s[b, :n[b]]), b
        for b in range(B):
            _, o1, bd1, pl1 = run_rule(ag, c, upload(c, dev, [b]))
            n1, r1, s1, rp1 = lists(o1)
            assert n1[0] == n[b] and np.array_equal(rp1[0], rp[b]) and np.array_equal(pl1.cpu().numpy()[0], pl[b])
            assert np.array_equal(r1[0, :n[b]], r[b, :n[b]]) and np.array_equal(s1[0, :n[b]], s[b, :n[b]]), b


def test_rows_striped_two_per_thread_equal_the_one_graph_path(dev):
    """1023 + 2 particles: a 1024-thread workgroup owns two rows per thread, its last busy thread one, the rest none.  Three graphs
    of a 5-graph batch behind the non-fixed rule: every particle valid, S = every valid particle, and a kNN of 0.5."""
    import adaptigraph_amd as ag
    c = make_batch(1023, 2, 5, 0.8, True, 0, True, seed=41)
    sel = [0, 3, 4]
    assert all(c["n_obj"][b] > 400 for b in sel) and c["kNN"][4] == 0.5
    _, out, bd, _ = run_rule(ag, c, upload(c, dev, sel))
    n, r, s, rp = lists(out)
    bd = bd.cpu().numpy()
    for j, b in enumerate(sel):
        assert np.array_equal(bd[j], np.array([c["bounds"][b][k] for k in SR.BOUND_KEYS], F32), equal_nan=True), b
        wn, wr, ws, wrp = partner(ag, c, dev, b)
        assert n[j] == wn, (b, n[j], wn)
        assert np.array_equal(r[j, :wn], wr) and np.array_equal(s[j, :wn], ws) and np.array_equal(rp[j], wrp), b


@pytest.mark.parametrize("chained", [False, True])
def test_rule_attempt_chains_the_two_launches(dev, chained):
    import adaptigraph_amd as ag
    c = make_batch(24, 2, 5, 0.8, True, 1, chained, seed=3)
    d = upload(c, dev)
    _, want, _, _ = run_rule(ag, c, d)
    wide = c["N"] * (TOPK + c["M"])
    base = ag.construct_edges_graphs(d["pos"], 0, d["mask"], d["tool"], d["thr2"], d["cull"], TOPK, False, edge_cap=wide)
    cfg = ag.RuleConfig(chained, c["M"], c["ratio"], False, surface=True, bounds_order=1)
    got = ag.rule_attempt(cfg, d["pos"], 0, d["mask"], d["tool"], base, d["kNN"], (d["bnd"], d["first"], None, d["n"], c["pad_rows"]), wide)
    n, r, s, rp = lists(want)
    n2, r2, s2, rp2 = lists(got)
    assert np.array_equal(n, n2) and np.array_equal(rp, rp2)
    for b in range(5):
        assert np.array_equal(r[b, :n[b]], r2[b, :n[b]]) and np.array_equal(s[b, :n[b]], s2[b, :n[b]])


def test_a_nan_bounds_row_behaves_as_the_one_graph_path_does(dev):
    import adaptigraph_amd as ag
    c = make_batch(24, 2, 5, 0.8, False, 0, False, seed=4, nan_graph=0)
    assert np.isnan(c["bounds"][0]["max_x"]) and np.isnan(c["bounds"][0]["min_x"]) and not np.isnan(c["bounds"][0]["max_y"])
    d = upload(c, dev)
    _, out, bd, pl = run_rule(ag, c, d)
    n, r, s, rp = lists(out)
    for b in range(5):
        wn, wr, ws, wrp = partner(ag, c, dev, b)
        assert n[b] == wn and np.array_equal(r[b, :wn], wr) and np.array_equal(s[b, :wn], ws) and np.array_equal(rp[b], wrp), b
    assert np.array_equal(bd.cpu().numpy()[0], np.array([c["bounds"][0][k] for k in SR.BOUND_KEYS], F32), equal_nan=True)
    assert restated(c, 0)["check"] > 0                                   # the rule did apply on graph 0


# ------------------------------------------------------------------------------------------------ 2. guards
def test_a_wrong_tool_count_is_refused_per_graph_and_raises_where_the_count_is_read(dev):
    import adaptigraph_amd as ag
    c = make_batch(24, 2, 3, 1.0, True, 0, False, seed=6)
    c["tool"][1, 0] = True                                               # graph 1 alone has three tool particles
    _, out, bd, pl = run_rule(ag, c, upload(c, dev), sentinel=-7)
    n, r, s, rp = lists(out)
    assert n[1] == -1 and (r[1] == -7).all() and (s[1] == -7).all() and (rp[1] == -7).all()
    assert (bd.cpu().numpy()[1] == 7.0).all() and (pl.cpu().numpy()[1] == 7).all()
    assert n[0] >= 0 and n[2] >= 0 and rp[0][-1] == n[0] and rp[2][-1] == n[2]
    plan = ag.BackoffPlan([1.0] * 3, TOPK, 10000)
    with pytest.raises(RuntimeError, match="internal"):
        plan.record(n)


def test_a_graph_over_edge_cap_reports_its_count_and_writes_nothing(dev):
    import adaptigraph_amd as ag
    c = make_batch(24, 2, 5, 1.0, True, 0, False, seed=5)
    d = upload(c, dev)
    _, full, _, _ = run_rule(ag, c, d)
    n, r, s, rp = lists(full)
    cap = int(n.max()) - 1
    assert cap >= 1 and (n <= cap).any()
    _, out, _, _ = run_rule(ag, c, d, edge_cap=cap, sentinel=-7)
    n2, r2, s2, rp2 = lists(out)
    assert np.array_equal(n2, n)                                         # the TRUE counts
    for b in range(5):
        if n[b] > cap:
            assert (r2[b] == -7).all() and (s2[b] == -7).all() and (rp2[b] == -7).all(), b
        else:
            assert np.array_equal(r2[b, :n[b]], r[b, :n[b]]) and np.array_equal(s2[b, :n[b]], s[b, :n[b]]) and np.array_equal(rp2[b], rp[b])
            assert (r2[b, n[b]:] == -7).all() and (s2[b, n[b]:] == -7).all()


def test_above_the_size_limit_the_call_is_refused_before_any_launch(dev):
    import adaptigraph_amd as ag
    from adaptigraph_amd.graph import surface_graphs_limit
    N = 4097
    assert surface_graphs_limit(N, 1) is not None and surface_graphs_limit(4096, 64) is None and surface_graphs_limit(10, 65) is not None
    z = lambda *sh, dt=torch.int32: torch.zeros(sh, dtype=dt, device=dev)    # noqa: E731
    base = ag.EdgeList(z(1, 8), z(1, 8), z(1, N + 1), z(1), N)
    out = ag.EdgeList(torch.full((1, 8), -7, dtype=torch.int32, device=dev), z(1, 8), z(1, N + 1), torch.full((1,), -7, dtype=torch.int32, device=dev), N)
    with pytest.raises(NotImplementedError, match="4096"):
        ag.surface_rule_graphs(z(1, N, 3, dt=torch.float32), 0, z(1, N, dt=torch.uint8), z(1, N, dt=torch.uint8), base, 1,
                               z(4, 3, dt=torch.float32), z(1, dt=torch.int64), None, z(1), 0, 1.0, 0, 8, out=out)
    torch.cuda.synchronize()
    assert out.n_edges.item() == -7 and (out.recv == -7).all()


def test_the_surface_launch_does_not_wait_for_the_gpu(dev):
    """ag_edges_surface_rule_graphs only enqueues: it returns while an earlier kernel still spins on the stream."""
    import adaptigraph_amd as ag
    c = make_batch(24, 2, 3, 1.0, True, 0, False, seed=8)
    d = upload(c, dev)
    base, want, _, _ = run_rule(ag, c, d)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    ms_per_cycle = e0.elapsed_time(e1) / 10_000_000
    done = torch.cuda.Event()
    torch.cuda._sleep(int(200.0 / ms_per_cycle))
    done.record()
    out = ag.surface_rule_graphs(d["pos"], 0, d["mask"], d["tool"], base, 2, d["bnd"], d["first"], None, d["n"], c["pad_rows"], c["ratio"],
                                 0, want.edge_cap)
    still_busy = not done.query()
    torch.cuda.synchronize()
    assert still_busy, "ag_edges_surface_rule_graphs waited for the GPU"
    assert torch.equal(out.n_edges, want.n_edges)


# ------------------------------------------------------------------------------------------------ 3. the fixture
_EVAL = {}


def _eval_case(dev, name="eval_batch_surface"):
    import adaptigraph_amd as ag
    import eval_restate as ER
    import train_restate as TR
    from test_gpu_train import _model
    if name not in _EVAL:
        fx = ER.load_fixture(name)
        ds = ag.DeviceDynDataset(*ER.dataset_args(fx), device=dev, phase="valid")
        nh = ds.spec.n_his
        model = _model(dev, TR.make_weights(fx["w_seed"], n_his=nh), n_his=nh, pstep=3 if name == "eval_batch_rope" else 4,
                       material=fx["material"])
        dr = ds.eval_draws(fx["samples"], fps_start=fx["fps_start"], rad_start=fx["rad_start"])
        _EVAL[name] = (fx, ds, model, dr, ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr, keep_pred=True))
    return _EVAL[name]


def _edges_at(res, s, b):
    e = res.edges[s]
    n = int(e.n_edges[b])
    return e.recv[b, :n].cpu().numpy(), e.send[b, :n].cpu().numpy()


def test_the_start_graphs_of_the_surface_fixture_equal_the_reference(dev):
    """The start graphs of rollout_eval_batch on a surface config are the eval script's (construct_graph: both rules, six bounds
    from the padded rows in its own order), edges and back-off trails.  Fails where the start batch follows the training path."""
    fx, ds, _, _, res = _eval_case(dev)
    assert ds.spec.connect_tool_surface and ds.spec.connect_tool_all_non_fixed and ds.spec.connect_tool_surface_ratio == 0.8
    for j, r in enumerate(fx["runs"]):
        recv, send = _edges_at(res, 0, j)
        assert [(float(a), int(k), int(c)) for a, k, c in res.trails[j][0]] == r["trail"][0], (j, res.trails[j][0], r["trail"][0])
        assert np.array_equal(recv, r["recv"][0]) and np.array_equal(send, r["send"][0]), j


def test_teacher_forced_steps_of_the_surface_fixture_as_one_batch(dev):
    """Every cloud the reference's builder was fed inside the step loop, as ONE batch: base build, both rule launches fed from those
    rows (no gather, n_obj rows, no padding, the step loop's bound order), the round-based back-off -> the fixture's edge lists and
    trails, and the planes the reference chose (as a set: only the pair matters)."""
    import adaptigraph_amd as ag
    fx, ds, _, _, _ = _eval_case(dev)
    sp = ds.spec
    clouds, n_obj, want, planes = [], [], [], []
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_batch_surface.npz"))
    for j, r in enumerate(fx["runs"]):
        first_call = np.concatenate([[0], np.cumsum([len(t) for t in r["trail"]])])
        for s in range(len(r["cloud"])):
            clouds.append(r["cloud"][s])
            n_obj.append(fx["n_obj"][j])
            want.append((r["recv"][s + 1], r["send"][s + 1], r["trail"][s + 1]))
            planes.append(set(g[f"r{j}::call::planes"][first_call[s + 1]].tolist()))
    S, N, M = len(clouds), ds.N, ds.n_eef
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    pos = t(np.stack(clouds).astype(F32))
    n_t = t(np.asarray(n_obj, np.int32))
    mask = torch.zeros((S, N), dtype=torch.uint8, device=dev)
    mask[torch.arange(N, device=dev)[None, :] < n_t[:, None]] = 1
    mask[:, sp.max_nobj:] = 1
    tool = torch.zeros((S, N), dtype=torch.uint8, device=dev)
    tool[:, sp.max_nobj:] = 1
    adj, knn0 = 0.5, 0.7
    thr2 = torch.full((S,), float(F32(adj * adj)), dtype=torch.float32, device=dev)
    cull = torch.full((S,), float(np.nextafter(F32(adj), F32(np.inf))), dtype=torch.float32, device=dev)
    knn = torch.full((S,), knn0, dtype=torch.float64, device=dev)
    bnd = (pos.view(-1, 3), torch.arange(S, dtype=torch.int64, device=dev) * N, None, n_t, 0)
    cfg = ag.RuleConfig(True, M, sp.connect_tool_surface_ratio, False, surface=True, bounds_order=0)
    wide = N * (min(N, sp.topk) + M)
    base = ag.construct_edges_graphs(pos, 0, mask, tool, thr2, cull, sp.topk, False, edge_cap=wide)
    el = ag.rule_attempt(cfg, pos, 0, mask, tool, base, knn, bnd, max(sp.max_nR, wide))
    plan = ag.BackoffPlan([knn0] * S, sp.topk, sp.max_nR, sp.min_kNN, sp.knn_increment)
    plan.record(el.n_edges.cpu().numpy())
    ag.backoff_rounds(cfg, plan, el, base, pos, mask, tool, thr2, cull, bnd)
    n, r, s, _ = lists(el)
    for i in range(S):
        assert [(float(a), int(k), int(c)) for a, k, c in plan.trail[i]] == want[i][2], (i, plan.trail[i], want[i][2])
        assert n[i] == len(want[i][0]) and np.array_equal(r[i, :n[i]], want[i][0]) and np.array_equal(s[i, :n[i]], want[i][1]), i
    # the first attempt's planes, from a launch of its own on the chained input
    mid = ag.nonfixed_rule_graphs(pos, 0, mask, tool, base, M, knn, *bnd, sp.connect_tool_surface_ratio, wide)
    pl = torch.zeros((S, 2), dtype=torch.int32, device=dev)
    ag.surface_rule_graphs(pos, 0, mask, tool, mid, M, *bnd, sp.connect_tool_surface_ratio, 0, wide, planes_out=pl)
    assert [set(p) for p in pl.cpu().numpy().tolist()] == planes


def test_free_running_surface_rollouts_equal_the_reference(dev):
    """rollout_eval_batch on eval_batch_surface.npz (the reference's construct_graph and rollout_from_start_graph on softbody.yaml
    with connect_tool_surface at ratio 0.8): edges and trails identical at every step, positions within POS_TOL, errors within the
    bound of tests/test_gpu_rule_batch.py; host_waits = steps + extra back-off rounds."""
    from test_gpu_parity import POS_TOL
    fx, ds, _, _, res = _eval_case(dev)
    sp = ds.spec
    B = len(fx["samples"])
    want_len = [len(r["idx_list"]) for r in fx["runs"]]
    assert res.lengths.tolist() == want_len and res.errors.shape == (max(want_len), B)
    assert [[tuple(p) for p in s] for s in res.schedule] == [[tuple(int(v) for v in p) for p in r["idx_list"]] for r in fx["runs"]]
    errors, pred = res.errors.cpu().numpy(), res.pred.cpu().numpy()
    bar = np.sqrt(3.0) * POS_TOL + fx["ref_gap"]              # the mean of norms is 1-Lipschitz in the positions
    worst_p = worst_e = 0.0
    kinds, extra = set(), 0
    for j, r in enumerate(fx["runs"]):
        L = want_len[j]
        assert np.isnan(errors[L:, j]).all() and not np.isnan(errors[:L, j]).any()
        assert [[(float(a), int(k), int(c)) for a, k, c in t] for t in res.trails[j]] == r["trail"], (j, res.trails[j], r["trail"])
        for t in r["trail"][1:]:
            kinds.add("fits" if len(t) == 1 else "topk" if t[-1][1] < sp.topk else "knn")
        for s in range(L):
            recv, send = _edges_at(res, s, j)
            assert np.array_equal(recv, r["recv"][s]) and np.array_equal(send, r["send"][s]), (j, s)
            worst_p = max(worst_p, float(np.abs(pred[s, j] - r["pred"][s]).max()))
            worst_e = max(worst_e, float(np.abs(np.float64(errors[s, j]) - np.float64(r["error_list"][s]))))
    print(f"eval_batch_surface: max |pred - reference| {worst_p:.3e} (bar {POS_TOL:.0e}), max |error - error_list| {worst_e:.3e} (bar {bar:.3e})")
    assert {"fits", "topk"} <= kinds
    assert worst_p <= POS_TOL and worst_e <= bar
    L_max = max(want_len)
    for s in range(1, L_max):
        extra += max(len(r["trail"][s]) for r in fx["runs"] if len(r["trail"]) > s) - 1
    print(f"host_waits {res.host_waits} = {L_max} steps + {extra} back-off rounds")
    assert res.host_waits == L_max + extra


# ------------------------------------------------------------------------------------------------ 4. paths
def test_the_batched_surface_rollout_equals_the_graph_by_graph_path(dev):
    import adaptigraph_amd as ag
    fx, ds, model, dr, res = _eval_case(dev)
    pg = ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr, keep_pred=True, per_graph=True)
    assert pg.lengths.tolist() == res.lengths.tolist() and pg.schedule == res.schedule
    for j in range(len(fx["samples"])):
        for s in range(int(res.lengths[j])):
            ra, sa = _edges_at(pg, s, j)
            rb, sb = _edges_at(res, s, j)
            assert np.array_equal(ra, rb) and np.array_equal(sa, sb), (j, s)
        assert pg.trails[j] == res.trails[j], j
    nn = lambda x: torch.nan_to_num(x, nan=-9.0)                          # noqa: E731
    assert torch.equal(nn(pg.errors), nn(res.errors)) and torch.equal(nn(pg.pred), nn(res.pred))


# ------------------------------------------------------------------------------------------------ 5. unchanged configs
def _same_batch(a, b):
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
    ea, eb = a["edges"], b["edges"]
    na, nb = ea.n_edges.cpu().numpy(), eb.n_edges.cpu().numpy()
    assert np.array_equal(na, nb) and torch.equal(ea.row_ptr, eb.row_ptr)
    for x in range(len(na)):
        assert torch.equal(ea.recv[x, :na[x]], eb.recv[x, :na[x]]) and torch.equal(ea.send[x, :na[x]], eb.send[x, :na[x]]), x


def test_the_public_batch_of_a_surface_config_still_follows_the_training_path(dev):
    """ds.batch as the public calls it never fires the surface rule: bit-equal to the sample-by-sample path (four bounds), trails
    included, and - on this fixture - different from the eval rollout's start graphs."""
    fx, ds, _, dr, res = _eval_case(dev)
    a = ds.batch(fx["samples"], draws=dr)
    trail = ds.last_trail
    b = ds.batch(fx["samples"], draws=dr, per_sample_edges=True)
    _same_batch(a, b)
    assert trail == ds.last_trail
    differ = sum(int(a["edges"].n_edges[j]) != len(fx["runs"][j]["recv"][0]) or
                 not np.array_equal(a["edges"].recv[j, :int(a["edges"].n_edges[j])].cpu().numpy(), fx["runs"][j]["recv"][0]) or
                 not np.array_equal(a["edges"].send[j, :int(a["edges"].n_edges[j])].cpu().numpy(), fx["runs"][j]["send"][0])
                 for j in range(len(fx["samples"])))
    assert differ >= 1


@pytest.mark.parametrize("name", ["eval_batch_rope", "eval_batch_softbody"])
def test_configs_without_the_surface_rule_are_unchanged(dev, name):
    """The rope (plain) and softbody (non-fixed rule, kNN range) fixtures: rollout_eval_batch's edges and trails at every step are
    the ones their own tests pin on the reference (tests/test_gpu_eval_batch.py, tests/test_gpu_rule_batch.py), predictions within
    POS_TOL; the start graphs equal ds.batch's public output bit for bit (the private start-graph switch has no effect there)."""
    from test_gpu_parity import POS_TOL
    fx, ds, _, dr, res = _eval_case(dev, name)
    assert not ds.spec.connect_tool_surface
    pred = res.pred.cpu().numpy()
    for j, r in enumerate(fx["runs"]):
        assert [[(float(a), int(k), int(c)) for a, k, c in t] for t in res.trails[j]] == r["trail"], j
        for s in range(len(r["idx_list"])):
            recv, send = _edges_at(res, s, j)
            assert np.array_equal(recv, r["recv"][s]) and np.array_equal(send, r["send"][s]), (j, s)
            assert float(np.abs(pred[s, j] - r["pred"][s]).max()) <= POS_TOL
    a = ds.batch(fx["samples"], draws=dr, with_fps=True)
    e0 = res.edges[0]
    for j in range(len(fx["samples"])):
        n = int(a["edges"].n_edges[j])
        assert n == int(e0.n_edges[j]) and torch.equal(a["edges"].recv[j, :n], e0.recv[j, :n]) and torch.equal(a["edges"].send[j, :n], e0.send[j, :n])
