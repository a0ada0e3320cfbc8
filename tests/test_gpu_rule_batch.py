"""GPU checks (-m gpu) of the batched tool-to-non-fixed rule: ag_edges_nonfixed_rule_graphs against the one-graph path
(construct_edges_from_states, itself pinned on the reference by edges_single_rules.npz), DeviceDynDataset's batched rule path and
its round-based back-off against the per-sample path, the fixtures and the CPU restatement."""
import copy
import json

import numpy as np
import pytest
import torch

import dataset_restate as DR

pytestmark = pytest.mark.gpu

F32 = np.float32
TOPK = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ 1. the kernel against the one-graph path
def host_threshold(rows_y, ratio):
    """rollout.surface_bounds + graph.py:134 on numpy float32 scalars; no row at all: NaN (the device's empty subset)."""
    if len(rows_y) == 0:
        return F32(np.nan), F32(np.nan), F32(np.nan)
    max_y = np.max(rows_y) * ratio
    min_y = np.min(rows_y)
    thr = (max_y - min_y) * 0.1 + min_y
    assert isinstance(thr, np.float32)
    return max_y, min_y, thr


def make_batch(No, M, B, ratio, padded, gather, seed):
    """B graphs of No object rows + M tool rows (the tools behind the objects, as the dataset lays them out) with ragged n_obj.
    Clouds alternate between a jittered one (no ties) and a lattice on a 1/8 grid with the tools on grid points (tied pair
    distances).  Special graphs: b % 7 == 1 no tool contact (the tool rows are masked out), 2 every particle below the threshold
    (its bounds rows lie 10 above its positions), 3 n_obj = 0.  kNN cycles through 1.0, keepK = 0, 1, #pairs - 1 and 0.5."""
    rng = np.random.default_rng(seed)
    N = No + M
    pos = np.zeros((B, N, 3), F32)
    mask = np.zeros((B, N), bool)
    tool = np.zeros((B, N), bool)
    tool[:, No:] = True
    n_obj = np.zeros(B, np.int32)
    stride = max(1, No)
    cloud_pts = No + 3                                                   # every graph's cloud in the flat bounds buffer
    bnd = np.zeros((B * cloud_pts + 1, 3), F32)
    first = np.arange(B, dtype=np.int64) * cloud_pts
    idx = np.full((B, stride), -1, np.int32)
    adj = np.zeros(B)
    kNN = np.ones(B)
    thr = np.zeros(B, F32)
    bounds = []
    for b in range(B):
        kind = b % 7
        n = int(rng.integers(0, No + 1)) if b else No
        if kind == 3:
            n = 0
        if b % 2:                                                        # lattice, ties
            cloud = (rng.integers(0, 9, (cloud_pts, 3)) / 8.0).astype(F32) * F32([1.0, 0.5, 1.0])
            tools = (rng.integers(2, 7, (M, 3)) / 8.0).astype(F32) * F32([1.0, 0.5, 1.0])
            tools[:, 1] += F32(0.125)
        else:
            cloud = rng.uniform(0, 1, (cloud_pts, 3)).astype(F32) * F32([1.0, 0.5, 1.0])
            tools = rng.uniform(0.3, 0.7, (M, 3)).astype(F32) * F32([1.0, 0.5, 1.0]) + F32([0, 0.2, 0])
        sel = rng.permutation(cloud_pts)[:n].astype(np.int32) if gather else np.arange(n, dtype=np.int32)
        bnd[first[b]:first[b] + cloud_pts] = cloud
        idx[b, :n] = sel
        pos[b, :n] = cloud[sel]
        pos[b, No:] = tools
        if kind == 2:
            bnd[first[b]:first[b] + cloud_pts, 1] += F32(10.0)
        mask[b, :n] = True
        mask[b, No:] = kind != 1
        n_obj[b] = n
        adj[b] = rng.uniform(0.25, 0.45)
        rows = bnd[first[b] + sel, 1]
        if padded and No > n:
            rows = np.concatenate([rows, np.zeros(1, F32)])
        max_y, min_y, thr[b] = host_threshold(rows, ratio)
        bounds.append((max_y, min_y))
        pairs = int((mask[b] & (pos[b, :, 1] > thr[b])).sum()) * M
        choice = b % 5
        if pairs >= 2:
            kNN[b] = [1.0, 1e-9, 1.5 / pairs, (pairs - 0.5) / pairs, 0.5][choice]
            want_keep = [None, 0, 1, pairs - 1, None][choice]
            assert want_keep is None or int(kNN[b] * pairs) == want_keep
        else:
            kNN[b] = [1.0, 0.5][b % 2]
    return dict(No=No, M=M, B=B, N=N, pos=pos, mask=mask, tool=tool, n_obj=n_obj, bnd=bnd, first=first, idx=idx if gather else None,
                adj=adj, kNN=kNN, thr=thr, bounds=bounds, ratio=ratio, pad_rows=No if padded else 0)


def upload(c, dev, order=None):
    o = np.arange(c["B"]) if order is None else np.asarray(order)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[o])).to(dev)   # noqa: E731
    adj = c["adj"][o]
    thr2 = (adj * adj).astype(F32)
    cull = np.nextafter(np.abs(adj).astype(F32), F32(np.inf))
    return dict(pos=t(c["pos"]), mask=t(c["mask"]).view(torch.uint8), tool=t(c["tool"]).view(torch.uint8), kNN=t(c["kNN"]),
                first=t(c["first"]), idx=None if c["idx"] is None else t(c["idx"]), n=t(c["n_obj"]),
                thr2=torch.from_numpy(thr2).to(dev), cull=torch.from_numpy(cull).to(dev), bnd=torch.from_numpy(c["bnd"]).to(dev))


def run_rule(ag, c, d, edge_cap=None, n_tools=None, sentinel=None):
    """The base build and the rule launch on uploaded tensors -> (base, out EdgeList, thr)."""
    B, N, M = d["mask"].shape[0], c["N"], c["M"]
    base = ag.construct_edges_graphs(d["pos"], 0, d["mask"], d["tool"], d["thr2"], d["cull"], TOPK, False,
                                     edge_cap=max(1, N * (min(TOPK, N) + M)))
    cap = max(1, N * (min(TOPK, N) + M) + N * M) if edge_cap is None else edge_cap
    out = None
    if sentinel is not None:
        full = lambda *s: torch.full(s, sentinel, dtype=torch.int32, device=d["pos"].device)   # noqa: E731
        out = ag.EdgeList(full(B, cap), full(B, cap), full(B, N + 1), full(B), N)
    thr = torch.full((B,), 7.0, dtype=torch.float32, device=d["pos"].device)
    out = ag.nonfixed_rule_graphs(d["pos"], 0, d["mask"], d["tool"], base, M if n_tools is None else n_tools, d["kNN"], d["bnd"],
                                  d["first"], d["idx"], d["n"], c["pad_rows"], c["ratio"], cap, out=out, thr_out=thr)
    return base, out, thr


def lists(el):
    n = el.n_edges.cpu().numpy()
    r, s, rp = el.recv.cpu().numpy(), el.send.cpu().numpy(), el.row_ptr.cpu().numpy()
    return n, r, s, rp


def partner(ag, c, dev, b):
    max_y, min_y = c["bounds"][b]
    el = ag.construct_edges_from_states(torch.from_numpy(c["pos"][b]).to(dev), float(c["adj"][b]), torch.from_numpy(c["mask"][b]).to(dev),
                                        torch.from_numpy(c["tool"][b]).to(dev), topk=TOPK, connect_tools_all=False, max_y=max_y,
                                        min_y=min_y, connect_tool_all_non_fixed=True, kNN=float(c["kNN"][b]), as_index=True)
    n, r, s, rp = lists(el)
    return int(n[0]), r[0, :n[0]], s[0, :n[0]], rp[0]


SIZES = [(1, 1), (7, 2), (63, 1), (64, 1), (65, 5), (205, 5), (230, 5), (300, 5)]
MODES = [(1.0, True, True), (0.8, False, False), (0.8, True, True), (1.0, False, False)]      # ratio, padded, gather


def test_the_modes_cover_both_ratios_padded_and_unpadded():
    used = {MODES[i % 4] for i in range(len(SIZES))}
    assert {m[0] for m in used} == {1.0, 0.8} and {m[1] for m in used} == {True, False}


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("si", range(len(SIZES)), ids=[f"{a}+{b}" for a, b in SIZES])
def test_the_batched_rule_equals_the_one_graph_path(dev, si, B):
    """recv, send, row_ptr and n_edges of every graph bit-equal to construct_edges_from_states(..., as_index=True); thr bit-equal
    to the host expression; a permuted batch and B = 1 slices bit-equal to the batch."""
    import adaptigraph_amd as ag
    No, M = SIZES[si]
    ratio, padded, gather = MODES[si % 4]
    c = make_batch(No, M, B, ratio, padded, gather, seed=100 * si + B)
    d = upload(c, dev)
    base, out, thr = run_rule(ag, c, d)
    n, r, s, rp = lists(out)
    got_thr = thr.cpu().numpy()
    nan = np.isnan(c["thr"])                                             # (no bounds row at all; NaN payloads are not compared)
    assert np.array_equal(np.isnan(got_thr), nan) and np.array_equal(got_thr[~nan].view(np.uint32), c["thr"][~nan].view(np.uint32))
    nb, _, bs, _ = lists(base)
    applied = changed = 0
    for b in range(B):
        wn, wr, ws, wrp = partner(ag, c, dev, b)
        assert n[b] == wn, (b, n[b], wn)
        assert np.array_equal(r[b, :wn], wr) and np.array_equal(s[b, :wn], ws) and np.array_equal(rp[b], wrp), b
        if b % 7 in (1, 2):                                              # no contact / empty subset: nothing gained
            assert n[b] <= nb[b]
        if b % 7 == 1:
            assert n[b] == nb[b] and np.array_equal(s[b, :wn], bs[b, :wn])   # copied through
        if b % 7 == 3:
            assert c["n_obj"][b] == 0
        applied += int(c["mask"][b, No:].any())
        changed += int(n[b] != nb[b])
    print(f"{No}+{M} B={B}: {applied} graphs with tool contact, {changed} whose count the rule changed, counts up to {n.max()}")
    # permuted batch
    perm = np.random.default_rng(si).permutation(B)
    _, outp, thrp = run_rule(ag, c, upload(c, dev, perm))
    n2, r2, s2, rp2 = lists(outp)
    assert np.array_equal(n2, n[perm]) and np.array_equal(rp2, rp[perm])
    assert np.array_equal(thrp.cpu().numpy().view(np.uint32), got_thr[perm].view(np.uint32))
    for j, b in enumerate(perm):
        assert np.array_equal(r2[j, :n[b]], r[b, :n[b]]) and np.array_equal(s2[j, :n[b]], s[b, :n[b]]), b
    # B = 1 slices
    for b in range(min(B, 8)):
        _, o1, _ = run_rule(ag, c, upload(c, dev, [b]))
        n1, r1, s1, rp1 = lists(o1)
        assert n1[0] == n[b] and np.array_equal(rp1[0], rp[b])
        assert np.array_equal(r1[0, :n[b]], r[b, :n[b]]) and np.array_equal(s1[0, :n[b]], s[b, :n[b]]), b


def test_rows_striped_two_per_thread_equal_the_one_graph_path(dev):
    """1023 + 2 particles: a 1024-thread workgroup owns two rows per thread, its last busy thread one, the rest none - the striping
    of the guard, the tool list and the merge that no smaller size reaches.  Three graphs of a 14-graph batch: every particle valid
    with kNN 1.0, a jittered cloud with kNN 0.5, a lattice (tied distances) with keepK = #pairs - 1."""
    import adaptigraph_amd as ag
    c = make_batch(1023, 2, 14, 0.8, True, True, seed=80)
    sel = [0, 4, 13]
    assert [c["kNN"][0], c["kNN"][4]] == [1.0, 0.5] and 0.5 < c["kNN"][13] < 1.0 and all(c["n_obj"][b] > 700 for b in sel)
    _, out, thr = run_rule(ag, c, upload(c, dev, sel))
    n, r, s, rp = lists(out)
    assert np.array_equal(thr.cpu().numpy().view(np.uint32), c["thr"][sel].view(np.uint32))
    for j, b in enumerate(sel):
        wn, wr, ws, wrp = partner(ag, c, dev, b)
        assert n[j] == wn, (b, n[j], wn)
        assert np.array_equal(r[j, :wn], wr) and np.array_equal(s[j, :wn], ws) and np.array_equal(rp[j], wrp), b
        assert (ws >= 1023).sum() > 0                                    # the rule's tool senders are in the list


def apply_tool_rule(dev, c, base, subset, kNN, n_tools, edge_cap):
    """ag_edges_apply_tool_rule itself on graph 0 of c, into outputs filled with -7 -> (n_out, recv, send, row_ptr)."""
    from adaptigraph_amd.context import current_stream, default_engine, ptr
    eng = default_engine(dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    pos, mask, tool, sub = t(c["pos"][0]), t(c["mask"][0]).view(torch.uint8), t(c["tool"][0]).view(torch.uint8), t(subset).view(torch.uint8)
    full = lambda n: torch.full((n,), -7, dtype=torch.int32, device=dev)  # noqa: E731
    recv, send, row_ptr, n_out = full(edge_cap), full(edge_cap), full(c["N"] + 1), full(1)
    eng.check(eng.lib.ag_edges_apply_tool_rule(eng.ctx, current_stream(dev), ptr(pos), ptr(mask), ptr(tool), c["N"], n_tools,
                                               ptr(base.send), ptr(base.row_ptr), ptr(sub), float(kNN), edge_cap, ptr(recv), ptr(send),
                                               ptr(row_ptr), ptr(n_out)))
    return int(n_out.item()), recv.cpu().numpy(), send.cpu().numpy(), row_ptr.cpu().numpy()


@pytest.mark.parametrize("kNN", [1.0, 0.5])
def test_the_one_graph_export_keeps_its_own_overflow_and_tool_count_contracts(dev, kNN):
    """include/adaptigraph_amd.h on ag_edges_apply_tool_rule, at 7 + 2 particles: above edge_cap the TRUE count and all of row_ptr
    are written and recv / send are not; with a wrong n_tools the count is -1 and nothing else is written."""
    import adaptigraph_amd as ag
    c = make_batch(7, 2, 1, 1.0, False, False, seed=9)
    d = upload(c, dev)
    N, M = c["N"], c["M"]
    base = ag.construct_edges_graphs(d["pos"], 0, d["mask"], d["tool"], d["thr2"], d["cull"], TOPK, False, edge_cap=N * (TOPK + M))
    subset = c["mask"][0] & (c["pos"][0, :, 1] > c["thr"][0])
    assert subset.sum() >= 2
    wide = N * (TOPK + M) + N * M
    n, r, s, rp = apply_tool_rule(dev, c, base, subset, kNN, M, wide)
    assert 2 <= n <= wide and rp[0] == 0 and rp[N] == n and (np.diff(rp) >= 0).all() and (r[n:] == -7).all() and (s[n:] == -7).all()
    assert np.array_equal(r[:n], np.repeat(np.arange(N), np.diff(rp))) and (s[:n] >= 0).all() and (s[:n] < N).all()
    n2, r2, s2, rp2 = apply_tool_rule(dev, c, base, subset, kNN, M, n - 1)
    assert n2 == n and np.array_equal(rp2, rp) and (r2 == -7).all() and (s2 == -7).all()
    for wrong in (M - 1, M + 1):
        n3, r3, s3, rp3 = apply_tool_rule(dev, c, base, subset, kNN, wrong, wide)
        assert n3 == -1 and (r3 == -7).all() and (s3 == -7).all() and (rp3 == -7).all(), wrong


def test_a_graph_over_edge_cap_reports_its_count_and_writes_nothing(dev):
    import adaptigraph_amd as ag
    c = make_batch(65, 5, 9, 1.0, True, True, seed=5)
    d = upload(c, dev)
    _, full, _ = run_rule(ag, c, d)
    n, r, s, rp = lists(full)
    g = int(np.argmax(n))
    cap = int(n[g]) - 1
    assert cap >= 1 and (n <= cap).sum() >= 3
    _, out, _ = run_rule(ag, c, d, edge_cap=cap, sentinel=-7)
    n2, r2, s2, rp2 = lists(out)
    assert np.array_equal(n2, n)                                         # the TRUE counts
    for b in range(9):
        if n[b] > cap:
            assert (r2[b] == -7).all() and (s2[b] == -7).all() and (rp2[b] == -7).all(), b
        else:
            assert np.array_equal(r2[b, :n[b]], r[b, :n[b]]) and np.array_equal(s2[b, :n[b]], s[b, :n[b]]) and np.array_equal(rp2[b], rp[b])
            assert (r2[b, n[b]:] == -7).all() and (s2[b, n[b]:] == -7).all()


def test_a_wrong_tool_count_is_refused_per_graph_and_raises_in_python(dev):
    import adaptigraph_amd as ag
    c = make_batch(7, 2, 3, 1.0, True, True, seed=6)
    _, out, thr = run_rule(ag, c, upload(c, dev), n_tools=3, sentinel=-7)
    n, r, s, rp = lists(out)
    assert (n == -1).all() and (r == -7).all() and (s == -7).all() and (rp == -7).all() and (thr.cpu().numpy() == 7.0).all()
    plan = ag.BackoffPlan(c["kNN"], TOPK, 1000)
    with pytest.raises(RuntimeError, match="internal"):
        plan.record(n)


def test_a_base_count_above_its_capacity_is_refused(dev):
    import adaptigraph_amd as ag
    c = make_batch(7, 2, 3, 1.0, True, True, seed=7)
    d = upload(c, dev)
    base, good, _ = run_rule(ag, c, d)
    base.n_edges[1] = base.edge_cap + 1
    out = ag.nonfixed_rule_graphs(d["pos"], 0, d["mask"], d["tool"], base, 2, d["kNN"], d["bnd"], d["first"], d["idx"], d["n"],
                                  c["pad_rows"], c["ratio"], good.edge_cap)
    n = out.n_edges.cpu().numpy()
    assert n[1] == -1 and n[0] == good.n_edges[0].item() and n[2] == good.n_edges[2].item()


def test_above_the_pair_limit_the_call_is_refused_before_any_launch(dev):
    import adaptigraph_amd as ag
    from adaptigraph_amd.graph import RULE_GRAPHS_MAX_PAIRS, rule_graphs_limit
    N, M = 4096, 3
    assert N * M > RULE_GRAPHS_MAX_PAIRS and rule_graphs_limit(N, M) is not None and rule_graphs_limit(305, 5) is None
    z = lambda *sh, dt=torch.int32: torch.zeros(sh, dtype=dt, device=dev)    # noqa: E731
    base = ag.EdgeList(z(1, 8), z(1, 8), z(1, N + 1), z(1), N)
    out = ag.EdgeList(torch.full((1, 8), -7, dtype=torch.int32, device=dev), z(1, 8), z(1, N + 1), torch.full((1,), -7, dtype=torch.int32, device=dev), N)
    with pytest.raises(NotImplementedError, match="8192"):
        ag.nonfixed_rule_graphs(z(1, N, 3, dt=torch.float32), 0, z(1, N, dt=torch.uint8), z(1, N, dt=torch.uint8), base, M,
                                torch.ones(1, dtype=torch.float64, device=dev), z(4, 3, dt=torch.float32), z(1, dt=torch.int64), None,
                                z(1), 0, 1.0, 8, out=out)
    torch.cuda.synchronize()
    assert out.n_edges.item() == -7 and (out.recv == -7).all()


def test_the_rule_launch_does_not_wait_for_the_gpu(dev):
    """ag_edges_nonfixed_rule_graphs only enqueues: it returns while an earlier kernel still spins on the stream."""
    import adaptigraph_amd as ag
    c = make_batch(65, 5, 3, 1.0, True, True, seed=8)
    d = upload(c, dev)
    base, want, _ = run_rule(ag, c, d)
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
    out = ag.nonfixed_rule_graphs(d["pos"], 0, d["mask"], d["tool"], base, 5, d["kNN"], d["bnd"], d["first"], d["idx"], d["n"],
                                  c["pad_rows"], c["ratio"], want.edge_cap)
    still_busy = not done.query()
    torch.cuda.synchronize()
    assert still_busy, "ag_edges_nonfixed_rule_graphs waited for the GPU"
    assert torch.equal(out.n_edges, want.n_edges)


# ------------------------------------------------------------------------------------------------ 2. the dataset
def _draws(ag, d, dev):
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)   # noqa: E731
    return ag.BatchDraws(t(d["fps_start"], torch.int32), t(d["fps_radius"], torch.float32), t(d["rad_start"], torch.int32),
                         t(d["phys_noise"], torch.float64), t(d["state_noise"], torch.float64), t(d["rot"], torch.float64),
                         t(d["adj_thresh"], torch.float64), t(d["knn_thresh"], torch.float64))


def _edges_of(el):
    n, r, s, rp = lists(el)
    return n, [r[b, :n[b]] for b in range(len(n))], [s[b, :n[b]] for b in range(len(n))], rp


def _same_edges(a, b):
    na, ra, sa, rpa = _edges_of(a)
    nb, rb, sb, rpb = _edges_of(b)
    assert np.array_equal(na, nb) and np.array_equal(rpa, rpb)
    for x in range(len(na)):
        assert np.array_equal(ra[x], rb[x]) and np.array_equal(sa[x], sb[x]), x


def test_the_softbody_fixture_batch_waits_once(dev):
    import adaptigraph_amd as ag
    fx = DR.load_fixture("dataset_softbody")
    ds = ag.DeviceDynDataset(*DR.dataset_args(fx), device=dev)
    assert not ds.spec.batched_edges
    data = ds.batch(fx["samples"], draws=_draws(ag, fx["draws"], dev))
    assert ds.last_waits == 1
    n, recv, send, _ = _edges_of(data["edges"])
    assert np.array_equal(n, fx["want"]["n_edges"])
    for b in range(len(n)):
        assert np.array_equal(recv[b], fx["want"]["recv"][b]) and np.array_equal(send[b], fx["want"]["send"][b]), b
        assert [(float(a), int(k), int(c)) for a, k, c in ds.last_trail[b]] == fx["trail"][b], b


def synthetic_softbody(max_nR, B=40, seed=11):
    """A softbody-like set: softbody.yaml's switches (n_his 5, rest frame, non-fixed rule, knn_range [0.4, 1.0], min_knn 0.4) on
    three ragged episodes of 40 / 55 / 70 points, max_nobj 24, two tool points, top-k 6.  -> (constructor arguments, idx, draws)."""
    fx = DR.load_fixture("dataset_softbody")
    dcfg, mcfg = copy.deepcopy(fx["dataset_config"]), copy.deepcopy(fx["material_config"])
    dcfg["datasets"][0].update(max_nobj=24, max_nR=max_nR, fps_radius_range=[0.16, 0.22], adj_radius_range=[0.3, 0.45], topk=6)
    rng = np.random.default_rng(seed)
    obj, eef, phys, pairs = [], [], [], []
    T = 12
    for e, n_e in enumerate((40, 55, 70)):
        base = rng.uniform(0, 1, (n_e, 3)).astype(F32) * F32([1.0, 0.4, 1.0])
        drift = rng.normal(0, 0.01, (T, n_e, 3)).astype(F32).cumsum(0)
        obj.append(base[None] + drift)
        eef.append(np.stack([F32([0.3 + 0.02 * t, 0.42, 0.5]) + F32([[0, 0, 0], [0.2, 0.0, 0.05]]) for t in range(T)]).astype(F32))
        phys.append({fx["material"]: np.array([0.3 + 0.1 * e])})
        for s in range(T - 8 + 1):
            pairs.append([e] + list(range(s, s + 8)))
    pairs = np.asarray(pairs, np.int64)
    idx = rng.integers(0, len(pairs), B)
    n_e = np.array([obj[pairs[i, 0]].shape[1] for i in idx])
    draws = dict(fps_start=(rng.uniform(size=B) * n_e).astype(np.int32), fps_radius=rng.uniform(0.16, 0.22, B).astype(F32),
                 rad_start=(rng.uniform(size=B) * np.minimum(n_e, 24)).astype(np.int32), phys_noise=np.zeros((B, 1)),
                 state_noise=None, rot=None, adj_thresh=rng.uniform(0.3, 0.45, B), knn_thresh=rng.uniform(0.4, 1.0, B))
    return (dcfg, mcfg, pairs, phys, obj, eef), idx, draws


@pytest.mark.parametrize("max_nR", [400, 120])
def test_the_batched_rule_path_equals_the_per_sample_path_and_the_restatement(dev, max_nR):
    """B = 40.  max_nR 400: every graph fits, one wait.  max_nR 120: by the restatement the batch holds all three trail kinds
    (fits / kNN only / kNN then top-k); the waits are 1 + the longest trail's extra attempts."""
    import adaptigraph_amd as ag
    args, idx, draws = synthetic_softbody(max_nR)
    want = DR.restate_batch(*args, idx, draws)
    kinds = {"fits" if len(t) == 1 else "topk" if t[-1][1] < t[0][1] else "knn" for t in want["trail"]}
    assert kinds == ({"fits"} if max_nR == 400 else {"fits", "knn", "topk"})
    ds = ag.DeviceDynDataset(*args, device=dev)
    dr = _draws(ag, draws, dev)
    a = ds.batch(idx, draws=dr)
    waits, trail = ds.last_waits, ds.last_trail
    b = ds.batch(idx, draws=dr, per_sample_edges=True)
    assert ds.last_waits is None
    _same_edges(a["edges"], b["edges"])
    assert trail == ds.last_trail
    assert waits == max(len(t) for t in want["trail"]) and (max_nR != 400 or waits == 1)
    n, recv, send, _ = _edges_of(a["edges"])
    assert (n <= max_nR).all()
    for x in range(len(n)):
        assert np.array_equal(recv[x], want["recv"][x]) and np.array_equal(send[x], want["send"][x]), x
        assert [(float(p), int(k), int(c)) for p, k, c in trail[x]] == [tuple(r) for r in want["trail"][x]], x
    for k in ("state", "action", "attrs"):
        assert torch.equal(a[k], b[k])


# ------------------------------------------------------------------------------------------------ 3. eval, teacher-forced
def test_teacher_forced_steps_of_the_softbody_eval_fixture_as_one_batch(dev):
    """The 12 clouds the reference's builder was fed (eval_rollout_softbody.npz: its predicted rows, then the tool rows) as ONE
    batch: the base build, the rule launch fed from those rows (no gather, n_obj rows, no padding) and the round-based back-off
    reproduce the fixture's edge lists and (kNN, topk, n_rel) trails at every step, kNN-only and top-k back-off steps included."""
    import adaptigraph_amd as ag
    from helpers import load_golden, split_edges
    g = load_golden("eval_rollout_softbody")
    meta = json.loads(bytes(g["meta_json"]).decode())
    assert meta["connect_tool_all_non_fixed"] and not meta["connect_tool_surface"]
    clouds = np.ascontiguousarray(g["builder_states"], F32)
    S, N, _ = clouds.shape
    n_obj = int(g["obj_mask"].sum())
    assert g["obj_mask"][:n_obj].all() and np.array_equal(clouds[:, :g["pred_pos"].shape[1]], g["pred_pos"])
    M = int(g["eef_mask"].sum())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    pos = t(clouds)
    mask = t(np.broadcast_to(g["state_mask"], (S, N))).view(torch.uint8)
    tool = t(np.broadcast_to(g["eef_mask"], (S, N))).view(torch.uint8)
    adj = float(meta["adj_thresh"])
    thr2 = torch.full((S,), float(F32(adj * adj)), dtype=torch.float32, device=dev)
    cull = torch.full((S,), float(np.nextafter(F32(abs(adj)), F32(np.inf))), dtype=torch.float32, device=dev)
    knn = torch.full((S,), float(meta["knn_thresh"]), dtype=torch.float64, device=dev)
    bnd = (pos.view(-1, 3), torch.arange(S, dtype=torch.int64, device=dev) * N, None, torch.full((S,), n_obj, dtype=torch.int32, device=dev), 0)
    cfg = ag.RuleConfig(True, M, meta["connect_tool_surface_ratio"], meta["connect_tool_all"])
    k = min(N, meta["topk"])
    base = ag.construct_edges_graphs(pos, 0, mask, tool, thr2, cull, meta["topk"], meta["connect_tool_all"], edge_cap=N * (k + M))
    el = ag.rule_attempt(cfg, pos, 0, mask, tool, base, knn, bnd, max(meta["max_nR"], N * (k + M)))
    plan = ag.BackoffPlan([meta["knn_thresh"]] * S, meta["topk"], meta["max_nR"], meta["min_kNN"], meta["knn_increment"])
    plan.record(el.n_edges.cpu().numpy())
    ag.backoff_rounds(cfg, plan, el, base, pos, mask, tool, thr2, cull, bnd)
    edges = split_edges(g, "step::")
    n, r, s, _ = lists(el)
    kinds = set()
    for i in range(S):
        assert [list(x) for x in plan.trail[i]] == meta["trails"][i], (i, plan.trail[i], meta["trails"][i])
        assert n[i] == len(edges[i][0]) and np.array_equal(r[i, :n[i]], edges[i][0]) and np.array_equal(s[i, :n[i]], edges[i][1]), i
        tr = plan.trail[i]
        kinds.add("fits" if len(tr) == 1 else "topk" if tr[-1][1] < meta["topk"] else "knn")
    assert kinds == {"fits", "knn", "topk"} and plan.rounds == max(len(x) for x in meta["trails"])


# ------------------------------------------------------------------------------------------------ 4. eval, free-running
_EVAL = {}


def _eval_case(dev):
    import adaptigraph_amd as ag
    import eval_restate as ER
    import train_restate as TR
    from test_gpu_train import _model
    if not _EVAL:
        fx = ER.load_fixture("eval_batch_softbody")
        ds = ag.DeviceDynDataset(*ER.dataset_args(fx), device=dev, phase="valid")
        model = _model(dev, TR.make_weights(fx["w_seed"], n_his=5), n_his=5, pstep=4, material=fx["material"])
        dr = ds.eval_draws(fx["samples"], fps_start=fx["fps_start"], rad_start=fx["rad_start"])
        _EVAL["case"] = (fx, ds, model, dr, ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr, keep_pred=True))
    return _EVAL["case"]


def _edges_at(res, s, b):
    e = res.edges[s]
    n = int(e.n_edges[b])
    return e.recv[b, :n].cpu().numpy(), e.send[b, :n].cpu().numpy()


def test_free_running_rule_rollouts_equal_the_reference(dev):
    """rollout_eval_batch on eval_batch_softbody.npz (the reference's construct_graph and rollout_from_start_graph on softbody.yaml's
    switches): edges and trails identical at every step, positions within POS_TOL, errors within the bound of
    tests/test_gpu_eval_batch.py; the rebuilt graphs hold a kNN-only and a kNN-then-top-k back-off."""
    from test_gpu_parity import POS_TOL
    fx, ds, _, _, res = _eval_case(dev)
    sp = ds.spec
    assert sp.connect_tool_all_non_fixed and not sp.connect_tool_surface and sp.min_kNN == 0.4 and not sp.batched_edges
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
    print(f"eval_batch_softbody: max |pred - reference| {worst_p:.3e} (bar {POS_TOL:.0e}), max |error - error_list| {worst_e:.3e} (bar {bar:.3e})")
    assert kinds == {"fits", "knn", "topk"}
    assert worst_p <= POS_TOL and worst_e <= bar
    # the waits: one per step, plus the extra rounds of each step's back-off (the longest trail among the graphs rebuilt there)
    L_max = max(want_len)
    for s in range(1, L_max):
        extra += max(len(r["trail"][s]) for r in fx["runs"] if len(r["trail"]) > s) - 1
    print(f"host_waits {res.host_waits} = {L_max} steps + {extra} back-off rounds")
    assert res.host_waits == L_max + extra


def test_the_batched_rule_rollout_equals_the_graph_by_graph_path(dev):
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
