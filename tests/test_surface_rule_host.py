"""CPU checks of the batched two-closest-planes rule: the export and its declaration, the numpy restatement of the kernel
(tests/surface_restate.py) on every builder call the reference made for tests/golden/eval_batch_surface.npz - start graphs in
construct_graph's bound order, rebuilt graphs in the step loop's -, and graph.rule_attempt / backoff_rounds chaining the two rule
launches and graph.attempt_with_backoff on a config with neither rule, driven through a stub engine that records what would be
launched."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import dataset_restate as DR
import eval_restate as ER
import surface_restate as SR
from oracle import adaptigraph_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ADJ, RATIO = 0.5, 0.8


# ------------------------------------------------------------------------------------------------ the boundary
def test_the_export_is_declared_and_exported_and_the_abi_version_stays_7():
    from adaptigraph_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()
    assert re.search(r"#define\s+AG_ABI_VERSION\s+7u?\b", hdr)
    assert re.search(r"int\s+ag_edges_surface_rule_graphs\s*\(\s*ag_ctx\*\s*ctx,\s*void\*\s*stream,\s*const\s+ag_surface_rule_graphs_args\*", hdr)
    assert "never waits for the GPU" in hdr[hdr.index("typedef struct ag_surface_rule_graphs_args") - 3000:hdr.index("typedef struct ag_surface_rule_graphs_args")]
    assert "ag_edges_surface_rule_graphs" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.ag_abi_version() == 7 and hasattr(lib, "ag_edges_surface_rule_graphs")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T ag_edges_surface_rule_graphs$", out, flags=re.M)
    # the ctypes struct follows the header field for field
    body = hdr[hdr.index("typedef struct ag_surface_rule_graphs_args {"):hdr.index("} ag_surface_rule_graphs_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in decl.split(",")[0].rsplit(None, 1)[-1:]] + [n.strip(" *") for n in decl.split(",")[1:]]
    assert names == [n for n, _ in _lib.AgSurfaceRuleGraphsArgs._fields_]


# ------------------------------------------------------------------------------------------------ the restatement on the reference's calls
def _calls():
    """Every builder call of the fixture: (run, build, attempt, is last attempt, cloud, kNN, topk, n_rel, bounds rows, pad_rows, order,
    recorded bounds, recorded planes)."""
    fx = ER.load_fixture("eval_batch_surface")
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_batch_surface.npz"))
    No = fx["dataset_config"]["datasets"][0]["max_nobj"]
    nh = fx["dataset_config"]["n_his"]
    out = []
    for j, r in enumerate(fx["runs"]):
        ep = int(fx["pair_lists"][fx["samples"][j]][0])
        t0 = int(fx["pair_lists"][fx["samples"][j]][nh - 1])              # frame n_his - 1 of the start pair (short pairs, rest frame in front)
        n = int(fx["n_obj"][j])
        fps = fx["fps_idx"][j, :n]
        mask = np.zeros(No + 2, bool)
        mask[:n] = mask[No:] = True
        tool = np.zeros(No + 2, bool)
        tool[No:] = True
        c = 0
        for bi, trail in enumerate(r["trail"]):
            cloud = r["state"][0][-1] if bi == 0 else r["cloud"][bi - 1]
            rows, pad, order = (fx["obj_pos"][ep][t0][fps], No, 1) if bi == 0 else (cloud[:n], 0, 0)
            for ai, (kNN, k, n_rel) in enumerate(trail):
                out.append(dict(j=j, bi=bi, ai=ai, last=ai == len(trail) - 1, cloud=cloud, kNN=kNN, topk=k, n_rel=n_rel, rows=rows, pad=pad,
                                order=order, mask=mask, tool=tool, bounds=g[f"r{j}::call::bounds"][c], planes=g[f"r{j}::call::planes"][c],
                                recv=r["recv"][bi], send=r["send"][bi]))
                c += 1
        assert c == len(g[f"r{j}::call::bounds"])
    return fx, out


def test_the_restatement_reproduces_every_builder_call_of_the_reference():
    """Bounds bit-equal to the float32 scalars the reference passed (start graphs: construct_graph's order on the padded rows;
    rebuilt graphs: the step loop's order on the predicted rows), the chosen plane pair, every attempt's edge count and the edge
    list the forward ran on.  The fixture holds what makes this a test: calls where the rule fires and changes the graph, calls it
    copies through, and start graphs whose bounds the other order would get wrong."""
    fx, calls = _calls()
    fired = {0: 0, 1: 0}
    changed = {0: 0, 1: 0}
    copied = wrong_order = 0
    for c in calls:
        got = SR.chained(c["cloud"], ADJ, c["mask"], c["tool"], c["topk"], False, True, c["kNN"], c["rows"], c["pad"], RATIO, c["order"])
        where = (c["j"], c["bi"], c["ai"])
        assert np.array_equal(got["bounds"], c["bounds"]), (where, got["bounds"], c["bounds"])
        assert set(got["planes"]) == set(c["planes"].tolist()), (where, got["planes"], c["planes"])
        assert len(got["recv"]) == c["n_rel"], where
        if c["last"]:
            assert np.array_equal(got["recv"], c["recv"]) and np.array_equal(got["send"], c["send"]), where
        start = int(c["bi"] == 0)
        if start and not np.array_equal(SR.bounds6(c["rows"], c["pad"], RATIO, 0), c["bounds"]):
            wrong_order += 1
        if got["check"] == 0:
            copied += 1
            assert np.array_equal(got["recv"], got["mid"][0]) and np.array_equal(got["send"], got["mid"][1])
            continue
        fired[start] += 1
        before = set(zip(got["mid"][0].tolist(), got["mid"][1].tolist()))
        after = set(zip(got["recv"].tolist(), got["send"].tolist()))
        changed[start] += int(bool(after - before) and bool(before - after) and bool((got["S"] & ~c["tool"]).any()))
    assert min(fired.values()) >= 1 and min(changed.values()) >= 1 and copied >= 1 and wrong_order >= 1, (fired, changed, copied, wrong_order)
    kinds = {"fits" if len(t) == 1 else "topk" if t[-1][1] < 5 else "knn" for r in fx["runs"] for t in r["trail"][1:]}
    assert {"fits", "topk"} <= kinds


def test_the_restatement_agrees_with_the_oracles_single_graph_builder():
    """The oracle's builder (plane values from float64 differences, the reference's own formula) and the restatement (the kernel's
    fp32 differences) give the same graphs on the fixture's calls: the ranking margins of the fixture cover the difference."""
    _, calls = _calls()
    for c in calls:
        bd = dict(zip(SR.BOUND_KEYS, c["bounds"]))
        r, s = O.construct_edges_from_states(c["cloud"], ADJ, c["mask"], c["tool"], topk=c["topk"], connect_tools_all=False,
                                             connect_tools_surface=True, connect_tool_all_non_fixed=True, kNN=c["kNN"], **bd)
        got = SR.chained(c["cloud"], ADJ, c["mask"], c["tool"], c["topk"], False, True, c["kNN"], c["rows"], c["pad"], RATIO, c["order"])
        assert np.array_equal(r, got["recv"]) and np.array_equal(s, got["send"]), (c["j"], c["bi"], c["ai"])


def test_the_two_bound_orders_agree_at_ratio_one_and_differ_below_it():
    rng = np.random.default_rng(1)
    rows = rng.uniform(0.5, 2.0, (17, 3)).astype(F32)
    assert np.array_equal(SR.bounds6(rows, 0, 1.0, 0), SR.bounds6(rows, 0, 1.0, 1))
    a, b = SR.bounds6(rows, 0, 0.8, 0), SR.bounds6(rows, 0, 0.8, 1)
    assert np.array_equal(a[:4], b[:4]) and a[4] != b[4] and a[5] != b[5]
    assert np.array_equal(a, np.array([O.surface_bounds(rows, 0.8)[k] for k in SR.BOUND_KEYS], F32))          # the step loop's order
    from adaptigraph_amd.dataset import start_graph_bounds
    from adaptigraph_amd.rollout import surface_bounds
    assert np.array_equal(a, np.array([surface_bounds(rows, 0.8)[k] for k in SR.BOUND_KEYS], F32))
    assert np.array_equal(b, np.array([start_graph_bounds(rows, 0.8)[k] for k in SR.BOUND_KEYS], F32))
    padded = SR.bounds6(rows, 24, 0.8, 1)                                                                      # the zero row takes part
    assert padded[1] == 0.0 and np.array_equal(padded, np.array([start_graph_bounds(np.concatenate([rows, np.zeros((7, 3), F32)]), 0.8)[k]
                                                                 for k in SR.BOUND_KEYS], F32))
    nan = rows.copy()
    nan[3, 0] = np.nan
    got = SR.bounds6(nan, 0, 0.8, 0)
    assert np.isnan(got[[2, 4]]).all() and not np.isnan(got[[0, 1, 3, 5]]).any()


# ------------------------------------------------------------------------------------------------ chaining, with a stub engine
class _StubLib:
    """Records the launches rule_attempt / backoff_rounds would make; writes the edge counts it is told to into the outputs, and a
    base launch marks each graph it builds: recv[b, 0] = 100 * topk + b."""

    def __init__(self, counts):
        self.calls, self.counts = [], counts

    def _write(self, ptr, B, kind):
        out = (C.c_int32 * B).from_address(ptr)
        for b in range(B):
            out[b] = self.counts[kind].pop(0)

    def ag_build_edges_graphs(self, ctx, stream, pos, bstride, mask, tool, B, N, thr2, cull, topk, all_, cap, recv, send, rp, n):
        self.calls.append(("base", B, topk, cap))
        self._write(n.value, B, "base")
        out = (C.c_int32 * (B * cap)).from_address(recv.value)
        for b in range(B):
            out[b * cap] = 100 * topk + b
        return 0

    def ag_edges_nonfixed_rule_graphs(self, ctx, stream, ref):
        a = ref._obj
        self.calls.append(("nonfixed", a.B, a.base_cap, a.edge_cap, a.d_send_in, a.d_send, a.pad_rows))
        self._write(a.d_n_edges_out, a.B, "nonfixed")
        return 0

    def ag_edges_surface_rule_graphs(self, ctx, stream, ref):
        a = ref._obj
        self.calls.append(("surface", a.B, a.base_cap, a.edge_cap, a.d_send_in, a.d_send, a.pad_rows, a.bounds_order))
        self._write(a.d_n_edges_out, a.B, "surface")
        return 0


class _StubEngine:
    ctx = None

    def __init__(self, counts):
        self.lib = _StubLib(counts)

    def check(self, rc):
        assert rc == 0


def _graphs(B, N, cap):
    from adaptigraph_amd.graph import EdgeList
    z = lambda *s: torch.zeros(s, dtype=torch.int32)                      # noqa: E731
    return EdgeList(z(B, cap), z(B, cap), z(B, N + 1), z(B), N)


@pytest.fixture()
def cpu_stream(monkeypatch):
    import adaptigraph_amd.graph as G
    monkeypatch.setattr(G, "current_stream", lambda dev: C.c_void_p(0))


def _inputs(B, N):
    mask = torch.ones((B, N), dtype=torch.uint8)
    tool = torch.zeros((B, N), dtype=torch.uint8)
    tool[:, -2:] = 1
    pos = torch.zeros((B, N, 3))
    bnd = (pos.view(-1, 3), torch.arange(B, dtype=torch.int64) * N, None, torch.full((B,), N - 2, dtype=torch.int32), 7)
    return pos, mask, tool, bnd


def test_rule_attempt_chains_the_surface_launch_behind_the_non_fixed_one(cpu_stream):
    from adaptigraph_amd.graph import RuleConfig, rule_attempt
    B, N, wide, cap = 3, 10, 70, 40
    pos, mask, tool, bnd = _inputs(B, N)
    knn = torch.ones(B, dtype=torch.float64)
    base = _graphs(B, N, wide)
    # neither rule: the base graphs themselves, no launch
    eng = _StubEngine({})
    assert rule_attempt(RuleConfig(False, 2, 0.8, engine=eng), pos, 0, mask, tool, base, knn, bnd, cap) is base and eng.lib.calls == []
    # the non-fixed rule alone: one launch, straight into `out` (what it did before this rule existed)
    eng = _StubEngine(dict(nonfixed=[5, 6, 7]))
    out = _graphs(B, N, cap)
    got = rule_attempt(RuleConfig(True, 2, 0.8, engine=eng), pos, 0, mask, tool, base, knn, bnd, cap, out=out)
    assert got is out and [c[0] for c in eng.lib.calls] == ["nonfixed"] and eng.lib.calls[0][2:6] == (wide, cap, base.send.data_ptr(), out.send.data_ptr())
    assert out.n_edges.tolist() == [5, 6, 7]
    # the surface rule alone: directly on the base graphs
    eng = _StubEngine(dict(surface=[1, 2, 3]))
    out = _graphs(B, N, cap)
    got = rule_attempt(RuleConfig(False, 2, 0.8, engine=eng, surface=True, bounds_order=1), pos, 0, mask, tool, base, knn, bnd, cap, out=out)
    assert got is out and [c[0] for c in eng.lib.calls] == ["surface"]
    assert eng.lib.calls[0][2:] == (wide, cap, base.send.data_ptr(), out.send.data_ptr(), 7, 1) and out.n_edges.tolist() == [1, 2, 3]
    # both: the graphs between them live in a buffer as wide as the base graphs', the surface launch reads it and writes `out`
    eng = _StubEngine(dict(nonfixed=[50, 60, 65], surface=[30, 41, 39]))
    out = _graphs(B, N, cap)
    got = rule_attempt(RuleConfig(True, 2, 0.8, engine=eng, surface=True), pos, 0, mask, tool, base, knn, bnd, cap, out=out)
    nf, sf = eng.lib.calls
    assert got is out and (nf[0], sf[0]) == ("nonfixed", "surface")
    assert nf[2:5] == (wide, wide, base.send.data_ptr()) and nf[5] not in (base.send.data_ptr(), out.send.data_ptr())
    assert sf[2:6] == (wide, cap, nf[5], out.send.data_ptr()) and sf[7] == 0
    assert out.n_edges.tolist() == [30, 41, 39]


def test_backoff_rounds_rerun_both_rules_in_every_attempt(cpu_stream):
    """Graph 0 fits; graph 1 lowers kNN once (the base graph stands, both rules rerun); graph 2 is at its minimum kNN and lowers
    top-k (the base graph is rebuilt, both rules rerun).  One read-back per round, the fitting rows copied into el."""
    from adaptigraph_amd.graph import BackoffPlan, RuleConfig, backoff_rounds, rule_attempt
    B, N, wide, max_nR = 3, 10, 70, 40
    pos, mask, tool, bnd = _inputs(B, N)
    thr2 = cull = torch.ones(B)
    base = _graphs(B, N, wide)
    eng = _StubEngine(dict(nonfixed=[50, 60, 65, 55, 58], surface=[30, 41, 45, 38, 36], base=[44]))
    cfg = RuleConfig(True, 2, 0.8, engine=eng, surface=True)
    knn0 = [0.5, 0.5, 0.4]
    el = rule_attempt(cfg, pos, 0, mask, tool, base, torch.tensor(knn0, dtype=torch.float64), bnd, max_nR)
    plan = BackoffPlan(knn0, 5, max_nR, 0.4, 0.1)
    assert plan.record(el.n_edges.numpy()) == [0] and plan.active == [1, 2]
    del eng.lib.calls[:]
    backoff_rounds(cfg, plan, el, base, pos, mask, tool, thr2, cull, bnd)
    assert [c[0] for c in eng.lib.calls] == ["nonfixed", "surface", "base", "nonfixed", "surface"]        # top-k 5 group, then top-k 4
    assert eng.lib.calls[2][1:3] == (1, 4) and all(c[1] == 1 for c in eng.lib.calls)
    assert plan.rounds == 2 and not plan.active and el.n_edges.tolist() == [30, 38, 36]
    assert plan.trail == [[(0.5, 5, 30)], [(0.5, 5, 41), (0.4, 5, 38)], [(0.4, 5, 45), (0.4, 4, 36)]]
    assert plan.has_rule                                                  # (still "the non-fixed rule is on")


def test_attempt_with_backoff_on_a_config_with_neither_rule_is_the_top_k_loop(cpu_stream):
    """The counts of tests/golden/dataset_backoff's four trails (top-k 20, max_nR 260) fed to attempt_with_backoff under a RuleConfig
    with neither rule: only base launches, one per round at top-k 19, 18, ..., 4 on the sub-batch that is still over max_nR (two
    graphs down to top-k 8, then one), each into buffers of the base graphs' capacity; the fixture's trails; a graph that fits lands
    in its own row of the result and in no other."""
    from adaptigraph_amd.graph import BackoffPlan, RuleConfig, attempt_with_backoff
    trails = [[tuple(a) for a in t] for t in DR.load_fixture("dataset_backoff")["trail"]]
    assert [len(t) for t in trails] == [1, 1, 17, 13]
    B, N, topk, max_nR = 4, 10, 20, 260
    pos, mask, tool, _ = _inputs(B, N)
    thr2 = cull = torch.ones(B)
    base = _graphs(B, N, max_nR)
    base.n_edges[:] = torch.tensor([t[0][2] for t in trails], dtype=torch.int32)
    later = [t[r][2] for r in range(1, 17) for t in trails if len(t) > r]                     # round by round, in graph order
    eng = _StubEngine(dict(base=list(later)))
    plan = BackoffPlan([1.0] * B, topk, max_nR, 1.0, 0.1, has_rule=False)
    el = attempt_with_backoff(RuleConfig(False, 2, 1.0, engine=eng), plan, pos, 0, base, None, pos, mask, tool, thr2, cull, None, max_nR)
    assert el is base and eng.lib.counts["base"] == []
    assert eng.lib.calls == [("base", 2 if k >= 8 else 1, k, max_nR) for k in range(19, 3, -1)]
    assert plan.rounds == 17 and not plan.active and plan.trail == trails
    assert el.n_edges.tolist() == [t[-1][2] for t in trails] == [112, 185, 253, 255]
    # rows 0 and 1 were never rebuilt; row 2 is graph 0 of the top-k 4 launch, row 3 graph 1 of the top-k 8 launch
    assert el.recv[:, 0].tolist() == [0, 0, 400, 801]


def test_knn_attempts_without_the_rule_cost_no_launch_and_no_round(cpu_stream):
    """has_rule=False with a kNN above min_kNN: the kNN attempts are recorded with the unchanged count - no launch, no round -, then
    top-k goes down.  The plan's kNN values are the device's draws, read with the counts."""
    from adaptigraph_amd.graph import BackoffPlan, RuleConfig, attempt_with_backoff
    B, N, max_nR = 2, 10, 40
    pos, mask, tool, _ = _inputs(B, N)
    thr2 = cull = torch.ones(B)
    base = _graphs(B, N, max_nR)
    base.n_edges[:] = torch.tensor([50, 30], dtype=torch.int32)
    eng = _StubEngine(dict(base=[35]))
    plan = BackoffPlan([1.0] * B, 5, max_nR, 0.4, 0.1, has_rule=False)
    knn = torch.tensor([0.6, 0.4], dtype=torch.float64)
    el = attempt_with_backoff(RuleConfig(False, 2, 1.0, engine=eng), plan, pos, 0, base, knn, pos, mask, tool, thr2, cull, None, max_nR,
                              read_knn=True)
    assert eng.lib.calls == [("base", 1, 4, max_nR)] and plan.rounds == 2 and not plan.active
    k1 = 0.6 - 0.1
    k2 = k1 - 0.1
    assert k2 <= 0.4 and plan.trail == [[(0.6, 5, 50), (k1, 5, 50), (k2, 5, 50), (k2, 4, 35)], [(0.4, 5, 30)]]
    assert el is base and el.n_edges.tolist() == [35, 30] and el.recv[:, 0].tolist() == [400, 0]


def test_the_fixture_meta_lists_what_the_generator_asserted():
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_batch_surface.npz"))
    meta = json.loads(bytes(g["meta_json"]).decode())
    c = meta["conditions"]
    assert min(c["fired"].values()) >= 1 and min(c["adds_and_removes"].values()) >= 1 and c["copied"] >= 1 and c["orders_differ"] >= 1
    assert {"fits", "topk"} <= set(meta["kinds"])
    for k in ("radius", "topk", "y", "knn", "side"):
        assert float(g["margin_" + k]) >= 1e-4, k
    assert float(g["margin_rank_abs"]) > 0 and float(g["margin_rank_rel"]) >= 1e-3
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "eval_batch_surface.npz")) < (1 << 20)
