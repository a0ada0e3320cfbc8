"""GPU checks of the batched open-loop eval rollout (-m gpu): ag_eval_step's advance kernel against the float64 restatement
(tests/eval_restate.py), adaptigraph_amd.rollout_eval_batch against the reference's own rollouts (tests/golden/eval_batch_*.npz),
its independence of order and batch, the graph-by-graph path, the waits and the overflow."""
import copy
import ctypes as C
import time

import numpy as np
import pytest
import torch

import eval_restate as ER
import train_restate as TR
from test_gpu_parity import POS_TOL
from test_gpu_train import _model

pytestmark = pytest.mark.gpu

FIXTURES = ["eval_batch_rope", "eval_batch_rest"]
# ag_forward's kernel family at B = 1 and B = 4 (N = 26): the n_his = 4 model takes the latency-mode chains at both sizes (a
# handful of 128-row workgroups either way), the n_his = 5 model has no latency-mode image and takes the throughput chains at both.
# So in BOTH fixtures the family is the same at both sizes and the predictions must be bit-equal.
SAME_FAMILY = {"eval_batch_rope": True, "eval_batch_rest": True}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_CACHE = {}


def _case(name, dev):
    """(fixture, dataset, model, draws, the B = 4 result), built once."""
    import adaptigraph_amd as ag
    if name not in _CACHE:
        fx = ER.load_fixture(name)
        ds = ag.DeviceDynDataset(*ER.dataset_args(fx), device=dev, phase="valid")
        n_his = fx["dataset_config"]["n_his"]
        model = _model(dev, TR.make_weights(fx["w_seed"], n_his=n_his), n_his=n_his, pstep=3, material=fx["material"])
        dr = ds.eval_draws(fx["samples"], fps_start=fx["fps_start"], rad_start=fx["rad_start"])
        res = ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr, keep_pred=True)
        _CACHE[name] = (fx, ds, model, dr, res)
    return _CACHE[name]


def _edges_at(res, s, b):
    e = res.edges[s]
    n = int(e.n_edges[b])
    return e.recv[b, :n].cpu().numpy(), e.send[b, :n].cpu().numpy()


def _nn(t):
    """NaN padding made comparable (no error and no coordinate here is -9)."""
    return torch.nan_to_num(t, nan=-9.0)


def _trail(t):
    return [(float(a), int(k), int(c)) for a, k, c in t]


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _advance(dev, engine, n_his, rest, obj, eef, state, pred, fps_idx, n_obj, frames, topk=5, adj=0.5, cap=4096, sentinel=None):
    """ag_eval_step with pred_given on B graphs -> (err, state_next, action_next, n_edges_next) as numpy.  obj (P, 3), eef (Q, 3)
    flat buffers; state (B, n_his, N, 3); pred (B, max_nobj, 3); frames (B, 3)."""
    from adaptigraph_amd import _lib
    from adaptigraph_amd.context import current_stream
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)   # noqa: E731
    B, No = pred.shape[:2]
    N = state.shape[2]
    d_obj, d_eef = t(obj, torch.float32), t(np.concatenate([eef, np.zeros((1, 3), np.float32)]), torch.float32)
    d_state, d_pred = t(state, torch.float32), t(pred, torch.float32)
    d_idx, d_n, d_fr = t(fps_idx, torch.int32), t(n_obj, torch.int32), t(frames, torch.int64)
    mask = np.zeros((B, N), np.uint8)
    for b in range(B):
        mask[b, :n_obj[b]] = 1
    mask[:, No:] = 1
    tool = np.zeros((B, N), np.uint8)
    tool[:, No:] = 1
    d_mask, d_tool = t(mask, torch.uint8), t(tool, torch.uint8)
    thr2 = torch.full((B,), float(np.float32(adj * adj)), dtype=torch.float32, device=dev)
    cull = torch.full((B,), float(np.nextafter(np.float32(adj), np.float32(np.inf))), dtype=torch.float32, device=dev)
    fill = float("nan") if sentinel is None else sentinel
    err = torch.full((B,), -1.0, dtype=torch.float32, device=dev)
    nstate = torch.full((B, n_his, N, 3), fill, dtype=torch.float32, device=dev)
    nact = torch.full((B, N, 3), fill, dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    recv, send = torch.zeros((B, cap), **i32), torch.zeros((B, cap), **i32)
    rptr, cnt, status = torch.zeros((B, N + 1), **i32), torch.full((B,), -1, **i32), torch.zeros(4, **i32)
    a = _lib.AgEvalStepArgs()
    a.d_state, a.d_obj_pos, a.d_eef_pos = d_state.data_ptr(), d_obj.data_ptr(), d_eef.data_ptr()
    a.d_fps_idx, a.d_n_obj, a.d_frames = d_idx.data_ptr(), d_n.data_ptr(), d_fr.data_ptr()
    a.d_state_mask, a.d_eef_mask, a.d_thr2, a.d_cull = d_mask.data_ptr(), d_tool.data_ptr(), thr2.data_ptr(), cull.data_ptr()
    a.obj_points, a.eef_points = len(obj), len(eef)
    a.B, a.max_nobj, a.n_eef, a.n_inst, a.edge_cap, a.edge_rows = B, No, N - No, 1, cap, cap
    a.topk, a.connect_tools_all, a.store_rest_state, a.pred_given, a.step, a.err_stride = topk, 0, int(rest), 1, 0, B
    a.d_pred, a.d_err, a.d_state_next, a.d_action_next = d_pred.data_ptr(), err.data_ptr(), nstate.data_ptr(), nact.data_ptr()
    a.d_recv_next, a.d_send_next, a.d_row_ptr_next, a.d_n_edges_next = recv.data_ptr(), send.data_ptr(), rptr.data_ptr(), cnt.data_ptr()
    a.d_status = status.data_ptr()
    engine.check(engine.lib.ag_eval_step(engine.ctx, current_stream(dev), C.byref(a)))
    torch.cuda.synchronize()
    return err.cpu().numpy(), nstate.cpu().numpy(), nact.cpu().numpy(), cnt.cpu().numpy()


def _err_ok(got, want64):
    """fp64 accumulation of <= 4096 terms of relative error ~1e-16 each, then ONE rounding: float32(want64) or its neighbour."""
    w = np.float32(want64)
    return got == w or got == np.nextafter(w, np.float32(np.inf)) or got == np.nextafter(w, np.float32(-np.inf))


def _engine(dev, n_his):
    import adaptigraph_amd as ag
    return ag.Engine(dev, n_his=n_his, rel_dim=5 + 3 * n_his)


@pytest.mark.parametrize("name", FIXTURES)
def test_advance_kernel_teacher_forced_on_the_references_predictions(dev, name):
    """Every (rollout, step) of the fixture as one graph of ONE launch (19 graphs), fed the reference's own prediction."""
    fx = ER.load_fixture(name)
    dcfg = fx["dataset_config"]
    n_his, rest = dcfg["n_his"], dcfg["store_rest_state"]
    episode = np.asarray(fx["pair_lists"])[:, 0]
    n_e = [o.shape[1] for o in fx["obj_pos"]]
    obj_off = np.concatenate([[0], np.cumsum([o.shape[0] * o.shape[1] for o in fx["obj_pos"]])])
    eef_off = np.concatenate([[0], np.cumsum([e.shape[0] * e.shape[1] for e in fx["eef_pos"]])])
    obj = np.concatenate([o.reshape(-1, 3) for o in fx["obj_pos"]])
    eef = np.concatenate([e.reshape(-1, 3) for e in fx["eef_pos"]])
    n_eef = fx["eef_pos"][0].shape[1]
    rows = []
    for j, (i, r) in enumerate(zip(fx["samples"], fx["runs"])):
        e, L = int(episode[i]), len(r["idx_list"])
        for s in range(L):
            fr = [obj_off[e] + int(r["idx_list"][s][1]) * n_e[e], -1, 0]
            if s + 1 < L:
                fr[1:] = [eef_off[e] + int(r["idx_list"][s + 1][0]) * n_eef, eef_off[e] + int(r["idx_list"][s + 1][1]) * n_eef]
            rows.append((j, s, fr))
    state = np.stack([fx["runs"][j]["state"][s] for j, s, _ in rows])
    pred = np.stack([fx["runs"][j]["pred"][s] for j, s, _ in rows])
    err, ns, na, cnt = _advance(dev, _engine(dev, n_his), n_his, rest, obj, eef, state, pred, np.stack([fx["fps_idx"][j] for j, _, _ in rows]),
                                np.array([fx["n_obj"][j] for j, _, _ in rows]), np.array([fr for _, _, fr in rows], np.int64),
                                cap=dcfg["datasets"][0]["max_nR"] + 64, sentinel=-7.0)
    for b, (j, s, fr) in enumerate(rows):
        r = fx["runs"][j]
        print(f"{name} rollout {j} step {s}: err {err[b]!r} float64 {r['error64'][s]!r} reference {r['error_list'][s]!r}")
        assert _err_ok(err[b], r["error64"][s]), (j, s)
        if fr[1] >= 0:
            assert np.array_equal(ns[b], r["state"][s + 1]) and np.array_equal(na[b], r["action"][s + 1]), (j, s)
            assert cnt[b] == r["trail"][s + 1][0][2], (j, s)              # the next graph's first attempt, the true count
        else:
            assert (ns[b] == -7.0).all() and (na[b] == -7.0).all() and cnt[b] == 0, (j, s)


def test_advance_kernel_on_a_synthetic_case_past_one_workgroup_pass(dev):
    """max_nobj 300 with n_obj 257 and 300 (a second pass of the 256-thread loop, full and one row), n_obj 1, n_his 5 with the
    rest frame; a graph's results do not depend on its neighbour; a NaN prediction gives a NaN error; an ended graph writes
    nothing and builds an empty graph."""
    rng = np.random.default_rng(7)
    n_his, No, n_eef, n_e, T = 5, 300, 3, 700, 3
    N = No + n_eef
    obj = rng.normal(size=(T * n_e, 3)).astype(np.float32)
    eef = rng.normal(size=(T * n_eef, 3)).astype(np.float32)
    eng = _engine(dev, n_his)

    def run(n_objs, nan_at=None, ended=()):
        B = len(n_objs)
        r = np.random.default_rng(11)
        state = r.normal(size=(2, n_his, N, 3)).astype(np.float32)[:B]
        pred = (r.normal(size=(2, No, 3)) * 0.3).astype(np.float32)[:B]
        idx = np.stack([r.permutation(n_e)[:No] for _ in range(2)]).astype(np.int32)[:B]
        # graph 0 and graph 1 keep their own inputs whatever n_objs says: graph 1 is the same in every launch
        for b in range(B):
            idx[b, n_objs[b]:] = -1
        if nan_at is not None:
            pred[nan_at] = np.nan
        frames = np.array([[1 * n_e, 2 * n_eef, 1 * n_eef], [2 * n_e, 0, 2 * n_eef]], np.int64)[:B]
        for b in ended:
            frames[b, 1] = -1
        out = _advance(dev, eng, n_his, True, obj, eef, state, pred, idx, np.array(n_objs), frames, cap=N * 8, sentinel=-7.0)
        return state, pred, idx, frames, out

    for n_objs in ([257, 300], [1, 300]):
        state, pred, idx, frames, (err, ns, na, cnt) = run(n_objs)
        for b in range(2):
            want = ER.error64(pred[b], obj[frames[b, 0]:frames[b, 0] + n_e], idx[b], n_objs[b])
            print(f"n_obj {n_objs[b]}: err {err[b]!r} float64 {want!r}")
            assert _err_ok(err[b], want), (n_objs, b)
            ws, wa = ER.advance(state[b], pred[b], eef[frames[b, 1]:frames[b, 1] + n_eef], eef[frames[b, 2]:frames[b, 2] + n_eef], True)
            assert np.array_equal(ns[b], ws) and np.array_equal(na[b], wa), (n_objs, b)
            assert cnt[b] > 0
        if n_objs[0] == 257:
            first, first0 = (err[1], ns[1].copy(), na[1].copy(), cnt[1]), err[0]
        else:                                                 # graph 1 next to another neighbour: the same bits
            assert err[1] == first[0] and np.array_equal(ns[1], first[1]) and np.array_equal(na[1], first[2]) and cnt[1] == first[3]
    # a NaN in a sampled row of a graph that ended (its prediction goes nowhere else): NaN error, nothing written, no edges
    _, _, _, _, (err, ns, na, cnt) = run([257, 300], nan_at=(1, 299, 1), ended=(1,))
    assert np.isnan(err[1]) and err[0] == first0
    assert (ns[1] == -7.0).all() and (na[1] == -7.0).all() and cnt[1] == 0 and not (ns[0] == -7.0).any()


# ------------------------------------------------------------------------------------------------ 2. free-running
@pytest.mark.parametrize("name", FIXTURES)
def test_free_running_rollouts_equal_the_reference(dev, name):
    fx, ds, _, _, res = _case(name, dev)
    B = len(fx["samples"])
    want_len = [len(r["idx_list"]) for r in fx["runs"]]
    assert res.lengths.tolist() == want_len and res.errors.shape == (max(want_len), B) and res.errors.dtype == torch.float32
    assert [[tuple(p) for p in s] for s in res.schedule] == [[tuple(int(v) for v in p) for p in r["idx_list"]] for r in fx["runs"]]
    errors, pred = res.errors.cpu().numpy(), res.pred.cpu().numpy()
    bar = np.sqrt(3.0) * POS_TOL + fx["ref_gap"]              # the mean of norms is 1-Lipschitz in the positions
    worst_p = worst_e = 0.0
    for j, r in enumerate(fx["runs"]):
        L = want_len[j]
        assert np.isnan(errors[L:, j]).all() and np.isnan(pred[L:, j]).all() and not np.isnan(errors[:L, j]).any()
        assert [_trail(t) for t in res.trails[j]] == r["trail"], j
        for s in range(L):
            recv, send = _edges_at(res, s, j)
            assert np.array_equal(recv, r["recv"][s]) and np.array_equal(send, r["send"][s]), (j, s)
            worst_p = max(worst_p, float(np.abs(pred[s, j] - r["pred"][s]).max()))
            worst_e = max(worst_e, float(np.abs(np.float64(errors[s, j]) - np.float64(r["error_list"][s]))))
    print(f"{name}: max |pred - reference| {worst_p:.3e} (bar {POS_TOL:.0e}), max |error - error_list| {worst_e:.3e} (bar {bar:.3e})")
    assert worst_p <= POS_TOL and worst_e <= bar
    se = res.step_error()
    assert se.shape == (min(want_len), B) and np.array_equal(se, errors[:min(want_len)].astype(np.float64))
    s = res.summary()
    assert np.array_equal(s["median"], np.median(se, axis=1)) and s["p25"].shape == s["p75"].shape == (min(want_len),)


# ------------------------------------------------------------------------------------------------ 3. order and batch
def _same_graphs(res_a, ja, res_b, jb, L):
    for s in range(L):
        ra, sa = _edges_at(res_a, s, ja)
        rb, sb = _edges_at(res_b, s, jb)
        assert np.array_equal(ra, rb) and np.array_equal(sa, sb), (ja, jb, s)
    assert res_a.trails[ja] == res_b.trails[jb]


@pytest.mark.parametrize("name", FIXTURES)
def test_permuted_and_single_rollouts_equal_the_batch(dev, name):
    import adaptigraph_amd as ag
    fx, ds, model, dr, res = _case(name, dev)
    from adaptigraph_amd.rollout import _take
    perm = np.array([2, 0, 3, 1])
    rp = ag.rollout_eval_batch(model, ds, fx["samples"][perm], draws=_take(dr, perm), keep_pred=True)
    assert rp.lengths.tolist() == res.lengths[perm].tolist() and rp.schedule == [res.schedule[p] for p in perm]
    assert torch.equal(_nn(rp.errors), _nn(res.errors[:, perm])) and torch.equal(_nn(rp.pred), _nn(res.pred[:, perm]))   # same B, same kernels: bits
    for k, p in enumerate(perm):
        _same_graphs(rp, k, res, int(p), int(res.lengths[p]))
    for j in range(len(fx["samples"])):
        one = ag.rollout_eval_batch(model, ds, fx["samples"][j:j + 1], draws=_take(dr, [j]), keep_pred=True)
        L = int(res.lengths[j])
        assert one.lengths.tolist() == [L] and one.errors.shape == (L, 1)
        _same_graphs(one, 0, res, j, L)
        diff = float((one.pred[:, 0] - res.pred[:L, j]).abs().max())
        print(f"{name} rollout {j}: max |pred(B=1) - pred(B=4)| {diff:.3e}")
        assert diff <= POS_TOL
        if SAME_FAMILY[name]:
            assert torch.equal(one.pred[:, 0], res.pred[:L, j]) and torch.equal(one.errors[:, 0], res.errors[:L, j])


# ------------------------------------------------------------------------------------------------ 4. graph by graph
def test_per_graph_path_equals_the_batched_path(dev):
    import adaptigraph_amd as ag
    name = "eval_batch_rope"
    fx, ds, model, dr, res = _case(name, dev)
    pg = ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr, keep_pred=True, per_graph=True)
    assert pg.lengths.tolist() == res.lengths.tolist() and pg.schedule == res.schedule
    for j in range(len(fx["samples"])):
        _same_graphs(pg, j, res, j, int(res.lengths[j]))
    assert torch.equal(_nn(pg.errors), _nn(res.errors))
    assert SAME_FAMILY[name] and torch.equal(_nn(pg.pred), _nn(res.pred))


def test_a_knn_range_without_a_tool_rule_equals_the_single_graph_paths(dev):
    """knn_range [0.4, 1.0] with min_knn 0.4 and no tool rule on the rope fixture: the back-off walks kNN down first (recorded, nothing
    rebuilt) and then top-k.  The batched build equals the sample-by-sample one and the batched rollout the graph-by-graph one.
    (The fixture's fourth rollout backs off at its start graph and inside the loop; without a rule kNN does not change a count.)"""
    import adaptigraph_amd as ag
    fx, _, model, _, _ = _case("eval_batch_rope", dev)
    args = [copy.deepcopy(a) for a in ER.dataset_args(fx)]
    args[0]["datasets"][0].update(knn_range=[0.4, 1.0], min_knn=0.4)
    ds = ag.DeviceDynDataset(*args, device=dev, phase="valid")
    sp = ds.spec
    assert not sp.connect_tool_all_non_fixed and not sp.connect_tool_surface and sp.min_kNN == 0.4 and not sp.batched_edges
    dr = ds.eval_draws(fx["samples"], fps_start=fx["fps_start"], rad_start=fx["rad_start"])
    built = {}
    for per_sample in (False, True):
        e = ds.batch(fx["samples"], dr, per_sample_edges=per_sample)["edges"]
        built[per_sample] = (e, [_trail(t) for t in ds.last_trail])
    (ea, ta), (eb, tb) = built[False], built[True]
    assert ta == tb and any(len(t) > 2 and t[1][0] < t[0][0] and t[-1][1] < sp.topk for t in ta)        # kNN went down, then top-k
    assert torch.equal(ea.n_edges, eb.n_edges) and torch.equal(ea.row_ptr, eb.row_ptr)
    for b, n in enumerate(ea.n_edges.tolist()):
        assert n <= sp.max_nR and torch.equal(ea.recv[b, :n], eb.recv[b, :n]) and torch.equal(ea.send[b, :n], eb.send[b, :n]), b
    res = ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr, keep_pred=True)
    pg = ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr, keep_pred=True, per_graph=True)
    assert pg.lengths.tolist() == res.lengths.tolist() and pg.schedule == res.schedule
    for j in range(len(fx["samples"])):
        _same_graphs(pg, j, res, j, int(res.lengths[j]))
    assert any(len(t) > 2 and t[1][0] < t[0][0] and t[-1][1] < sp.topk for tr in res.trails for t in tr[1:])  # inside the loop too
    assert torch.equal(_nn(pg.errors), _nn(res.errors)) and torch.equal(_nn(pg.pred), _nn(res.pred))


# ------------------------------------------------------------------------------------------------ 5. it enqueues
def test_eval_step_enqueues_and_the_rollout_waits_once_per_step(dev):
    import adaptigraph_amd as ag
    from adaptigraph_amd import rollout as R
    from adaptigraph_amd.context import current_stream
    fx, ds, model, dr, res = _case("eval_batch_rope", dev)
    # back-off attempts inside the loop (not the start graphs'): one sub-batch, hence one read, per attempt round of a step
    L_max = int(res.lengths.max())
    attempts = sum(max(len(tr[s]) - 1 for tr in res.trails if len(tr) > s) for s in range(1, L_max))
    assert attempts >= 1 and res.host_waits == L_max + attempts
    # one ag_eval_step behind a spin kernel: the call returns while the spin is still running
    data = ds.batch(fx["samples"], dr, with_fps=True)
    aux, eng, sp = ds._last_build, model.engine(dev), ds.spec
    B, N = len(fx["samples"]), ds.N
    kw = {k: v for k, v in data.items() if k.endswith("_physics_param")}
    inp = model._inputs(dev, data["state"], data["attrs"], None, None, data["p_instance"], data["action"], data["edges"], kw)
    attrs, action, phys, group, edges = inp.attrs, inp.action, inp.phys, inp.group, inp.edges
    tab = torch.tensor([[0, 0, ds.n_eef]] * B, dtype=torch.int64, device=dev)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    out = dict(pred=torch.empty((B, sp.max_nobj, 3), **f32), err=torch.empty((B,), **f32), state=torch.empty_like(data["state"]),
               action=torch.empty_like(action), recv=torch.empty_like(edges.recv), send=torch.empty_like(edges.send),
               rptr=torch.empty_like(edges.row_ptr), cnt=torch.empty_like(edges.n_edges), status=torch.zeros(4, **i32))
    a = R._eval_step_args(ds, B, sp.topk, edges.edge_cap)
    a.d_state, a.d_action, a.d_attrs, a.d_phys, a.d_group = (t.data_ptr() for t in (data["state"], action, attrs, phys, group))
    a.d_recv, a.d_send, a.d_row_ptr, a.d_n_edges = (t.data_ptr() for t in (edges.recv, edges.send, edges.row_ptr, edges.n_edges))
    a.d_fps_idx, a.d_n_obj, a.d_frames = data["fps_idx"].data_ptr(), data["n_obj"].data_ptr(), tab.data_ptr()
    a.d_state_mask, a.d_eef_mask, a.d_thr2, a.d_cull = (aux[k].data_ptr() for k in ("state_mask", "eef_mask", "thr2", "cull"))
    a.pred_given, a.step, a.err_stride = 0, 0, B
    a.d_pred, a.d_err, a.d_state_next, a.d_action_next = (out[k].data_ptr() for k in ("pred", "err", "state", "action"))
    a.d_recv_next, a.d_send_next, a.d_row_ptr_next, a.d_n_edges_next = (out[k].data_ptr() for k in ("recv", "send", "rptr", "cnt"))
    a.d_status = out["status"].data_ptr()
    call = lambda: eng.check(eng.lib.ag_eval_step(eng.ctx, current_stream(dev), C.byref(a)))   # noqa: E731
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    T = time.perf_counter() - t0                                   # host time of an enqueue on an idle stream
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(10_000_000)
    e1.record()
    torch.cuda.synchronize()
    ms_per_cycle = e0.elapsed_time(e1) / 10_000_000
    want_ms = max(100.0, 4e3 * T)
    done = torch.cuda.Event()
    torch.cuda._sleep(int(want_ms / ms_per_cycle))
    done.record()
    call()
    still_busy = not done.query()
    torch.cuda.synchronize()
    print(f"host time of ag_eval_step {T * 1e3:.2f} ms, spin {want_ms:.0f} ms")
    assert still_busy, "ag_eval_step waited for the GPU"
    fw, _ = model(**{k: v for k, v in data.items() if k in ("state", "attrs", "p_instance", "action", "edges") or k.endswith("_physics_param")})
    assert torch.equal(out["pred"], fw) and int(out["status"][0]) == 0                   # ag_forward's bits


# ------------------------------------------------------------------------------------------------ 6. overflow
def test_start_graphs_that_cannot_fit_raise_before_any_step(dev, monkeypatch):
    import adaptigraph_amd as ag
    from adaptigraph_amd import rollout as R
    fx, _, model, _, _ = _case("eval_batch_rope", dev)
    args = [copy.deepcopy(a) for a in ER.dataset_args(fx)]
    args[0]["datasets"][0]["max_nR"] = 1                           # (a graph keeps at least its self-loops)
    args[0]["datasets"][0]["topk"] = 1
    ds = ag.DeviceDynDataset(*args, device=dev, phase="valid")
    dr = ds.eval_draws(fx["samples"], fps_start=fx["fps_start"], rad_start=fx["rad_start"])
    steps, orig = [], R._eval_step_args
    monkeypatch.setattr(R, "_eval_step_args", lambda *a, **k: steps.append(1) or orig(*a, **k))      # every step fills one
    with pytest.raises(Exception, match="Exceeds max dims"):
        ag.rollout_eval_batch(model, ds, fx["samples"], draws=dr)
    torch.cuda.synchronize()
    assert not steps
