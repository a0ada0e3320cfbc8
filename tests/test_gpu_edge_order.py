"""Class-major work list of the relation encoder (-m gpu).  Option edge_order = 1 makes k_ell_index write a candidate's list of
non-self slots class by class - object-object slots by the signs and the dominant axis of pos_r - pos_s (24 classes), every
slot with a tool at either end last, slot order inside a class - where edge_order = 0 writes it in slot order.  k_edge_enc
stores a C row by slot and a row's chain does not depend on the lane that computes it, so every output must keep its bits:
each case runs the same rollout with edge_order 0 and 1 and asks for torch.equal on state_seqs, and for equal share_counts(),
rollout_counts() and overflow flag.  With the class-major list the fp32 relation-encoder chain takes the zero skip in the
tiles that start among the object-object classes (n_oo), so the crafted weights of tests/test_gpu_zero_skip.py are run under
edge_order = 1 with zero_skip 0 against 1 as well.

Shapes are tiny: 2-3 candidates, an 8 x 8 cloth + 1 tool (about 320 non-self edges: three 128-row tiles, the last one partial,
the tool class starting in the middle of a tile) or a rope of 64 + 1, 3 forwards.  The latency-mode chains are off unless a case
says otherwise, so the 128-row throughput kernels run."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import _cfg, _ppm, POS_TOL
from test_gpu_more import _task, _grid, _rope, _actions
from test_gpu_zero_skip import _craft, LIMITS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(latency=0, share_prefix=0)


def _census():
    spec = importlib.util.spec_from_file_location("zero_skip_census", os.path.join(ROOT, "tools", "zero_skip_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ag():
    import adaptigraph_amd
    return adaptigraph_amd


@pytest.fixture(scope="module")
def O():
    from oracle import adaptigraph_oracle
    return adaptigraph_oracle


@pytest.fixture(scope="module")
def models(ag, dev):
    """one model per material; the cases load their weights into it"""
    return {mat: ag.DynamicsPredictor(*_cfg(mat, 3), dev) for mat in ("rope", "cloth")}


def _load(m, W):
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})


def _cloud(material, rng):
    return _rope(64, rng) if material == "rope" else _grid(8, 0.3, 0.02, rng)


def _batch(material, rng, reps=(3, 3, 3)):
    """three candidates: one pushing into the object, one whose tool stays out of reach (no tool edge: n_oo == n_ns), one more"""
    cloud = _cloud(material, rng)
    a = _actions(cloud, 3, 1, np.asarray(reps), rng, spread=0.2)
    c = cloud.mean(0)
    a[0, 0, 0], a[0, 0, 1] = c[0] + 0.1, c[2] - 0.1            # starts on the object
    a[1, 0, 0] += 30.0                                         # never within adj_thresh of a particle
    return cloud, a


def _run(ag, m, dev, s0, a, ppm, order, call=None, **opts):
    """(state_seqs, share_counts, rollout_counts, overflow flag) of one rollout under edge_order = order"""
    eng = m.engine(dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    with eng.options(**{**BASE, **opts, "edge_order": order}):
        assert eng.get_option("edge_order") == order
        if call is None:
            out = ag.dynamics(s0, a, m, dev, ppm, _sync=False, _overflow_flag=flags)["state_seqs"]
        else:
            out = call()
        torch.cuda.synchronize()
        return out, eng.share_counts(), eng.rollout_counts(), flags.cpu().tolist()


def _same(r0, r1, finite=True):
    assert torch.equal(r0[0].view(torch.int32), r1[0].view(torch.int32)), float((r0[0] - r1[0]).abs().max())
    assert r0[1:] == r1[1:], (r0[1:], r1[1:])
    if finite:
        assert torch.isfinite(r0[0]).all()


def _both(ag, m, dev, s0, a, ppm, **opts):
    r0 = _run(ag, m, dev, s0, a, ppm, 0, **opts)
    r1 = _run(ag, m, dev, s0, a, ppm, 1, **opts)
    _same(r0, r1)
    return r1


@pytest.mark.parametrize("device_plan", [False, True])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_class_major_list_gives_the_same_bits(ag, O, dev, models, material, device_plan):
    """Cloth: classes straddle wavefront and tile boundaries, the tool class starts mid-tile, and candidate 1 has no tool edge.
    Rope along x: nearly every object-object edge falls into two of the 24 classes, most classes are empty."""
    rng = np.random.default_rng(503)
    task = _task(material, max_nR=40000, **(LIMITS if device_plan else {}))
    cloud, a_np = _batch(material, rng)
    m = models[material]
    _load(m, O.random_weights(503))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, material)
    got = []
    for share_first in (0, 1):
        got.append(_both(ag, m, dev, s0, a, ppm, share_first=share_first, device_decode=1 if device_plan else 0))
    assert torch.equal(got[0][0], got[1][0])
    assert got[1][1][1] > 0                                     # the shared first forward did share
    assert float((got[0][0][0] - got[0][0][1]).abs().max()) > 0  # pushed and untouched candidates differ
    if not device_plan:                                         # and the list that was reordered is the reference's
        want = O.dynamics(O.random_weights(503), 3, cloud, a_np, task)["state_seqs"]
        assert np.abs(got[0][0].cpu().numpy() - want).max() <= POS_TOL


def test_class_major_list_with_the_prefix_shared(ag, O, dev, models):
    rng = np.random.default_rng(509)
    task = _task("cloth", max_nR=40000)
    cloud, a_np = _batch("cloth", rng)
    m = models["cloth"]
    _load(m, O.random_weights(509))
    a_np[2, 0, 0] += 30.0                                       # two candidates out of reach: one base rollout serves both
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    r = _both(ag, m, dev, s0, a, _ppm(task, "cloth"), share_prefix=1, device_decode=0)
    assert r[2][0] < r[2][1]                                    # (executed counts the base rollout's forwards once)
    assert torch.equal(r[0], _run(ag, m, dev, s0, a, _ppm(task, "cloth"), 1, device_decode=0)[0])


@pytest.mark.parametrize("streams", [2, 4])
def test_class_major_list_over_two_chunks_on_streams(ag, O, dev, models, streams):
    rng = np.random.default_rng(521)
    task = _task("cloth", max_nR=40000)
    cloud, a_np = _batch("cloth", rng)
    m = models["cloth"]
    _load(m, O.random_weights(521))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    eng = m.engine(dev)
    whole = _run(ag, m, dev, s0, a, _ppm(task, "cloth"), 0, device_decode=0)
    eng.set_chunk(2)
    try:
        r = _both(ag, m, dev, s0, a, _ppm(task, "cloth"), streams=streams, stream_min_rows=0, device_decode=0)
    finally:
        eng.set_chunk(0)
    assert torch.equal(r[0], whole[0])


def test_class_major_list_of_a_masked_batch(ag, O, dev, models):
    rng = np.random.default_rng(523)
    task = _task("rope", max_nR=4000)
    m = models["rope"]
    _load(m, O.random_weights(523))
    B, n = 3, 100
    state = np.zeros((B, n, 3), np.float32)
    mask = np.zeros((B, n), bool)
    for b in range(B):
        state[b] = _rope(n, rng)
        mask[b] = rng.uniform(size=n) > (0.0, 0.2, 0.35)[b]
        state[b, ~mask[b]] = 0
    a = _actions(state[0], B, 1, [3, 2, 4], rng)[:, 0]
    args = (torch.from_numpy(state).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(a).to(dev))
    call = lambda: ag.dynamics_masked(*args, m, dev, _ppm(task, "rope"))["state_seqs"]
    for ragged in (1, 0):
        _same(_run(ag, m, dev, None, None, None, 0, call=call, ragged=ragged), _run(ag, m, dev, None, None, None, 1, call=call, ragged=ragged))


def test_class_major_list_with_five_history_frames(ag, dev):
    """n_his = 5: k_edge_enc<5> reads the reordered list (the softbody golden's model and batch)"""
    from helpers import load_golden, task_of
    g = load_golden("dyn_softbody_nhis5")
    task = task_of(g)
    mc, mat, ds = _cfg("softbody", 4)
    m = ag.DynamicsPredictor(mc, mat, dict(ds, n_his=5), dev)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("w::")})
    s0, a = torch.from_numpy(g["state0"]).to(dev), torch.from_numpy(g["action"]).to(dev)
    r = _both(ag, m, dev, s0, a, _ppm(task, "softbody"), device_decode=0)
    assert np.abs(r[0].cpu().numpy() - g["state_seqs"]).max() <= POS_TOL


def test_class_major_list_in_bf16x3_and_in_the_latency_chains(ag, O, dev, models):
    rng = np.random.default_rng(541)
    task = _task("cloth", max_nR=40000)
    cloud, a_np = _batch("cloth", rng)
    m = models["cloth"]
    _load(m, O.random_weights(541))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, "cloth")
    m.set_precision("bf16x3")
    try:
        _both(ag, m, dev, s0, a, ppm, device_decode=0)          # k_edge_enc_b3
    finally:
        m.set_precision("fp32")
    _both(ag, m, dev, s0, a[:1], ppm, latency=1, device_decode=0)   # a batch of one: k_edge_enc_lat


@pytest.mark.parametrize("device_plan", [False, True])
def test_class_major_list_with_a_candidate_that_has_no_forward_left(ag, O, dev, models, device_plan):
    """repeats 3, 0, 1: candidate 1 is never live and candidate 2 only at the first forward - its graph is then empty (n_ns = 0)"""
    rng = np.random.default_rng(547)
    task = _task("cloth", max_nR=40000, **(LIMITS if device_plan else {}))
    cloud, a_np = _batch("cloth", rng, reps=(3, 0, 1))
    m = models["cloth"]
    _load(m, O.random_weights(547))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    r = _both(ag, m, dev, s0, a, _ppm(task, "cloth"), share_first=0, device_decode=1 if device_plan else 0)
    assert r[2] == (4, 4)
    assert float(r[0][1, 0].abs().max()) == 0.0


def test_class_major_list_of_a_graph_over_max_nR(ag, O, dev, models):
    """a graph above max_nR is presented as empty downstream (zero_on_overflow) and reported: same outputs, same flag"""
    rng = np.random.default_rng(557)
    cloud, a_np = _batch("cloth", rng)
    m = models["cloth"]
    _load(m, O.random_weights(557))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    big = _both(ag, m, dev, s0, a, _ppm(_task("cloth", max_nR=40000), "cloth"), share_first=0, device_decode=0)
    assert big[3][0] == 0
    r0 = _run(ag, m, dev, s0, a, _ppm(_task("cloth", max_nR=350), "cloth"), 0, share_first=0, device_decode=0)
    r1 = _run(ag, m, dev, s0, a, _ppm(_task("cloth", max_nR=350), "cloth"), 1, share_first=0, device_decode=0)
    _same(r0, r1, finite=False)
    assert r1[3][0] > 350                                       # a pushed candidate's graph (65 x 5 slots + 64 tool edges) is over,
                                                                # the untouched one's (65 x 5) is not
    assert not torch.equal(r1[0].view(torch.int32), big[0].view(torch.int32))


def test_lds_fallbacks_give_the_same_list_users_the_same_bits(ag, O, dev, models):
    """65 particles x 6 slots = 390 slots = 7 bitmap words: 25 bitmaps need 175 words, two need 14, one needs 7.  The debug budget
    ell_lds_words walks 25 -> 2 -> 1 bitmaps (and 1 is the slot-order list)."""
    rng = np.random.default_rng(563)
    task = _task("cloth", max_nR=40000)
    cloud, a_np = _batch("cloth", rng)
    m = models["cloth"]
    _load(m, _craft(O.random_weights(563), "fixed"))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, "cloth")
    ref = _run(ag, m, dev, s0, a, ppm, 0, device_decode=0)
    for words in (0, 175, 174, 14, 13, 7, 1):                   # 25, 25, 2, 2, 1, 1, 1 bitmaps
        for share_first in (0, 1):
            r = _run(ag, m, dev, s0, a, ppm, 1, ell_lds_words=words, share_first=share_first, device_decode=0)
            assert torch.equal(r[0], ref[0]) and r[2:] == ref[2:], (words, share_first)


def _zs_pair(ag, m, dev, s0, a, ppm, active=1, **opts):
    out = []
    for zs in (1, 0):
        out.append(_run(ag, m, dev, s0, a, ppm, 1, zero_skip=zs, **opts))
        if zs:
            assert m.engine(dev).get_option("zero_skip_active") == active
    return out


@pytest.mark.parametrize("kind", ["fixed", "all_dead", "all_live"])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_edge_skip_on_the_class_major_list_gives_the_same_bits(ag, O, dev, models, material, kind):
    rng = np.random.default_rng(569)
    task = _task(material, max_nR=40000)
    cloud, a_np = _batch(material, rng)
    m = models[material]
    _load(m, _craft(O.random_weights(569), kind))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    for share_first in (0, 1):
        on, off = _zs_pair(ag, m, dev, s0, a, _ppm(task, material), share_first=share_first, device_decode=0)
        _same(on, off)
        _same(on, _run(ag, m, dev, s0, a, _ppm(task, material), 0, zero_skip=0, share_first=share_first, device_decode=0))


@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_edge_skip_decides_per_wavefront_of_the_class_major_list(ag, O, dev, models, material):
    """The keyed units 16 and 20 (one k-step) are made to be on where d = pos_r - pos_s is positive along one axis: x for the rope,
    z for the cloth (a flat sheet: the sign bit of d.z is the highest bit of the class key, so the classes with d.z < 0 lie together
    and fill whole wavefronts).  In slot order every full wavefront holds such an edge; in class-major order some wavefronts among
    the object-object classes hold none - checked on the oracle's edge list of candidate 0's first forward, reordered by the
    census tool's restatement of the key."""
    from test_gpu_zero_skip import DX_CUR, KEYED_0
    C = _census()
    col = 0 if material == "rope" else 2
    rng = np.random.default_rng(571)
    task = _task(material, max_nR=40000)
    cloud, a_np = _batch(material, rng)
    trace = []
    O.dynamics(O.random_weights(571), 3, cloud, a_np[:1] * np.array([1, 1, 1, 0], np.float32) + np.array([0, 0, 0, 1.5], np.float32),
               task, trace=trace)
    rec = trace[0][0]
    ns = np.flatnonzero(rec["recv"] != rec["send"])
    recv, send, pos = rec["recv"][ns], rec["send"][ns], rec["state_last"]
    perm, n_oo = C.work_list_order(recv, send, pos, 64, "class")
    assert 0 < n_oo < len(ns)                                  # candidate 0 has tool edges, behind the object-object ones
    slot = pos[recv, col] - pos[send, col]
    d = slot[perm]
    waves = [d[i:i + 32] for i in range(0, n_oo - n_oo % 32, 32)]           # the wavefronts wholly among the object-object classes
    on = [bool((w > 0).any()) for w in waves]
    assert any(on) and not all(on), "the keyed step must be dead in some wavefronts and live in others"
    assert all(bool((slot[i:i + 32] > 0).any()) for i in range(0, len(slot) - 31, 32))   # slot order: never a whole wavefront
    W = _craft(O.random_weights(571), "keyed", float(np.quantile(pos[recv, 0] - pos[send, 0], 0.97)), 0.0)
    w, b = W["relation_encoder.model.0.weight"], W["relation_encoder.model.0.bias"]
    for f in KEYED_0:                                          # on where d[col] > 0
        w[f, :] = 0.0
        w[f, DX_CUR + col] = 50.0
        b[f] = 0.0
    m = models[material]
    _load(m, W)
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    on_, off_ = _zs_pair(ag, m, dev, s0, a, _ppm(task, material), share_first=0, device_decode=0)
    _same(on_, off_)
    _same(on_, _run(ag, m, dev, s0, a, _ppm(task, material), 0, zero_skip=0, share_first=0, device_decode=0))


def test_an_inf_weight_turns_the_edge_skip_off_on_the_class_major_list(ag, O, dev, models):
    """as tests/test_gpu_zero_skip.py: 0 * inf must stay NaN, so the guard turns the skip off for the model; the class-major list
    changes nothing about that, NaNs included"""
    rng = np.random.default_rng(577)
    task = _task("cloth", max_nR=40000)
    cloud, a_np = _batch("cloth", rng, reps=(1, 1, 1))
    W = _craft(O.random_weights(577), "fixed")
    W["relation_encoder.model.2.weight"][3, 1] = np.inf
    W["relation_encoder.model.2.bias"][3] = 10.0
    m = models["cloth"]
    _load(m, W)
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    on, off = _zs_pair(ag, m, dev, s0, a, _ppm(task, "cloth"), active=0, share_first=0, device_decode=0)
    _same(on, off, finite=False)
    _same(on, _run(ag, m, dev, s0, a, _ppm(task, "cloth"), 0, zero_skip=0, share_first=0, device_decode=0), finite=False)
