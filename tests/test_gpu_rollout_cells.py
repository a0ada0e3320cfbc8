"""The rollout over cell-list graphs (-m gpu): adaptigraph_amd.dynamics_cells / dynamics_masked_cells (ag_rollout_cells).

Below the 4096-particle limit the yardstick is the existing drivers' own bits: dynamics() returns the same bits under every
combination of its options (tests/test_gpu_fuzz.py) and the cell builder's lists are the LDS builder's, so torch.equal is the bar.
Above the limit: the reference's own records (tests/golden/full_cloth_4097.npz, protocol of tests/test_gpu_fullsize_golden.py with
no tie verdict accepted - the fixture is chosen so that none is needed, tests/test_rollout_cells_fixture.py), the oracle on a
granular pile with five tool rows per candidate, and size-independent properties at 16,385 rows."""
import numpy as np
import pytest
import torch

import bench as BN
import cells_rollout_cases as CR
from helpers import load_golden, task_of, fullsize_records
from test_gpu_parity import _cfg, _ppm, POS_TOL
from test_gpu_more import _task, _grid, _rope, _actions, _model

pytestmark = pytest.mark.gpu


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


def _cloth(n_obj, rng):
    side = int(np.ceil(np.sqrt(n_obj)))
    return _grid(max(side, 1), 0.3, 0.02, rng)[:n_obj]


def _same(ag, s0, a, m, dev, ppm, **kw):
    """dynamics_cells == dynamics, bit for bit; returns the state tensor."""
    want = ag.dynamics(s0, a, m, dev, ppm, **kw)
    got = ag.dynamics_cells(s0, a, m, dev, ppm, **kw)
    assert got["state_seqs"].shape == want["state_seqs"].shape
    assert torch.equal(got["action_seqs"], want["action_seqs"])
    assert torch.equal(got["state_seqs"], want["state_seqs"])
    return got["state_seqs"]


# ------------------------------------------------------------------------------------------------- bit-equal below the limit
@pytest.mark.parametrize("N", [2, 64, 65, 257, 1029, 4096])
def test_equals_dynamics_at_every_size(ag, O, dev, N):
    """N_o + M = N on the cloth task (connect_tools_all, gripper offset): one candidate x one look-ahead step, and five candidates x
    two look-ahead steps (step 1 starts from the captured state) with mixed repeats, a 0 among them.  257 = two row blocks of the
    row kernels' grid, 4096 = the last size both drivers serve."""
    rng = np.random.default_rng(100 + N)
    task = _task("cloth", max_nR=40000)
    _, m = _model(ag, O, "cloth", 5, dev)
    cloud = _cloth(N - 1, rng)
    s0, ppm = torch.from_numpy(cloud).to(dev), _ppm(task, "cloth")
    one = _same(ag, s0, torch.from_numpy(_actions(cloud, 1, 1, 2, rng, spread=0.3)), m, dev, ppm)
    assert torch.isfinite(one).all() and float(one.abs().max()) > 0
    rep = np.array([[2, 1], [0, 2], [3, 0], [1, 1], [2, 3]], np.float32)
    five = _same(ag, s0, torch.from_numpy(_actions(cloud, 5, 2, rep, rng, spread=0.3)), m, dev, ppm)
    assert m.engine(dev).rollout_counts() == (int(rep.sum()), int(rep.sum()))            # live candidates only
    assert torch.count_nonzero(five[1, 0]) == 0 and torch.count_nonzero(five[2, 1]) == 0   # repeat 0: never captured (:32,:160)


@pytest.mark.parametrize("variant", ["rope_topk", "granular_pusher", "topk_ge_N", "phys_vec", "chunk2", "latency0", "latency1"])
def test_equals_dynamics_in_every_variant(ag, O, dev, variant):
    rng = np.random.default_rng(7)
    kw = {}
    if variant == "granular_pusher":                                    # 5-point pusher, top-k 20
        material, cloud = "granular", _grid(12, 0.12, 0.02, rng)
        task = _task("granular")
    elif variant == "topk_ge_N":
        material, cloud = "rope", _rope(60, rng)
        task = _task("rope", topk=100, max_nR=4000)
    else:                                                               # 1-point pusher; top-k 10 binds along the rope
        material, cloud = "rope", _rope(150, rng)
        task = _task("rope")
    _, m = _model(ag, O, material, 7, dev)
    eng = m.engine(dev)
    if variant == "phys_vec":
        kw["physics_param"] = {material: torch.from_numpy(rng.uniform(0.1, 0.9, cloud.shape[0]).astype(np.float32))}
    rep = np.array([[2, 1], [1, 2], [3, 1], [1, 0], [2, 2]], np.float32)
    a = torch.from_numpy(_actions(cloud, 5, 2, rep, rng, spread=0.3))
    s0, ppm = torch.from_numpy(cloud).to(dev), _ppm(task, material)
    if variant == "chunk2":
        eng.set_chunk(2)                                                # three chunks, the last one short
        try:
            got = ag.dynamics_cells(s0, a, m, dev, ppm)["state_seqs"]
        finally:
            eng.set_chunk(0)
        assert torch.equal(got, ag.dynamics(s0, a, m, dev, ppm)["state_seqs"])
        assert torch.equal(got, ag.dynamics_cells(s0, a, m, dev, ppm)["state_seqs"])
    elif variant.startswith("latency"):
        with eng.options(latency=int(variant[-1])):
            got = ag.dynamics_cells(s0, a, m, dev, ppm)["state_seqs"]
        assert torch.equal(got, ag.dynamics(s0, a, m, dev, ppm)["state_seqs"])
    else:
        _same(ag, s0, a, m, dev, ppm, **kw)


def test_equals_dynamics_with_the_softbody_model(ag, dev):
    """n_his 5, pstep 4 (the row kernels' second instantiation), on the reference's own golden inputs."""
    g = load_golden("dyn_softbody_nhis5")
    task = task_of(g)
    mc, mat, ds = _cfg("softbody", 4)
    m = ag.DynamicsPredictor(mc, mat, dict(ds, n_his=5), dev)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("w::")})
    s0, a = torch.from_numpy(g["state0"]).to(dev), torch.from_numpy(g["action"])
    got = _same(ag, s0, a, m, dev, _ppm(task, "softbody"))
    assert np.abs(got.cpu().numpy() - g["state_seqs"]).max() <= POS_TOL


@pytest.mark.parametrize("N_o", [64, 1028])
def test_masked_equals_dynamics_masked(ag, O, dev, N_o):
    """Prefix masks, a hole inside the prefix, one valid particle, non-zero padding rows; N_o + M = 65 and 1029.  The yardstick
    runs with its compact row list (ragged 1) and with dense rows (ragged 0)."""
    rng = np.random.default_rng(200 + N_o)
    task = _task("rope", max_nR=20000)
    _, m = _model(ag, O, "rope", 9, dev)
    cloud = _rope(N_o, rng)
    B = 5
    state = np.repeat(cloud[None], B, 0).copy()
    mask = np.zeros((B, N_o), bool)
    mask[0] = True                                                      # all valid
    mask[1, :N_o // 2] = True                                           # prefix
    mask[2, :N_o - 3] = True
    mask[2, 5:9] = False                                                # a hole inside the prefix
    mask[3, 0] = True                                                   # one valid particle
    mask[4, :N_o // 3] = True
    state[4, N_o // 3:] = rng.normal(0, 1, (N_o - N_o // 3, 3))         # non-zero padding rows
    a = _actions(cloud, B, 1, np.array([3, 2, 4, 1, 2], np.float32)[:, None], rng, spread=0.3)[:, 0]
    args = (torch.from_numpy(state).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(a))
    ppm = _ppm(task, "rope")
    got = ag.dynamics_masked_cells(*args, m, dev, ppm)
    assert m.engine(dev).rollout_counts() == (12, 12)
    for ragged in (1, 0):
        with m.engine(dev).options(ragged=ragged):
            want = ag.dynamics_masked(*args, m, dev, ppm)
        assert torch.equal(got["state_seqs"], want["state_seqs"]) and torch.equal(got["action_seqs"], want["action_seqs"]), ragged
    assert torch.isfinite(got["state_seqs"]).all()


# ------------------------------------------------------------------------------------------------- above the limit
class _WithWeights:
    """The fixture plus bench.random_weights(0) under the keys test_gpu_parity._model reads (the generator checked them equal and
    left the megabyte out of the file)."""

    def __init__(self, g):
        self.g, self.w = g, {"w::" + k: v for k, v in BN.random_weights(0).items()}
        self.files = list(g.files) + list(self.w)

    def __getitem__(self, k):
        return self.w[k] if k in self.w else self.g[k]


@pytest.fixture(scope="module")
def cloth4097(ag, dev):
    from test_gpu_parity import _model as model_of
    g = load_golden("full_cloth_4097")
    task = task_of(g)
    return g, task, model_of(ag, _WithWeights(g), "cloth", dev), fullsize_records(g, task)


def _masks(N_o, M, dev):
    mask = torch.ones((1, N_o + M), dtype=torch.bool, device=dev)
    tool = torch.zeros((1, N_o + M), dtype=torch.bool, device=dev)
    tool[:, N_o:] = True
    return mask, tool


def test_rollout_vs_reference_at_4097_rows(ag, dev, cloth4097):
    """tests/test_gpu_fullsize.py's _check_candidate with construct_edges_cells where it builds edges, and its first verdict only:
    1. teacher-forced edges bit-exact at every forward, 2. free-running positions within POS_TOL.  Both candidates, no tie excused."""
    g, task, m, traces = cloth4097
    N_o, M = g["state0"].shape[0], task["eef_num"]
    assert N_o + M == 4097
    ppm = _ppm(task, "cloth")
    s0, a = torch.from_numpy(g["state0"]).to(dev), torch.from_numpy(g["action"])
    with pytest.raises(NotImplementedError):
        ag.dynamics(s0, a, m, dev, ppm)                                 # the LDS-resident builder's limit stands
    out = ag.dynamics_cells(s0, a, m, dev, ppm)
    assert torch.equal(out["action_seqs"].cpu(), torch.from_numpy(g["action_seqs"]))
    seq = out["state_seqs"].cpu().numpy()
    mask, tool = _masks(N_o, M, dev)
    for b, (recs, capture, want) in enumerate(traces):
        for k, rec in enumerate(recs):
            el = ag.construct_edges_cells(torch.from_numpy(rec["state_last"][None]).to(dev), task["adj_thresh"], mask, tool,
                                          task["topk"], task["connect_tools_all"])
            n = int(el.n_edges[0])
            assert np.array_equal(el.recv[0, :n].cpu().numpy(), rec["recv"]) and np.array_equal(el.send[0, :n].cpu().numpy(), rec["send"]), (b, k)
        errs = [float(np.abs(x - w).max()) for x, w in zip(seq[b], want)]
        print(f"full_cloth_4097 candidate {b}: free-running error {max(errs):.2e}")
        assert max(errs) <= POS_TOL, (b, errs)


def test_single_forward_from_reference_history_at_4097_rows(ag, dev, cloth4097):
    """3. one forward from the reference's own history (every recorded forward of candidate 0): no edge decision involved."""
    from oracle import adaptigraph_oracle as O
    g, task, m, traces = cloth4097
    N_o, M = g["state0"].shape[0], task["eef_num"]
    N = N_o + M
    recs, _, _ = traces[0]
    attrs = np.zeros((1, N, 2), np.float32)
    attrs[:, :N_o, 0] = 1
    attrs[:, N_o:, 1] = 1
    dec, _ = O.decode_action(g["action"], task["push_length"])
    _, delta = O.tool_keypoints(dec, g["action"][..., 2], task)
    mask, tool = _masks(N_o, M, dev)
    action = np.zeros((1, N, 3), np.float32)
    action[0, N_o:] = delta[0, 0]
    for f in range(len(recs)):
        hist = np.stack([recs[max(0, f - 3 + h)]["state_last"] for h in range(4)])[None]
        state = torch.from_numpy(hist).to(dev)
        el = ag.construct_edges_cells(state[:, -1], task["adj_thresh"], mask, tool, task["topk"], task["connect_tools_all"])
        pos, _ = m(state=state, attrs=torch.from_numpy(attrs).to(dev), edges=el, p_instance=torch.ones((1, N_o, 1), device=dev),
                   action=torch.from_numpy(action).to(dev), cloth_physics_param=torch.full((1, 1), 0.5, device=dev))
        err = float(np.abs(pos[0].cpu().numpy() - recs[f]["pred_pos"]).max())
        assert err <= POS_TOL, (f, err)


def test_pile_with_five_tools_vs_oracle(ag, O, dev):
    """4536 grains + the 5-point pusher, top-k 20, two candidates x repeat 2, against O.dynamics (recorded in
    tests/golden/cells_pile_rollout.npz; tests/test_rollout_cells_fixture.py holds the file to the oracle and to the stability
    precondition)."""
    cloud, a = CR.pile_case()
    task = CR.pile_task()
    rec = load_golden("cells_pile_rollout")
    assert np.array_equal(rec["state0"], cloud) and np.array_equal(rec["action"], a)
    m = ag.DynamicsPredictor(*_cfg("granular", 3), dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in O.random_weights(CR.PILE_WEIGHTS_SEED).items()})
    out = ag.dynamics_cells(torch.from_numpy(cloud).to(dev), torch.from_numpy(a), m, dev, _ppm(task, "granular"))
    errs = np.abs(out["state_seqs"].cpu().numpy() - rec["state_seqs"]).reshape(2, -1).max(1)
    print(f"pile: error per candidate {errs}")
    assert errs.max() <= POS_TOL, errs
    assert m.engine(dev).rollout_counts() == (4, 4)


def test_cloth_of_16385_rows(ag, O, dev):
    """No yardstick runs this size.  Three candidates share x, z, theta and have lengths 1.5 / 2.5 / 3.5: the per-step tool delta
    does not depend on the length, so their captures are the states after 1, 2 and 3 forwards of ONE rollout.  The first equals
    DynamicsPredictor.forward over construct_edges_cells' graph of the start state (POS_TOL; no edge decision between the two),
    everything is finite, and the call gives the same bytes twice - and a third time after a call of another shape re-carved the
    workspace."""
    rng = np.random.default_rng(31)
    task = _task("cloth", max_nR=int(1.2 * 6 * 16385) + 64)
    W, m = _model(ag, O, "cloth", 31, dev)
    cloud = _grid(128, 0.3, 0.02, rng)
    N_o, M = cloud.shape[0], 1
    a = np.repeat(_actions(cloud, 1, 1, 1, rng, spread=2.0), 3, 0)
    a[:, 0, 3] = [1.5, 2.5, 3.5]
    s0, ppm = torch.from_numpy(cloud).to(dev), _ppm(task, "cloth")
    first = ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, ppm)["state_seqs"]
    assert first.shape == (3, 1, N_o, 3) and torch.isfinite(first).all()
    assert m.engine(dev).rollout_counts() == (6, 6)
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])
    # the first capture against a plain forward on the start state
    dec, _ = O.decode_action(a[:1], task["push_length"])
    xz, delta = O.tool_keypoints(dec, a[:1, :, 2], task)
    y = np.float32(np.float32(cloud[:, 1].min()) + np.float32(0.01 * task["sim_real_ratio"]))
    frame = np.concatenate([cloud, np.array([[xz[0, 0, 0, 0], y, xz[0, 0, 0, 1]]], np.float32)], 0)
    state = torch.from_numpy(np.repeat(frame[None, None], 4, 1)).to(dev)
    action = np.zeros((1, N_o + M, 3), np.float32)
    action[0, N_o:] = delta[0, 0]
    attrs = np.zeros((1, N_o + M, 2), np.float32)
    attrs[:, :N_o, 0] = 1
    attrs[:, N_o:, 1] = 1
    mask, tool = _masks(N_o, M, dev)
    el = ag.construct_edges_cells(state[:, -1], task["adj_thresh"], mask, tool, task["topk"], True)
    pos, _ = m(state=state, attrs=torch.from_numpy(attrs).to(dev), edges=el, p_instance=torch.ones((1, N_o, 1), device=dev),
               action=torch.from_numpy(action).to(dev), cloth_physics_param=torch.full((1, 1), 0.5, device=dev))
    err = float((first[0, 0] - pos[0]).abs().max())
    print(f"16385 rows: first capture vs plain forward {err:.2e}")
    assert err <= POS_TOL
    again = ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, ppm)["state_seqs"]
    assert torch.equal(again, first)
    small = _cloth(300, rng)
    ag.dynamics_cells(torch.from_numpy(small).to(dev), torch.from_numpy(_actions(small, 7, 1, 2, rng, spread=0.3)), m, dev, ppm)
    third = ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, ppm)["state_seqs"]
    assert torch.equal(third, first)


# ------------------------------------------------------------------------------------------------- overflow and bookkeeping
def test_overflow_is_flagged_and_walked_as_an_empty_graph(ag, O, dev):
    """Cloth with connect_tools_all: a candidate whose tool never comes near has 5 edges per row, one that touches has a tool edge
    into every row on top.  max_nR between the two: the touching candidate overflows.  Ordinary control flow - the guard
    (k_cells_guard) zeroes the count and the row_ptr of such a graph before anything walks it, whether the builder wrote the
    graph (count <= edge_cap) or not."""
    rng = np.random.default_rng(77)
    cloud = _cloth(1023, rng)
    N_o = cloud.shape[0]
    a = _actions(cloud, 2, 1, 2, rng, spread=0.1)
    a[0, 0, 0] += 50.0                                                  # candidate 0: out of reach
    s0 = torch.from_numpy(cloud).to(dev)
    W, m = _model(ag, O, "cloth", 77, dev)
    roomy = _ppm(_task("cloth", max_nR=40000), "cloth")
    free = ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, roomy)["state_seqs"]
    flag = torch.zeros(2, dtype=torch.int32, device=dev)
    ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, roomy, _sync=False, _overflow_flag=flag)
    assert int(flag[0]) == 0
    for max_nR in (5 * N_o + 100, 5900):                                # edge_cap 5376: below the graph, the builder writes nothing; 6144: it writes all of it
        tight = _ppm(_task("cloth", max_nR=max_nR), "cloth")
        with pytest.raises(Exception, match="Exceeds max dims"):
            ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, tight)
        want = torch.zeros(2, dtype=torch.int32, device=dev)
        ag.dynamics(s0, torch.from_numpy(a), m, dev, tight, _sync=False, _overflow_flag=want)
        got = torch.zeros(2, dtype=torch.int32, device=dev)
        out = ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, tight, _sync=False, _overflow_flag=got)["state_seqs"]
        assert int(got[0]) == int(want[0]) > max_nR
        alone = ag.dynamics_cells(s0, torch.from_numpy(a[:1]), m, dev, tight)["state_seqs"]
        assert torch.equal(out[:1], alone) and torch.equal(alone, free[:1])
        assert torch.isfinite(out).all()
    assert torch.equal(ag.dynamics_cells(s0, torch.from_numpy(a), m, dev, roomy)["state_seqs"], free)   # the context is as good as before


def test_refusals_enqueue_nothing(ag, O, dev):
    _, m = _model(ag, O, "cloth", 5, dev)
    eng = m.engine(dev)
    cloud = _cloth(40, np.random.default_rng(1))
    a = torch.from_numpy(_actions(cloud, 2, 1, 2, np.random.default_rng(2)))
    ag.dynamics_cells(torch.from_numpy(cloud).to(dev), a, m, dev, _ppm(_task("cloth"), "cloth"))
    before = (eng.launch_counts(), eng.rollout_counts())
    with pytest.raises(NotImplementedError):
        ag.dynamics_cells(torch.from_numpy(cloud).to(dev), a, m, dev, _ppm(_task("cloth", topk=129), "cloth"))
    with pytest.raises(NotImplementedError):
        ag.dynamics_cells(torch.zeros((1 << 20, 3), device=dev), a, m, dev, _ppm(_task("cloth"), "cloth"))   # + 1 tool: one too many
    assert (eng.launch_counts(), eng.rollout_counts()) == before
