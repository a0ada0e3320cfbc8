"""The paired weight image of the half-step chains (-m gpu).  The layers that k_edge_enc and k_node_prop read (relation encoder
layers 2 and 3, W1, Wb, W2, W3, the predictor's first two layers) are packed for the two-block MFMA: m-blocks 2m and 2m + 1 of the
fp32 image hold [W(tile 2m, f) | W(tile 2m+1, f)] and [W(tile 2m, f+4) | W(tile 2m+1, f+4)] on the lane halves (csrc/ag_optim.hip,
pack_elem_f32), where they used to hold [W(tile, f) | W(tile, f+4)] per tile and every live k-step swapped them into place.  A
fragment that lands in the wrong tile, lane half or k slot gives finite, plausible, wrong numbers, and every on/off comparison of
the other test files would still agree with itself, so the yardstick here is the SECOND image: the latency-mode chains
(latency = 1, csrc/ag_lat.hip) read their own, untouched 16 x 16 image, and both families round identically.  Shapes and helpers
are those of tests/test_gpu_zero_skip.py: 2 candidates, 64 object particles + 1 tool, 3 forwards.

  1  throughput chains (latency = 0) == latency chains (latency = 1), rope and cloth, host-decoded and device-planned, with random
     weights (every weight distinct) and the one-sided weights of tests/test_gpu_half_step.py (steps with one live half)
  2  k_node_enc reads W2 / W3 - paired, because the propagate chains read them - in the two-block form on every step: one
     model(**graph) forward, throughput == latency, and a weight of W2's column 147 reaches the output
  3  the host packer (load_state_dict) and the device packer (ag_ctx_load_weights_device) write the same image
  4  one weight of relation-encoder layer 2 at a time, in every output tile and both lane halves and on both k slots of a step:
     each changes the result, and the result is again that of the latency chains"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_parity import _cfg, _ppm
from test_gpu_zero_skip import _load, _setup, dev, ag, O, models  # noqa: F401  (fixtures)
from test_gpu_half_step import _one_sided

pytestmark = pytest.mark.gpu

ROWS = [3, 35, 67, 99, 131, 149]                               # one output unit per tile 0..4 (tile 4: the unpaired m-block), and its last
COLS = [2, 6]                                                  # the two features of k-step 2: lanes 0-31 and lanes 32-63


def _run(ag, m, dev, s0, a, ppm, latency, device_plan=False, **opts):
    """state_seqs of one rollout on the throughput (latency = 0) or the latency-mode (1) chains"""
    eng = m.engine(dev)
    with eng.options(latency=latency, share_prefix=0, share_first=0, device_decode=1 if device_plan else 0, **opts):
        out = ag.dynamics(s0, a, m, dev, ppm)["state_seqs"]
    assert torch.isfinite(out).all()
    return out


@pytest.mark.parametrize("kind", ["random", "one_sided"])
@pytest.mark.parametrize("device_plan", [False, True])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_throughput_chains_equal_latency_chains(ag, O, dev, models, material, device_plan, kind):
    task, cloud, a_np = _setup(material, device_plan, 2, 701)
    m = models[material]
    W = O.random_weights(701)
    _load(m, _one_sided(W) if kind == "one_sided" else W)
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, material)
    thr = _run(ag, m, dev, s0, a, ppm, 0, device_plan)
    lat = _run(ag, m, dev, s0, a, ppm, 1, device_plan)
    assert torch.equal(thr, lat), float((thr - lat).abs().max())


def _graph(ag, dev, cloud, B):
    """the small cloud with one tool particle above its middle, as the arguments of model(**graph)"""
    N_o = cloud.shape[0]
    rng = np.random.default_rng(709)
    state = np.zeros((B, 4, N_o + 1, 3), np.float32)
    action = np.zeros((B, N_o + 1, 3), np.float32)
    for b in range(B):
        tool = cloud.mean(0) + np.float32([0.1 * b, 0.1, 0.05])
        for h in range(4):
            state[b, h] = np.concatenate([cloud + rng.normal(0, 0.01, cloud.shape), tool[None] - 0.02 * (3 - h)], 0)
        action[b, N_o:] = np.float32([0.02, 0.0, 0.01])
    attrs = np.zeros((B, N_o + 1, 2), np.float32)
    attrs[:, :N_o, 0] = attrs[:, N_o:, 1] = 1
    mask = torch.ones((B, N_o + 1), dtype=torch.bool, device=dev)
    toolm = torch.zeros((B, N_o + 1), dtype=torch.bool, device=dev)
    toolm[:, N_o:] = True
    st = torch.from_numpy(state).to(dev)
    el = ag.construct_edges_index(st[:, -1], 0.75, mask, toolm, 5, True)
    return dict(state=st, attrs=torch.from_numpy(attrs).to(dev), edges=el, p_instance=torch.ones((B, N_o, 1), device=dev),
                action=torch.from_numpy(action).to(dev), cloth_physics_param=torch.full((B, 1), 0.5, device=dev))


def test_node_encoder_reads_the_paired_blocks(ag, O, dev, models):
    """model(**graph) encodes every particle row with k_node_enc (the rollout takes them from a class table made by the latency
    chain): 130 rows, two workgroups, the second ragged.  Unit 147 of the particle encoding is kept on by its bias, so that
    W2[:, 147] multiplies something."""
    _, cloud, _ = _setup("cloth", False, 2, 719)
    m = models["cloth"]
    W = O.random_weights(719)
    W["particle_encoder.model.4.bias"][147] = 10.0
    g = _graph(ag, dev, cloud, 2)
    outs = []
    for delta in (0.0, 0.5):
        W2 = {k: v.copy() for k, v in W.items()}
        W2["relation_propagator.linear.weight"][:, 150 + 147] += delta        # W_rp = [W1 | W2 | W3]: column 147 of W2
        _load(m, W2)
        eng = m.engine(dev)
        with eng.options(latency=0):
            thr = m(**g)
        with eng.options(latency=1):
            lat = m(**g)
        assert torch.isfinite(thr[0]).all()
        assert torch.equal(thr[0], lat[0]) and torch.equal(thr[1], lat[1]), float((thr[1] - lat[1]).abs().max())
        outs.append(thr[1])
    assert not torch.equal(outs[0], outs[1])


def test_host_packer_equals_device_packer(ag, O, dev):
    """The same 22 tensors through load_state_dict (packed on the host) and through ag_ctx_load_weights_device (packed by
    k_pack_weights) into the same engine; zero_skip = 0, so that every fragment of every chunk is read."""
    from adaptigraph_amd.context import current_stream
    task, cloud, a_np = _setup("cloth", False, 2, 727)
    m = ag.DynamicsPredictor(*_cfg("cloth", 3), dev)
    W = O.random_weights(727)
    _load(m, W)
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, "cloth")
    host = _run(ag, m, dev, s0, a, ppm, 0, zero_skip=0)
    eng = m.engine(dev)
    outs = []
    for delta in (0.0, 0.01):                                  # 0.01: the image read afterwards is the one the device packed
        wd = [p.detach().to(dev, torch.float32).contiguous().clone() for p in m.ordered_parameters()]
        assert len(wd) == 22
        wd[21] += delta                                        # the head's bias: every particle's motion
        arr = (C.c_void_p * 22)(*[w.data_ptr() for w in wd])
        eng.check(eng.lib.ag_ctx_load_weights_device(eng.ctx, current_stream(dev), arr))
        outs.append(_run(ag, m, dev, s0, a, ppm, 0, zero_skip=0))
    assert torch.equal(host, outs[0]), float((host - outs[0]).abs().max())
    assert not torch.equal(host, outs[1])


@pytest.fixture(scope="module")
def coverage_case(ag, O, dev, models):
    """weights, inputs and the unperturbed result of the tile-coverage cases: the two input units and the six output units are kept
    on by their biases, so that each perturbed weight multiplies a non-zero and its unit is seen downstream"""
    task, cloud, a_np = _setup("cloth", False, 2, 733)
    W = O.random_weights(733)
    W["relation_encoder.model.0.bias"][COLS] = 10.0
    W["relation_encoder.model.2.bias"][ROWS] = 10.0
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, "cloth")
    m = models["cloth"]
    _load(m, W)
    return W, s0, a, ppm, _run(ag, m, dev, s0, a, ppm, 0)


@pytest.mark.parametrize("row", ROWS)
def test_every_tile_and_lane_half_reaches_the_result(ag, dev, models, coverage_case, row):
    W, s0, a, ppm, base = coverage_case
    m = models["cloth"]
    for col in COLS:
        W2 = {k: v.copy() for k, v in W.items()}
        W2["relation_encoder.model.2.weight"][row, col] += 0.5
        _load(m, W2)
        thr = _run(ag, m, dev, s0, a, ppm, 0)
        lat = _run(ag, m, dev, s0, a, ppm, 1)
        assert not torch.equal(thr, base), (row, col)
        assert torch.equal(thr, lat), (row, col, float((thr - lat).abs().max()))
