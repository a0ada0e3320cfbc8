"""Half-steps of the exact-fp32 chains (-m gpu).  A k-step of a 160-wide layer carries two input features, f on lanes 0-31 and
f + 4 on lanes 32-63 (the packed K order of csrc/ag_mlp.hip).  Where exactly one of them is zero in all 32 rows of a wavefront,
option half_step issues 3 MFMAs instead of 5: two two-block v_mfma_f32_32x32x1_2b_f32 over the live feature, one ordinary MFMA.
It rides on zero_skip (no effect where zero_skip_active is 0).  Every case compares state_seqs of three runs with torch.equal -
half_step = 1, half_step = 0, zero_skip = 0 - host-decoded and device-planned, with the first forward shared and not, with the
class-major work list and the slot-order one (the relation-encoder chain skips in every tile of either; its wavefronts hold like
edges only in the first).  Shapes and
helpers are those of tests/test_gpu_zero_skip.py: 2 candidates, 64 object particles + 1 tool, 3 forwards, throughput kernels.

Crafted through biases of -10 / +10 (a ReLU unit that is off / on whatever its input):
  one_sided  dead in every hidden layer: 2 alone (partner 6 live: a step with only lanes 32-63 live), 7 alone (partner 3: only lanes
             0-31), 66 and 71, 130 and 135 (the same in input tiles 2 and 4), 146 - its partner 150 is the bias slot, forced to 1.0:
             the half-step must keep the bias
  keyed      unit 8 of the relation encoder's first layer is on only where dx > c (the 97 % quantile), its partner 12 always: the
             step is full in the wavefronts that hold such an edge and half in the others
  all_dead / all_live / random  as in tests/test_gpu_zero_skip.py.  Step (147, 151) pairs a real unit with the K padding slot, so
             even an all-live model takes a half-step there in every wavefront
An inf weight that multiplies a dead unit whose partner is live must turn everything off (0 * inf has to stay NaN)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import _ppm
from test_gpu_more import _task
from test_gpu_zero_skip import _craft, _load, _setup, HIDDEN, DX_CUR, dev, ag, O, models  # noqa: F401  (fixtures)
from test_gpu_edge_order import _census

pytestmark = pytest.mark.gpu

ONE_SIDED = [2, 7, 66, 71, 130, 135, 146]
COMBOS = [(sf, eo) for sf in (0, 1) for eo in (1, 0)]          # share_first x edge_order


def _one_sided(W):
    W = {k: v.copy() for k, v in W.items()}
    for name in HIDDEN:
        W[name + ".bias"][ONE_SIDED] = -10.0
    return W


def _three(ag, m, dev, s0, a, ppm, active=1, **opts):
    """state_seqs with half-steps, with the skip alone, with neither; everything else the same"""
    eng = m.engine(dev)
    out = []
    for zs, hs in ((1, 1), (1, 0), (0, 1)):
        with eng.options(zero_skip=zs, half_step=hs, latency=0, share_prefix=0, **opts):
            assert eng.get_option("half_step") == hs
            if zs:
                assert eng.get_option("zero_skip_active") == active
            out.append(ag.dynamics(s0, a, m, dev, ppm)["state_seqs"])
    return out


def _check(ag, m, dev, s0, a, ppm, device_plan, **opts):
    res = None
    for share_first, edge_order in COMBOS:
        hs, zs, off = _three(ag, m, dev, s0, a, ppm, share_first=share_first, edge_order=edge_order,
                             device_decode=1 if device_plan else 0, **opts)
        assert torch.isfinite(off).all(), (share_first, edge_order)
        assert torch.equal(hs, off) and torch.equal(zs, off), (share_first, edge_order, float((hs - off).abs().max()))
        res = hs
    return res


@pytest.mark.parametrize("kind", ["one_sided", "all_dead", "all_live", "random"])
@pytest.mark.parametrize("device_plan", [False, True])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_half_step_gives_the_same_bits(ag, O, dev, models, material, device_plan, kind):
    task, cloud, a_np = _setup(material, device_plan, 2, 601)
    m = models[material]
    W = O.random_weights(601)
    _load(m, _one_sided(W) if kind == "one_sided" else _craft(W, kind))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    _check(ag, m, dev, s0, a, _ppm(task, material), device_plan)


@pytest.mark.parametrize("layer", ["relation_encoder.model.2", "non_rigid_predictor.linear_1"])
def test_the_ever_present_half_step_computes(ag, O, dev, models, layer):
    """Unit 147 shares its k-step with the padding slot 151: a half-step in every wavefront, also of an all-live model.  The weights
    that multiply it must reach the result - in the relation-encoder chain and in the propagate chain."""
    task, cloud, a_np = _setup("cloth", False, 2, 607)
    m = models["cloth"]
    W = _craft(O.random_weights(607), "all_live")
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    outs = []
    for delta in (0.0, 0.5):
        W2 = {k: v.copy() for k, v in W.items()}
        W2[layer + ".weight"][:, 147] += delta
        _load(m, W2)
        eng = m.engine(dev)
        with eng.options(zero_skip=1, half_step=1, latency=0, share_prefix=0, share_first=0, edge_order=1, device_decode=0):
            assert eng.get_option("zero_skip_active") == 1
            outs.append(ag.dynamics(s0, a, m, dev, _ppm(task, "cloth"))["state_seqs"])
    assert torch.isfinite(outs[0]).all() and torch.isfinite(outs[1]).all()
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("device_plan", [False, True])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_half_step_decides_per_wavefront(ag, O, dev, models, material, device_plan):
    C = _census()
    task, cloud, a_np = _setup(material, device_plan, 2, 613)
    trace = []
    O.dynamics(O.random_weights(613), 3, cloud, a_np[:1] * np.array([1, 1, 1, 0], np.float32) + np.array([0, 0, 0, 1.5], np.float32),
               _task(material, max_nR=40000), trace=trace)
    rec = trace[0][0]
    ns = np.flatnonzero(rec["recv"] != rec["send"])
    recv, send, pos = rec["recv"][ns], rec["send"][ns], rec["state_last"]
    dx = pos[recv, 0] - pos[send, 0]
    c = float(np.quantile(dx, 0.97))
    assert c > 0
    # candidate 0's work list of the first forward in class-major order: the wavefronts wholly among the object-object classes
    perm, n_oo = C.work_list_order(recv, send, pos, 64, "class")
    d = dx[perm]
    on = [bool((d[i:i + 32] > c).any()) for i in range(0, n_oo - n_oo % 32, 32)]
    assert any(on) and not all(on), "step (8, 12) must be full in some wavefronts and half in others"
    W = O.random_weights(613)
    w, b = W["relation_encoder.model.0.weight"], W["relation_encoder.model.0.bias"]
    w[8, :] = 0.0
    w[8, DX_CUR] = 50.0
    b[8] = -50.0 * c
    b[12] = 10.0
    m = models[material]
    _load(m, W)
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    _check(ag, m, dev, s0, a, _ppm(task, material), device_plan)


@pytest.mark.parametrize("device_plan", [False, True])
def test_half_step_over_two_launch_chunks_and_a_ragged_tile(ag, O, dev, models, device_plan):
    """130 candidates in launch chunks of 128 on one stream: chunks of 128 and 2 candidates, and 2 x 65 rows end in a ragged tile"""
    task, cloud, a_np = _setup("cloth", device_plan, 130, 617)
    m = models["cloth"]
    _load(m, _one_sided(O.random_weights(617)))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    eng = m.engine(dev)
    eng.set_chunk(128)
    try:
        on = _check(ag, m, dev, s0, a, _ppm(task, "cloth"), device_plan, streams=1)
    finally:
        eng.set_chunk(0)
    assert float((on[0] - on[129]).abs().max()) > 0            # the candidates differ: the last chunk computed its own


@pytest.mark.parametrize("device_plan", [False, True])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_an_inf_weight_turns_the_half_step_off(ag, O, dev, models, material, device_plan):
    """Column 2 of the relation encoder's second layer multiplies unit 2, which the one-sided weights keep at 0 while its partner 6
    is live.  With inf there, 0 * inf = NaN on every edge - unless the half-step left lanes 0-31 of step (2, 6) out."""
    task, cloud, a_np = _setup(material, device_plan, 2, 619, reps=1)
    W_ok = _one_sided(O.random_weights(619))
    W = {k: v.copy() for k, v in W_ok.items()}
    W["relation_encoder.model.2.weight"][3, 2] = np.inf
    W["relation_encoder.model.2.bias"][3] = 10.0
    m = models[material]
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, material)
    for share_first, edge_order in COMBOS:
        _load(m, W)
        hs, zs, off = _three(ag, m, dev, s0, a, ppm, active=0, share_first=share_first, edge_order=edge_order,
                             device_decode=1 if device_plan else 0)
        assert torch.equal(hs.view(torch.int32), off.view(torch.int32)) and torch.equal(zs.view(torch.int32), off.view(torch.int32))
        _load(m, W_ok)                                         # finite weights again: the guard lets go
        eng = m.engine(dev)
        assert eng.get_option("zero_skip_active") == 1 and eng.get_option("half_step") == 1
        hs, zs, off = _three(ag, m, dev, s0, a, ppm, share_first=share_first, edge_order=edge_order,
                             device_decode=1 if device_plan else 0)
        assert torch.isfinite(off).all() and torch.equal(hs, off) and torch.equal(zs, off)
