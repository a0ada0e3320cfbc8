"""Zero skip of the exact-fp32 chains (-m gpu).  A k-step of a 160-wide layer whose two input features (f, f + 4 in the
packed K order of csrc/ag_mlp.hip) are exactly zero in all 32 rows of a wavefront adds nothing to the accumulators, so
option zero_skip branches over its MFMAs, and over the weight-fragment reads of a chunk of four such steps.  Every case
runs a rollout with zero_skip = 1 and = 0 and asks for the same state_seqs with torch.equal: on rope and on cloth, with
host-decoded and device-planned actions, with the first forward shared and not.  Shapes are tiny (2 candidates, 64 object
particles + 1 tool, 3 forwards) and the latency-mode chains are switched off, so the 128-row throughput kernels run.
The shipped library has the skip in the propagate chains (k_node_prop); the relation-encoder and particle-encoder chains get it
in experiment builds only (csrc/ag_mlp.hip: AG_ZS_EDGE, AG_ZS_ENC), so the cases cover their layers as well.

The weights are crafted through biases of -10 / +10 (a ReLU unit that is off / on whatever its input):
  fixed     the same units dead in every hidden layer: the pair (1, 5) - a k-step that is skipped; 2 alone - its partner 6
            keeps the step; 16..23 - the four k-steps of chunk 2, whose fragment reads go too; 146 and 147..149 around the
            bias slot 150, which is forced to 1.0 and must keep k-step 74 (146, 150) live: skipping it would drop the bias
  all_dead  every hidden unit dead: the outputs are the bias paths only
  all_live  no unit dead
  keyed     relation-encoder units that are on only where the receiver lies more than c to the right of the sender, with c
            such that ~3 % of the edges qualify: some wavefronts hold such an edge and some do not (checked against the
            oracle's edge list), so the decision is seen to be per wavefront.  (The plain sign of dx is keyed too, but every
            receiver has senders on both sides, so that alone never clears a whole wavefront.)  For the propagate chains, units
            that are on only on tool edges with dx > c_tool are handed through to agg unchanged, so that agg holds them for the
            few receivers to one side of the tool: of candidate 0's two full wavefronts of particle rows one has them, one not
An inf weight must turn the skip off for that model (0 * inf is NaN and has to stay NaN)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import _cfg, _ppm
from test_gpu_more import _task, _grid, _rope, _actions

pytestmark = pytest.mark.gpu

LIMITS = dict(action_lower_lim=[-4.5, -2.5, -3.14, 0.0], action_upper_lim=[0.0, 4.5, 3.14, 7.0])
HIDDEN = ["relation_encoder.model.0", "relation_encoder.model.2", "relation_encoder.model.4",
          "particle_encoder.model.0", "particle_encoder.model.2", "particle_encoder.model.4",
          "relation_propagator.linear", "particle_propagator.linear",
          "non_rigid_predictor.linear_0", "non_rigid_predictor.linear_1"]
DEAD = [1, 5, 2] + list(range(16, 24)) + [146, 147, 148, 149]
DX_CUR = 5 + 9                # rel_inputs: attrs_r (2), attrs_s (2), group (1), pos_r - pos_s (3 residual frames, then the current one)
KEYED_C, KEYED_0 = (8, 12, 9, 13), (16, 20)   # pairs (f, f + 4): on where dx > c / where dx > 0
KEYED_TOOL = (40, 44, 41, 45)                 # pairs: on where the sender is the tool and dx > c_tool; carried through to agg
TOOL_S = 3                                    # rel_inputs: attrs_s[1], 1 for a tool sender


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


def _cloud(material, rng):
    return _rope(64, rng) if material == "rope" else _grid(8, 0.3, 0.02, rng)


def _craft(W, kind, c=0.0, c_tool=0.0):
    W = {k: v.copy() for k, v in W.items()}
    if kind == "fixed":
        for name in HIDDEN:
            W[name + ".bias"][DEAD] = -10.0
    elif kind == "all_dead":
        for name in HIDDEN:
            W[name + ".bias"][:] = -10.0
    elif kind == "all_live":
        for name in HIDDEN:
            W[name + ".bias"][:] = 10.0
    elif kind == "keyed":
        w, b = W["relation_encoder.model.0.weight"], W["relation_encoder.model.0.bias"]
        for units, thr in ((KEYED_C, c), (KEYED_0, 0.0)):
            for f in units:
                w[f, :] = 0.0
                w[f, DX_CUR] = 50.0
                b[f] = -50.0 * thr
        for f in KEYED_TOOL:                                    # 50 (dx - c_tool) on tool edges, < 0 on all others (dx < 1 there)
            w[f, :] = 0.0
            w[f, TOOL_S] = w[f, DX_CUR] = 50.0
            b[f] = -50.0 * (1.0 + c_tool)
            for name in ("relation_encoder.model.2", "relation_encoder.model.4", "relation_propagator.linear"):
                W[name + ".weight"][f, :] = 0.0                 # ... handed on unchanged: agg[f] > 0 iff the receiver has such an edge
                W[name + ".weight"][f, f] = 1.0
                W[name + ".bias"][f] = 0.0
    else:
        assert kind == "random"
    return W


@pytest.fixture(scope="module")
def models(ag, dev):
    """one model per material; the cases load their weights into it"""
    return {mat: ag.DynamicsPredictor(*_cfg(mat, 3), dev) for mat in ("rope", "cloth")}


def _load(m, W):
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()})


def _pair(ag, m, dev, s0, a, ppm, **opts):
    """state_seqs with zero_skip on and off, everything else the same"""
    eng = m.engine(dev)
    out = []
    for zs in (1, 0):
        with eng.options(zero_skip=zs, latency=0, share_prefix=0, **opts):
            out.append(ag.dynamics(s0, a, m, dev, ppm)["state_seqs"])
            if zs:
                assert eng.get_option("zero_skip_active") == 1
    return out


def _setup(material, device_plan, B, seed, reps=3):
    rng = np.random.default_rng(seed)
    task = _task(material, max_nR=40000, **(LIMITS if device_plan else {}))
    cloud = _cloud(material, rng)
    a_np = _actions(cloud, B, 1, np.full(B, reps), rng, spread=0.4)
    return task, cloud, a_np


@pytest.mark.parametrize("kind", ["fixed", "all_dead", "all_live", "random"])
@pytest.mark.parametrize("device_plan", [False, True])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_zero_skip_gives_the_same_bits(ag, O, dev, models, material, device_plan, kind):
    task, cloud, a_np = _setup(material, device_plan, 2, 401)
    m = models[material]
    _load(m, _craft(O.random_weights(401), kind))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    ppm = _ppm(task, material)
    for share_first in (0, 1):                                 # the first forward with its C rows shared, and not
        on, off = _pair(ag, m, dev, s0, a, ppm, share_first=share_first, device_decode=1 if device_plan else 0)
        assert torch.isfinite(off).all() and torch.equal(on, off), (share_first, float((on - off).abs().max()))
    if kind == "all_dead" and material == "rope":
        # bias paths only: every particle moves by the head's bias, three times
        b2 = O.random_weights(401)["non_rigid_predictor.linear_2.bias"]
        want = cloud + 3 * b2[None, :]
        assert np.abs(on[0, 0].cpu().numpy() - want).max() <= 1e-5


@pytest.mark.parametrize("device_plan", [False, True])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_zero_skip_decides_per_wavefront(ag, O, dev, models, material, device_plan):
    task, cloud, a_np = _setup(material, device_plan, 2, 409)
    # the engine's relation-encoder work list: candidate 0's edges of the first forward in the reference's order, self-loops
    # left out, 32 consecutive ones per wavefront
    trace = []
    O.dynamics(O.random_weights(409), 3, cloud, a_np[:1] * np.array([1, 1, 1, 0], np.float32) + np.array([0, 0, 0, 1.5], np.float32),
               _task(material, max_nR=40000), trace=trace)
    rec = trace[0][0]
    ns = rec["recv"] != rec["send"]
    dx = (rec["state_last"][rec["recv"], 0] - rec["state_last"][rec["send"], 0])[ns]
    c = float(np.quantile(dx, 0.97))
    assert c > 0
    groups = [dx[i:i + 32] for i in range(0, len(dx), 32)]
    on_c = [bool((g > c).any()) for g in groups]
    assert any(on_c) and not all(on_c), "the keyed units must be off in some wavefronts and on in others"
    assert all(bool((g > 0).any()) for g in groups[:-1])       # what the plain sign gives: never a whole (full) wavefront
    # the propagate chains: rows candidate * 65 + particle, so candidate 0's particles 0..31 and 32..63 are two wavefronts
    tool = (rec["send"] >= 64) & ns
    dx_all = rec["state_last"][rec["recv"], 0] - rec["state_last"][rec["send"], 0]
    c_tool = float(np.quantile(dx_all[tool], 0.8))
    keyed_recv = rec["recv"][tool & (dx_all > c_tool)]
    assert len(keyed_recv) and bool((keyed_recv < 32).any()) != bool(((keyed_recv >= 32) & (keyed_recv < 64)).any()), keyed_recv
    m = models[material]
    _load(m, _craft(O.random_weights(409), "keyed", c, c_tool))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    on, off = _pair(ag, m, dev, s0, a, _ppm(task, material), share_first=0, device_decode=1 if device_plan else 0)
    assert torch.isfinite(off).all() and torch.equal(on, off)


def test_zero_skip_over_two_launch_chunks_and_a_ragged_tile(ag, O, dev, models):
    """130 candidates in launch chunks of 128: chunks of 128 and 2 candidates, and 2 x 65 rows end in a ragged tile"""
    task, cloud, a_np = _setup("cloth", False, 130, 419)
    m = models["cloth"]
    _load(m, _craft(O.random_weights(419), "fixed"))
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    eng = m.engine(dev)
    eng.set_chunk(128)
    try:
        on, off = _pair(ag, m, dev, s0, a, _ppm(task, "cloth"), streams=1, device_decode=0)
    finally:
        eng.set_chunk(0)
    assert torch.isfinite(off).all() and torch.equal(on, off)
    assert float((on[0] - on[129]).abs().max()) > 0            # the candidates differ: the last chunk computed its own


@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_an_inf_weight_turns_the_skip_off(ag, O, dev, models, material):
    """Column 1 of the relation encoder's second layer multiplies a unit that the "fixed" weights keep at 0.  With inf there,
    unit 3 of that layer is 0 * inf = NaN on every edge - unless the k-step (1, 5) were skipped, which would leave the finite
    rest of the sum, here > 0 (bias + 10).  The guard must see the inf at upload and report the skip as off; outputs then equal
    the option-off run bit for bit, NaNs included.  The chains' ReLU is a max(x, 0), which turns the NaN into 0, so what
    0 * inf = NaN must give is known: the outputs of the same model with unit 3 dead and no inf."""
    task, cloud, a_np = _setup(material, False, 2, 431, reps=1)
    W = _craft(O.random_weights(431), "fixed")
    W["relation_encoder.model.2.weight"][3, 1] = np.inf
    W["relation_encoder.model.2.bias"][3] = 10.0
    W_dead = {k: v.copy() for k, v in W.items()}
    W_dead["relation_encoder.model.2.weight"][3, 1] = 0.0
    W_dead["relation_encoder.model.2.bias"][3] = -10.0
    m = models[material]
    _load(m, W)
    s0, a = torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev)
    eng = m.engine(dev)
    outs = []
    for zs in (1, 0):
        with eng.options(zero_skip=zs, latency=0, share_prefix=0, share_first=0, device_decode=0):
            assert eng.get_option("zero_skip") == zs and eng.get_option("zero_skip_active") == 0
            outs.append(ag.dynamics(s0, a, m, dev, _ppm(task, material))["state_seqs"])
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    _load(m, W_dead)                                            # finite weights again: the guard lets go
    eng = m.engine(dev)
    assert eng.get_option("zero_skip_active") == 1
    with eng.options(zero_skip=0, latency=0, share_prefix=0, share_first=0, device_decode=0):
        want = ag.dynamics(s0, a, m, dev, _ppm(task, material))["state_seqs"]
    assert torch.equal(outs[0], want)
    W_live = {k: v.copy() for k, v in W_dead.items()}           # what a wrongly skipped step would have given differs
    W_live["relation_encoder.model.2.bias"][3] = 10.0
    _load(m, W_live)
    with m.engine(dev).options(zero_skip=0, latency=0, share_prefix=0, share_first=0, device_decode=0):
        assert not torch.equal(want, ag.dynamics(s0, a, m, dev, _ppm(task, material))["state_seqs"])
