"""Chunk list of the relation encoder (-m gpu).  Option edge_order = 2 makes the edge builder write ONE work list per launch over all
its live candidates (csrc/ag_edges.hip: k_chunk_count / k_chunk_scan / k_chunk_fill) - object-object slots by the transposed slot index, the same
slot of every candidate adjacent and in candidate order, then the tool slots by sector and ring of pos_r - pos_s - where edge_order
= 0 writes one list per candidate in slot order.  k_edge_enc stores a C row by slot and a row's chain does not depend on lane,
workgroup or launch, so every output must keep its bits: every case runs the same rollout with edge_order 0 and 2 and asks for
torch.equal on state_seqs, and for equal share_counts(), rollout_counts() and overflow flags.  A dropped entry would leave a stale
C row, so the three forwards of every case catch that as well; the last case reads the list itself back through the diagnostic
build of the library.

Shapes are tiny, as in tests/test_gpu_edge_order.py whose helpers these cases use: an 8 x 8 cloth + 1 tool (65 x 6 = 390 slots, 7
bitmap words, about 320 non-self slots per candidate) or a rope of 64 + 1, 3 forwards, latency-mode chains off so that the 128-row
throughput kernel runs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import _cfg, _ppm, POS_TOL
from test_gpu_more import _task, _rope, _actions
from test_gpu_zero_skip import _craft, LIMITS
from test_gpu_edge_order import _run, _same, _load, _cloud, dev, ag, O, models  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(material, rng, B, reps=3, H=1):
    """B candidates around the object: candidate 0 starts on it and pushes through it (its rows come to hold other senders than its
    neighbours' rows), candidate 1 stays out of reach (no tool edge at all), the others graze it - keys held by some candidates only"""
    cloud = _cloud(material, rng)
    reps = np.full((B, H), reps) if np.isscalar(reps) else np.asarray(reps)
    a = _actions(cloud, B, H, reps, rng, spread=0.2)
    c = cloud.mean(0)
    a[0, :, 0], a[0, :, 1] = c[0] + 0.1, c[2] - 0.1
    if B > 1:
        a[1, :, 0] += 30.0
    return cloud, a


def _both(ag, m, dev, s0, a, ppm, **opts):
    r0 = _run(ag, m, dev, s0, a, ppm, 0, **opts)
    r2 = _run(ag, m, dev, s0, a, ppm, 2, **opts)
    _same(r0, r2)
    return r2


def _setup(O, dev, models, material, seed, B, reps=3, H=1, craft=None, **task_kw):
    rng = np.random.default_rng(seed)
    task = _task(material, **{"max_nR": 40000, **task_kw})
    cloud, a_np = _batch(material, rng, B, reps, H)
    m = models[material]
    W = O.random_weights(seed)
    _load(m, _craft(W, craft) if craft else W)
    return m, torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev), _ppm(task, material), (cloud, a_np, task)


@pytest.mark.parametrize("B", [1, 31, 32, 33, 97, 129])
def test_chunk_list_gives_the_same_bits(ag, O, dev, models, B):
    """1: a list of one candidate; 31 / 32 / 33: a key's entries fill just under, exactly and just over a wavefront; 97: three
    wavefronts and one row; 129 with chunks of 128: a launch of 128 candidates and one of a single candidate.  With and without
    the shared first forward (its slots stay out of the list)."""
    m, s0, a, ppm, (cloud, a_np, task) = _setup(O, dev, models, "cloth", 601, B)
    eng = m.engine(dev)
    if B == 129:
        eng.set_chunk(128)
    try:
        got = [_both(ag, m, dev, s0, a, ppm, share_first=sf, device_decode=0) for sf in (0, 1)]
    finally:
        eng.set_chunk(0)
    assert torch.equal(got[0][0], got[1][0])
    if B > 1:
        assert got[1][1][1] > 0                                 # the shared first forward did share
        assert float((got[0][0][0] - got[0][0][1]).abs().max()) > 0
    if B == 33:                                                 # and the list that was reordered is the reference's
        want = O.dynamics(O.random_weights(601), 3, cloud, a_np[:4], task)["state_seqs"]
        assert np.abs(got[0][0][:4].cpu().numpy() - want).max() <= POS_TOL


@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_chunk_list_with_keys_that_only_some_candidates_hold(ag, O, dev, models, material):
    """five candidates: one without a tool edge, one pushing hard into the object - most tool keys and some object-object slots are
    held by one or two candidates only, so the runs of a key are short and of unequal length"""
    m, s0, a, ppm, _ = _setup(O, dev, models, material, 607, 5)
    a[0, 0, 3] = 3.5
    for share_first in (0, 1):
        _both(ag, m, dev, s0, a, ppm, share_first=share_first, device_decode=0)


def test_chunk_list_while_the_live_prefix_shrinks_on_the_device_plan(ag, O, dev, models):
    """device-planned repeats mixed over 1..4 (and 0), two look-ahead steps: the live prefix of a launch shrinks inside a look-ahead
    step down to 1 candidate, and the launches the host enqueues past a step's own maximum find 0"""
    reps = np.asarray([[4, 1], [3, 2], [2, 1], [1, 2], [1, 0], [2, 2], [3, 1], [1, 1], [2, 0]])
    m, s0, a, ppm, _ = _setup(O, dev, models, "cloth", 613, len(reps), reps, H=2, **LIMITS)
    a[1, :, 0] -= 30.0                                          # (back inside the action limits)
    dp = _both(ag, m, dev, s0, a, ppm, share_first=0, device_decode=1)
    assert dp[2][0] == int(reps.sum())
    hd = _both(ag, m, dev, s0, a, ppm, share_first=0, device_decode=0)   # the host-decoded plan: launches over the live prefix only
    assert torch.equal(dp[0], hd[0])
    _both(ag, m, dev, s0, a, ppm, share_first=1, device_decode=1)


def test_chunk_list_with_the_prefix_shared(ag, O, dev, models):
    m, s0, a, ppm, _ = _setup(O, dev, models, "cloth", 617, 4)
    a[2, 0, 0] += 30.0                                          # two candidates out of reach: one base rollout serves both
    r = _both(ag, m, dev, s0, a, ppm, share_prefix=1, device_decode=0)
    assert r[2][0] < r[2][1]
    assert torch.equal(r[0], _run(ag, m, dev, s0, a, ppm, 2, device_decode=0)[0])


def test_chunk_list_of_a_masked_batch_with_a_phantom_candidate(ag, O, dev, models):
    rng = np.random.default_rng(619)
    task = _task("rope", max_nR=4000)
    m = models["rope"]
    _load(m, O.random_weights(619))
    B, n = 5, 100
    state = np.zeros((B, n, 3), np.float32)
    mask = np.zeros((B, n), bool)
    for b in range(B):
        state[b] = _rope(n, rng)
        mask[b] = rng.uniform(size=n) > (0.0, 0.2, 0.35, 0.1, 0.5)[b]
        state[b, ~mask[b]] = 0
    a = _actions(state[0], B, 1, [3, 2, 4, 1, 3], rng)[:, 0]
    args = (torch.from_numpy(state).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(a).to(dev))
    call = lambda: ag.dynamics_masked(*args, m, dev, _ppm(task, "rope"))["state_seqs"]  # noqa: E731
    for ragged in (1, 0):
        _same(_run(ag, m, dev, None, None, None, 0, call=call, ragged=ragged), _run(ag, m, dev, None, None, None, 2, call=call, ragged=ragged))


def test_chunk_list_leaves_out_a_candidate_over_max_nR(ag, O, dev, models):
    """a graph above max_nR is presented as empty downstream and reported: it contributes no entry; same outputs, same flag"""
    m, s0, a, _, _ = _setup(O, dev, models, "cloth", 631, 4)
    big = _both(ag, m, dev, s0, a, _ppm(_task("cloth", max_nR=40000), "cloth"), share_first=0, device_decode=0)
    assert big[3][0] == 0
    small = _ppm(_task("cloth", max_nR=350), "cloth")
    r0 = _run(ag, m, dev, s0, a, small, 0, share_first=0, device_decode=0)
    r2 = _run(ag, m, dev, s0, a, small, 2, share_first=0, device_decode=0)
    _same(r0, r2, finite=False)
    assert r2[3][0] > 350                                       # a pushed candidate's graph is over, the untouched one's is not
    assert not torch.equal(r2[0].view(torch.int32), big[0].view(torch.int32))


def test_chunk_list_does_not_depend_on_the_lds_budget_of_the_class_bitmaps(ag, O, dev, models):
    """ell_lds_words walks k_ell_index's class bitmaps 25 -> 2 -> 1 under order 1; the chunk list keeps no bitmap in LDS"""
    m, s0, a, ppm, _ = _setup(O, dev, models, "cloth", 641, 5, craft="fixed")
    ref = _run(ag, m, dev, s0, a, ppm, 0, device_decode=0)
    for words in (174, 13, 1):
        for order in (1, 2):
            r = _run(ag, m, dev, s0, a, ppm, order, ell_lds_words=words, device_decode=0)
            assert torch.equal(r[0], ref[0]) and r[2:] == ref[2:], (words, order)


def test_chunk_list_on_one_stream_and_on_four(ag, O, dev, models):
    m, s0, a, ppm, _ = _setup(O, dev, models, "cloth", 643, 9)
    eng = m.engine(dev)
    whole = _run(ag, m, dev, s0, a, ppm, 0, device_decode=0)
    eng.set_chunk(2)                                            # five launches per forward: chunks of 2, 2, 2, 2, 1
    try:
        one = _both(ag, m, dev, s0, a, ppm, streams=1, device_decode=0)
        four = _both(ag, m, dev, s0, a, ppm, streams=4, stream_min_rows=0, device_decode=0)
    finally:
        eng.set_chunk(0)
    assert torch.equal(one[0], whole[0]) and torch.equal(four[0], whole[0])


@pytest.mark.parametrize("kind", ["fixed", "all_dead", "all_live"])
@pytest.mark.parametrize("material", ["rope", "cloth"])
def test_skips_on_the_chunk_list_give_the_same_bits(ag, O, dev, models, material, kind):
    """the crafted weights of tests/test_gpu_zero_skip.py: zero_skip and half_step 0 against 1 under order 2, and against order 0"""
    m, s0, a, ppm, _ = _setup(O, dev, models, material, 647, 33, craft=kind)
    for share_first in (0, 1):
        off = _run(ag, m, dev, s0, a, ppm, 0, zero_skip=0, half_step=0, share_first=share_first, device_decode=0)
        for zs, hs in ((1, 1), (1, 0), (0, 0)):
            _same(_run(ag, m, dev, s0, a, ppm, 2, zero_skip=zs, half_step=hs, share_first=share_first, device_decode=0), off)


def test_chunk_list_with_five_history_frames(ag, dev):
    """n_his = 5: k_edge_enc<5> reads the chunk list too (the softbody golden's model and batch)"""
    from helpers import load_golden, task_of
    g = load_golden("dyn_softbody_nhis5")
    task = task_of(g)
    mc, mat, ds = _cfg("softbody", 4)
    m = ag.DynamicsPredictor(mc, mat, dict(ds, n_his=5), dev)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("w::")})
    s0, a = torch.from_numpy(g["state0"]).to(dev), torch.from_numpy(g["action"]).to(dev)
    r = _both(ag, m, dev, s0, a, _ppm(task, "softbody"), device_decode=0)
    assert np.abs(r[0].cpu().numpy() - g["state_seqs"]).max() <= POS_TOL


def test_other_chains_keep_their_own_list_under_order_2(ag, O, dev, models):
    """bf16x3 and the latency-mode chains do not read a chunk list: under edge_order = 2 their launches take order 1"""
    m, s0, a, ppm, _ = _setup(O, dev, models, "cloth", 653, 5)
    m.set_precision("bf16x3")
    try:
        _both(ag, m, dev, s0, a, ppm, device_decode=0)
    finally:
        m.set_precision("fp32")
    _both(ag, m, dev, s0, a[:1], ppm, latency=1, device_decode=0)


_DUMP_CHILD = r'''
import importlib.util, os, sys
import numpy as np, torch
root = sys.argv[1]
sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, root)
import adaptigraph_amd as ag
from adaptigraph_amd import _lib
from oracle import adaptigraph_oracle as O
from test_gpu_parity import _ppm
from test_gpu_more import _task, _model
from test_gpu_chunk_order import _batch
assert _lib.LIB_PATH.endswith("_diag.so")
spec = importlib.util.spec_from_file_location("chunk_order_census", os.path.join(root, "tools", "chunk_order_census.py"))
C = importlib.util.module_from_spec(spec); spec.loader.exec_module(C)
dev = torch.device("cuda:0")
rng = np.random.default_rng(659)
task = _task("cloth", max_nR=40000)
cloud, a_np = _batch("cloth", rng, 37, reps=[3] * 30 + [1] * 7)      # the dumped third forward has 30 live candidates of 37
_, m = _model(ag, O, "cloth", 659, dev)
eng = m.engine(dev)
with eng.options(latency=0, share_prefix=0, share_first=0, edge_order=2, device_decode=0, streams=1):
    ag.dynamics(torch.from_numpy(cloud).to(dev), torch.from_numpy(a_np).to(dev), m, dev, _ppm(task, "cloth"))
torch.cuda.synchronize()
raw = np.fromfile(sys.argv[2], np.int32)
B, N, stride, cap, shift, n, n_oo, n_tools = (int(v) for v in raw[:8])
assert (B, N, stride) == (30, 65, 6) and 0 < n_oo < n, (B, N, stride, n, n_oo)
o = 8
lst = raw[o:o + n].view(np.uint32); o += n
deg = raw[o:o + B * N].reshape(B, N); o += B * N
send = raw[o:o + B * cap].reshape(B, cap)[:, :N * stride].reshape(B, N, stride); o += B * cap
pos = raw[o:o + B * N * 3].view(np.float32).reshape(B, N, 3); o += B * N * 3
thr = float(raw[o:o + 1].view(np.float32)[0])
cand, slot = (lst >> shift).astype(np.int64), (lst & ((1 << shift) - 1)).astype(np.int64)
# the non-self slots of the live candidates, from the graph itself
recv = np.broadcast_to(np.arange(N)[None, :, None], (B, N, stride))
t = np.broadcast_to(np.arange(stride)[None, None, :], (B, N, stride))
want = (t < deg[:, :, None]) & (send != recv)
assert n == int(want.sum()) and cand.max() < B and slot.max() < N * stride
got = np.zeros((B, N * stride), np.int64)
np.add.at(got, (cand, slot), 1)
assert np.array_equal(got.reshape(B, N, stride), want.astype(np.int64)), "not a permutation of the live candidates' non-self slots"
i, tt = slot // stride, slot % stride
j = send[cand, i, tt]
tool = (i >= N - n_tools) | (j >= N - n_tools)
assert not tool[:n_oo].any() and tool[n_oo:].all()             # every tool entry lies behind the object-object ones
key = C.chunk_keys(tt * N + i, tool, pos[cand, i] - pos[cand, j], np.float32(thr) * np.float32(thr), N * stride)
assert (np.diff(key) >= 0).all()                               # keys ascend, the numpy restatement's
oo = slice(0, n_oo)
same = np.diff(key[oo]) == 0
assert (np.diff(cand[oo])[same] > 0).all()                     # inside an object-object key: candidate order
assert len(np.unique(key[n_oo:])) > 8 and (key[n_oo:] >= N * stride).all()
print("CHILD_OK", n, n_oo)
'''


def test_the_chunk_list_itself(dev, tmp_path):
    """The list of one launch, read back through the diagnostic build of the library (-DAG_DIAG, AG_CHUNK_DUMP: the product library
    has no such hook) in a child process: a permutation of the non-self slots of the launch's live candidates (seven of its 37 have no
    forward left), object-object keys ascending with a key's entries in candidate order, every tool entry behind them and the tool
    keys ascending as tools/chunk_order_census.py restates them."""
    diag = os.path.join(ROOT, "adaptigraph_amd", "csrc", "libadaptigraph_hip_diag.so")
    assert os.path.exists(diag), "build the diagnostic library: adaptigraph_amd/csrc/build.sh diag"
    out = str(tmp_path / "chunk_list.bin")
    env = dict(os.environ, ADAPTIGRAPH_AMD_LIB=diag, AG_CHUNK_DUMP=out, AG_CHUNK_DUMP_AT="2")
    r = subprocess.run([sys.executable, "-c", _DUMP_CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
