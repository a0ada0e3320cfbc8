"""The numpy restatement of the chunk-list key (tools/chunk_order_census.py; csrc/ag_edges.hip: chunk_tool_key, k_chunk_count /
k_chunk_scan / k_chunk_fill) on hand-made positions, the list it builds, and a tiny synthetic case in which the chunk order must
beat the candidate order.  CPU only; the oracle rollout is not run."""
import importlib.util
import os

import numpy as np

from test_edge_order_census import _graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _tool():
    spec = importlib.util.spec_from_file_location("chunk_order_census", os.path.join(ROOT, "tools", "chunk_order_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


THR2 = F32(0.25)                                               # thr = 0.5: the ring edges are |d| = 0.5, 1.0, ... 7.5, exact in fp32


def _key(C, *d):
    return int(C.tool_keys(np.asarray([d], F32), THR2)[0])


def test_tool_key_sign_bits_swap_bit_and_rings():
    C = _tool()
    # |d|^2 = 1 = 2^2 thr^2 exactly: a ring edge belongs to the outer ring (>=)
    assert _key(C, 1, 0, 0) == 0 * 16 + 2                      # no sign bit, |d.z| <= |d.x|, min = 0: sector 0
    assert _key(C, -1, 0, 0) == (1 * 4) * 16 + 2               # d.x < 0
    assert _key(C, 0, 0, 1) == (4 * 4) * 16 + 2                # |d.z| > |d.x|
    assert _key(C, 0, 0, -1) == ((2 + 4) * 4) * 16 + 2         # d.z < 0 as well
    assert _key(C, -1, 0, -0.0) == (1 * 4) * 16 + 2            # -0.0 < 0 is false
    # rings: below, on and above an edge; the last ring is open
    below = np.nextafter(F32(1), F32(0))
    assert _key(C, below, 0, 0) == 1 and _key(C, 1, 0, 0) == 2 and _key(C, np.nextafter(F32(1), F32(2)), 0, 0) == 2
    assert _key(C, 0.25, 0, 0) == 0 and _key(C, 0.5, 0, 0) == 1
    assert [_key(C, 0.5 * k, 0, 0) for k in range(1, 16)] == list(range(1, 16))
    assert _key(C, 7.5, 0, 0) == 15 and _key(C, 1e6, 0, 0) == 15 and _key(C, np.inf, 0, 0) == 15
    # d.y counts in |d| and nowhere else; with d.x = d.z = 0 all three sector tests hold (0 >= t * 0)
    assert _key(C, 0, 2, 0) == 3 * 16 + 4
    assert _key(C, 1, 100, 0) // 16 == 0 and _key(C, 1, 100, 0) % 16 == 15


def test_tool_key_sector_edges_and_ties():
    C = _tool()
    # a tie |d.z| == |d.x| does not swap, and min = max passes all three tangent tests
    assert _key(C, 1, 0, 1) == 3 * 16 + 2                      # |d|^2 = 2: rings 0.25 and 1.0 passed, 2.25 not
    assert _key(C, -1, 0, 1) == (1 * 4 + 3) * 16 + 2
    # every tangent edge: on the edge is the higher sector (>=), one ulp below is the lower one
    for n, t in enumerate(C.TAN):
        assert _key(C, 1, 0, t) // 16 == n + 1, n
        assert _key(C, 1, 0, np.nextafter(t, F32(0))) // 16 == n, n
        assert _key(C, t, 0, 1) // 16 == 16 + n + 1, n         # mirrored about the diagonal: the swap bit
        assert _key(C, np.nextafter(t, F32(0)), 0, -1) // 16 == (2 + 4) * 4 + n, n
    # the 32 sector midpoints are 32 sectors, and inside an octant the sector follows the angle from the nearer axis
    ang = (np.arange(32) + 0.5) * (2 * np.pi / 32)
    d = np.stack([np.cos(ang), np.zeros(32), np.sin(ang)], 1).astype(F32) * F32(3.1)
    key = C.tool_keys(d, THR2)
    assert len(np.unique(key // 16)) == 32 and (key % 16 == 6).all()          # |d| = 3.1 = 6.2 thr
    assert list(key[:4] // 16) == [0, 1, 2, 3] and list(key[4:8] // 16) == [19, 18, 17, 16]
    # coarser keys are the same key with bits dropped
    assert np.array_equal(C.tool_keys(d, THR2, 8, 16) // 16, key // 16 // 4)
    assert np.array_equal(C.tool_keys(d, THR2, 32, 4) % 4, key % 16 // 4)


def test_a_nan_compares_false_and_lands_in_a_defined_bin():
    C = _tool()
    nan = np.nan
    assert _key(C, nan, nan, nan) == 0
    assert _key(C, nan, 0, 1) == 0                             # 1 > NaN is false: no swap; min >= t * NaN is false; NaN >= ring is false
    assert _key(C, 1, nan, 0) == 0 * 16 + 0                    # the sector needs no d.y, the ring does
    assert _key(C, -1, 0, nan) == (1 * 4) * 16 + 0             # NaN > 1 is false: no swap, min = NaN fails the tangent tests


def test_keys_of_a_graph_with_the_tool_as_sender_and_as_receiver():
    C = _tool()
    pos, recv, send = _graph()                                 # 5 x 5 grid, particle 25 the tool, edges receiver-major
    n_obj, N = 25, 26
    r, t = C.slots_of(recv, N)
    assert np.array_equal(r, recv) and t[0] == 0 and (t[recv == 3] == np.arange((recv == 3).sum())).all()
    stride = int(np.bincount(recv).max())
    tool = (recv >= n_obj) | (send >= n_obj)
    as_send, as_recv = send >= n_obj, recv >= n_obj
    assert as_send.any() and as_recv.any()
    d = pos[recv] - pos[send]
    key = C.chunk_keys(t * N + r, tool, d, THR2, N * stride)
    assert np.array_equal(key[~tool], (t * N + r)[~tool]) and (key[~tool] < N * stride).all()
    assert (key[tool] >= N * stride).all() and (key[tool] < N * stride + C.TOOL_SECTORS * C.TOOL_BINS).all()
    # the pair (i, tool) and (tool, i) has d and -d: the same ring, mirrored sign bits where the component is not zero
    for e in np.flatnonzero(as_send):
        back = int(np.flatnonzero((recv == send[e]) & (send == recv[e]))[0])
        k0, k1 = key[e] - N * stride, key[back] - N * stride
        assert k0 % 16 == k1 % 16
        s0, s1 = k0 // 16, k1 // 16
        assert s0 % 4 == s1 % 4 and s0 // 16 == s1 // 16       # tangent count and swap bit
        for bit, col in ((1, 0), (2, 2)):
            if d[e, col] != 0:
                assert (s0 // 4 & bit) != (s1 // 4 & bit)


def _random_chunk(C, rng, B, n_slots, n_tool_slots):
    per = []
    for b in range(B):
        slot = np.sort(rng.choice(n_slots, size=int(rng.integers(0, n_slots)), replace=False))
        tool = np.isin(slot, np.arange(n_tool_slots))
        d = rng.normal(0, 2, (len(slot), 3)).astype(F32)
        per.append((slot, tool, d))
    return per


def test_the_list_is_a_permutation_of_the_candidates_non_self_slots():
    C = _tool()
    rng = np.random.default_rng(11)
    n_slots = 90
    per = _random_chunk(C, rng, 7, n_slots, 20)
    per[3] = (np.zeros(0, np.int64), np.zeros(0, bool), np.zeros((0, 3), F32))      # a candidate that contributes nothing
    cand, idx, key, n_oo = C.chunk_list(per, THR2, n_slots)
    want = sorted((b, int(s)) for b, (slot, _, _) in enumerate(per) for s in slot)
    got = sorted((int(b), int(per[b][0][i])) for b, i in zip(cand, idx))
    assert got == want and len(set(got)) == len(got)
    assert (np.diff(key) >= 0).all()
    tool = np.asarray([per[b][1][i] for b, i in zip(cand, idx)])
    assert n_oo == int((~tool).sum()) and not tool[:n_oo].any() and tool[n_oo:].all()   # every tool entry behind the others
    assert np.array_equal(key[:n_oo], np.asarray([per[b][0][i] for b, i in zip(cand[:n_oo], idx[:n_oo])]))
    same = np.diff(key) == 0
    assert (np.diff(cand)[same] >= 0).all()                    # inside a key: candidate order
    assert (np.diff(cand[:n_oo])[same[:n_oo - 1]] > 0).all()   # an object-object slot at most once per candidate
    # compacted: a slot that few candidates hold takes that many entries, no padding
    held = np.bincount(np.concatenate([s[~t] for s, t, _ in per]), minlength=n_slots)
    assert np.array_equal(np.bincount(key[:n_oo], minlength=n_slots), held)


def test_a_case_where_the_chunk_order_must_beat_the_candidate_order():
    """32 candidates x 64 object-object slots; slot s lights the hidden units of one k-step, the same in every candidate.  A
    wavefront of a candidate's own list holds 32 slots - 32 different k-steps live; a wavefront of the chunk list holds one slot of
    32 candidates - one k-step live, 75 dead."""
    C = _tool()
    Z = C.Z
    B, S = 32, 64
    act = np.zeros((B, S, 150), F32)
    for s in range(S):
        act[:, s, Z.LO[s]] = 1.0
        act[:, s, Z.LO[s] + 4] = 1.0
    per = [(np.arange(S), np.zeros(S, bool), np.zeros((S, 3), F32)) for _ in range(B)]
    cand, idx, key, n_oo = C.chunk_list(per, THR2, S)
    assert n_oo == B * S and np.array_equal(cand[:B], np.arange(B)) and (idx[:B] == 0).all()
    by_candidate = Z.step_shares(act.reshape(B * S, 150))
    by_chunk = Z.step_shares(act[cand, idx])
    assert by_candidate[3] == by_chunk[3]                      # the same (wavefront, k-step) pairs
    # candidate order: 32 keyed steps + the bias step live per wavefront; chunk order: the keyed step (+ the bias step)
    assert by_candidate[2] + by_candidate[1] >= 32 * (B * S // 32)
    assert by_chunk[2] + by_chunk[1] <= 2 * (B * S // 32)
    assert by_chunk[5] * 10 < by_candidate[5]                  # MFMA issue cycles with half-steps
