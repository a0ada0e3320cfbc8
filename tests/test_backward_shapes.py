"""CPU checks of the degenerate-graph batches that tests/test_gpu_backward_shapes.py feeds the HIP backward (tests/backward_shapes.py):
they are what their docstring says, the restatement is well conditioned on them (fp32 within 1e-4 of float64, clamp not engaged)
and no reference gradient is all zero - so the GPU comparisons cannot pass vacuously."""
import numpy as np
import pytest
import torch

import backward_shapes as BS
import train_restate as TR


@pytest.mark.parametrize("N", [97, 65])
def test_graphs_are_what_the_docstring_says(N):
    rng = np.random.default_rng(0)
    g = {k: BS.graph(k, N, rng) for k in BS.KINDS}
    for k, (recv, send) in g.items():
        assert recv.dtype == send.dtype == np.int32 and recv.shape == send.shape
        assert np.all(np.diff(recv) >= 0), k                                    # sorted by receiver
        assert recv.size == 0 or (recv.min() >= 0 and recv.max() < N and send.min() >= 0 and send.max() < N)
    recv, send = g["dense"]
    assert recv.size == 12 * N and np.all(np.bincount(recv, minlength=N) == 12)
    assert len(set(zip(recv.tolist(), send.tolist()))) == recv.size             # distinct senders within a receiver
    assert g["empty"][0].size == 0
    recv, send = g["hub"]
    h = N - 1
    assert recv.size == 2 * (N - 1)
    assert np.bincount(send, minlength=N)[h] == N - 1 and np.bincount(recv, minlength=N)[h] == N - 1
    assert np.all(send[:N - 1] == h) and N - 1 >= 64                              # one sender through a whole sweep and beyond
    assert np.array_equal(np.sort(send[recv == h]), np.arange(N - 1)) and np.array_equal(recv[send == h], np.arange(N - 1))
    recv, send = g["half"]
    touched = np.union1d(recv, send)
    assert touched.max() == N // 2 - 1 and N - touched.size >= N // 2             # half of the nodes: no incident edge
    assert np.all(np.bincount(recv, minlength=N)[:N // 2] == 3)
    assert np.array_equal(send.reshape(-1, 3), np.tile([0, 0, 1], (N // 2, 1)))
    cnt0 = np.bincount(send, minlength=N)[0]
    assert cnt0 >= 64 and recv.size > 64 and send[64:].tolist().count(0) > 0       # sender 0: 64+ edges, in more than one sweep
    assert ((recv == 0) & (send == 0)).sum() == 2 and ((recv == 1) & (send == 1)).sum() == 1   # self edges


def test_row_ptr_of_a_batch_is_consistent():
    N, n_p, n_his, _ = BS.CONFIGS["tool_row"]
    bt = BS.make_batch(N, n_p, n_his, B=5)
    assert bt["kinds"] == ["dense", "empty", "hub", "half", "dense"]
    assert not np.array_equal(bt["state"][0], bt["state"][4]) and np.array_equal(bt["send_l"][0], bt["send_l"][4])
    b4 = BS.make_batch(N, n_p, n_his, B=4)
    assert all(np.array_equal(bt[k][:4], b4[k]) for k in ("state", "action", "phys", "gp", "gm"))   # B = 5 extends B = 4
    assert len({float(v) for v in bt["phys"][:, 0]}) == 5                         # every graph has a physics parameter of its own
    for recv in bt["recv_l"]:
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(recv, minlength=N))])   # as _edge_list builds it
        assert row_ptr[-1] == recv.size
        for i in (0, 1, N // 2, N - 1):
            assert np.all(recv[row_ptr[i]:row_ptr[i + 1]] == i)


@pytest.mark.parametrize("name,B", [(k, 4) for k in BS.CONFIGS] + [("tool_row", 5)])
def test_restatement_is_well_conditioned_on_the_batches(name, B):
    N, n_p, n_his, pstep = BS.CONFIGS[name]
    bt = BS.make_batch(N, n_p, n_his, B=B)
    W = TR.make_weights(5, n_his)
    g64, _, m64 = BS.restate(bt, W, pstep, torch.float64)
    g32, _, _ = BS.restate(bt, W, pstep, torch.float32)
    assert np.abs(m64).max() < 100.0, "the clamp must not be engaged"
    worst = 0.0
    for k in BS.NAMES:
        top = np.abs(g64[k]).max()
        assert top > 0, (name, k)                                                  # no all-zero reference gradient
        worst = max(worst, np.abs(g32[k] - g64[k]).max() / top)
    print(f"{name}: max|motion| {np.abs(m64).max():.3g}, fp32 restatement's worst per-tensor error {worst:.2e} of the tensor's max")
    assert worst <= 1e-4
    # per graph: the state gradient of every graph, the empty one included (d_pos on the last frame), is non-zero, and so is
    # the hub node's
    assert all(np.abs(g64["state"][b]).max() > 0 for b in range(4))
    assert np.abs(g64["state"][2, :, N - 1]).max() > 0


def test_split_k_case_is_well_conditioned():
    """The 33,600-row case of test_gpu_backward_shapes.py::test_split_k_slabs_all_real_rows: row count beyond the 32,768 of
    one-tile slabs, and a seed (BS.SPLITK_SEED) at which no ReLU input within fp32 rounding of zero decides the comparison."""
    N, n_p, n_his, pstep = BS.SPLITK_CONFIG
    bt = BS.dense_batch(N, n_p, n_his, B=4, per_recv=28, seed=BS.SPLITK_SEED)
    assert [len(r) for r in bt["recv_l"]] == [8400] * 4 and 4 * 8400 > 32 * 1024
    for recv, send in zip(bt["recv_l"], bt["send_l"]):
        assert np.all(np.diff(recv) >= 0) and send.min() >= 0 and send.max() < N
    W = TR.make_weights(5, n_his)
    g64, _, m64 = BS.restate(bt, W, pstep, torch.float64)
    g32, _, _ = BS.restate(bt, W, pstep, torch.float32)
    assert np.abs(m64).max() < 100.0
    worst = max(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max() for k in BS.NAMES)
    moved = BS.rounding_sensitivity(bt, W, pstep, g64, BS.NAMES)
    print(f"split-K case: fp32 restatement's worst per-tensor error {worst:.2e} of the tensor's max; float64 gradients move by "
          f"{moved:.2e} under fp32-rounding perturbations of the weights")
    assert all(np.abs(g64[k]).max() > 0 for k in BS.NAMES)
    assert worst <= 1e-4 and moved <= 1e-5
