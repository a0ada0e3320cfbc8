"""The numpy restatement of the class-major work-list key (tools/zero_skip_census.py --order, csrc/ag_edges.hip: k_ell_index) on a
hand-made graph: a 5 x 5 grid in the x-z plane, one tool particle above its centre, every particle connected to its grid
neighbours (8-neighbourhood) and the tool to and from every particle within reach.  CPU only; the oracle rollout is not run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _census():
    spec = importlib.util.spec_from_file_location("zero_skip_census", os.path.join(ROOT, "tools", "zero_skip_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _graph():
    g = np.arange(5, dtype=np.float32) * np.float32(0.25)
    xx, zz = np.meshgrid(g, g, indexing="ij")
    pos = np.stack([xx.ravel(), np.zeros(25, np.float32), zz.ravel()], 1).astype(np.float32)
    pos[7, 1] = 0.4                                            # one particle lifted: its edges have y as the dominant axis
    pos = np.concatenate([pos, np.array([[0.5, 0.3, 0.5]], np.float32)])   # particle 25: the tool
    recv, send = [], []
    for i in range(26):                                        # slot order: receiver-major, senders ascending
        for j in range(26):
            if i == j:
                continue
            if i == 25 or j == 25:
                near = np.abs(pos[i, [0, 2]] - pos[j, [0, 2]]).max() <= 0.3
            else:
                near = np.abs(pos[i, [0, 2]] - pos[j, [0, 2]]).max() <= 0.26
            if near:
                recv.append(i)
                send.append(j)
    return pos, np.asarray(recv), np.asarray(send)


def test_slot_order_is_the_identity():
    C = _census()
    pos, recv, send = _graph()
    perm, n_oo = C.work_list_order(recv, send, pos, 25, "slot")
    assert np.array_equal(perm, np.arange(len(recv))) and n_oo == len(recv)


def test_class_order_is_a_permutation_with_the_tool_edges_last_and_slot_order_inside_a_class():
    C = _census()
    pos, recv, send = _graph()
    n = len(recv)
    tool = (recv == 25) | (send == 25)
    assert 0 < tool.sum() < n
    for order in ("tool-last", "class"):
        perm, n_oo = C.work_list_order(recv, send, pos, 25, order)
        assert np.array_equal(np.sort(perm), np.arange(n))    # a permutation of the slot-order list
        assert n_oo == n - tool.sum()
        assert not tool[perm[:n_oo]].any() and tool[perm[n_oo:]].all()          # every tool edge last
        assert (np.diff(perm[n_oo:]) > 0).all()                # slot order inside the tool class
    perm, n_oo = C.work_list_order(recv, send, pos, 25, "class")
    cls = C.edge_classes(recv, send, pos, 25)
    assert (np.diff(cls[perm]) >= 0).all()                     # class-major
    for c in np.unique(cls):
        assert (np.diff(perm[cls[perm] == c]) > 0).all()       # slot order inside every class
    # the key itself: sign bits (x, y, z) x dominant axis, ties to the lower axis, the tool class 24
    assert (cls[tool] == 24).all() and (cls[~tool] < 24).all()
    d = pos[recv] - pos[send]
    e = int(np.flatnonzero((recv == 6) & (send == 0))[0])     # d = (+0.25, 0, +0.25): no sign bit, tie x/z -> x
    assert tuple(d[e]) == (0.25, 0.0, 0.25) and cls[e] == 0
    e = int(np.flatnonzero((recv == 0) & (send == 6))[0])     # d = (-0.25, 0, -0.25): sign bits x and z (1 + 4), axis x
    assert cls[e] == 5 * 3 + 0
    e = int(np.flatnonzero((recv == 1) & (send == 0))[0])     # d = (0, 0, +0.25): axis z
    assert cls[e] == 2
    e = int(np.flatnonzero((recv == 2) & (send == 7))[0])     # d = (-0.25, -0.4, 0): sign bits x and y, axis y
    assert cls[e] == 3 * 3 + 1
    assert len(np.unique(cls[~tool])) >= 8                    # the grid's eight directions, and the lifted particle's


def test_a_nan_position_compares_false():
    C = _census()
    pos, recv, send = _graph()
    pos = pos.copy()
    pos[0] = np.nan
    cls = C.edge_classes(recv, send, pos, 25)
    assert (cls[((recv == 0) | (send == 0)) & (recv != 25) & (send != 25)] == 0).all()   # no sign bit, axis x
