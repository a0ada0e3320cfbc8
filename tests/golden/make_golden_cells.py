#!/usr/bin/env python3
"""Generate the fixtures of the cell-list edge builder from the REAL reference (jhyau/AdaptiGraph): graphs ABOVE the
LDS-resident builder's 4096 particles, built by the reference's own construct_edges_from_states_batch
(src/dynamics/dataset/graph.py:233-298), which is CALLED, not restated.

Runs only where the reference checkout exists (the import recipe and the inert stand-ins of make_golden.py); the tests see only
the .npz files.  Stored: the inputs (positions, masks, threshold, top-k, connect_tools_all) and the int32 (recv, send) lists,
nothing dense.  The reference's dense (1, n_rel, N) one-hot pair needs about 6 GB for the second fixture.

  cells_cloth64.npz   64 x 64 grid of pitch 0.3 with N(0, 0.02^2) jitter on every coordinate, one tool particle above the
                      centre (last row), 37 object rows masked out; thr 0.75, topk 5, connect_tools_all=True; 4097 rows
  cells_pile.npz      6000 object + 5 tool particles uniform in a 4 x 3 x 4 box; thr 0.4, topk 20, connect_tools_all=False

For both, the numpy oracle must give the same lists and find no tie at the k-th boundary inside the radius (check_ties=True):
torch.topk's choice among equal distances is implementation-defined, and a fixture must not depend on it.

Usage:  python tests/golden/make_golden_cells.py          (rewrites both files; a second run reproduces them bit for bit)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import adaptigraph_oracle as O  # noqa: E402


def cloth64(rng):
    n, pitch = 64, 0.3
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pos = np.stack([ii.ravel() * pitch, np.zeros(n * n), jj.ravel() * pitch], 1) + rng.normal(0, 0.02, (n * n, 3))
    centre = np.array([[(n - 1) * pitch / 2, 0.1, (n - 1) * pitch / 2]])
    pos = np.concatenate([pos, centre]).astype(np.float32)
    N = n * n + 1
    mask = np.ones(N, bool)
    mask[rng.choice(n * n, 37, replace=False)] = False
    tool = np.zeros(N, bool)
    tool[-1] = True
    return dict(pos=pos, mask=mask, tool=tool, thr=0.75, topk=5, cta=True)


def pile(rng):
    N_o, M = 6000, 5
    pos = (rng.uniform(0, 1, (N_o + M, 3)) * [4.0, 3.0, 4.0]).astype(np.float32)
    mask = np.ones(N_o + M, bool)
    tool = np.zeros(N_o + M, bool)
    tool[N_o:] = True
    return dict(pos=pos, mask=mask, tool=tool, thr=0.4, topk=20, cta=False)


def reference_edges(build, c):
    t = torch.from_numpy
    Rr, Rs = build(t(c["pos"])[None], c["thr"], t(c["mask"])[None], t(c["tool"])[None], topk=c["topk"],
                   connect_tools_all=c["cta"])
    valid = Rr[0].sum(-1) > 0
    n = int(valid.sum())
    assert bool(valid[:n].all()) and torch.equal(valid, Rs[0].sum(-1) > 0)
    return Rr[0, :n].argmax(-1).to(torch.int32).numpy(), Rs[0, :n].argmax(-1).to(torch.int32).numpy()


def main():
    _, build, _, _ = MG.import_reference()
    for name, make, seed in (("cells_cloth64", cloth64, 2401), ("cells_pile", pile, 2402)):
        c = make(np.random.default_rng(seed))
        recv, send = reference_edges(build, c)
        o_recv, o_send = O.construct_edges_single(c["pos"], c["thr"], c["mask"], c["tool"], c["topk"], c["cta"], check_ties=True)
        assert np.array_equal(recv, o_recv) and np.array_equal(send, o_send), name
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, pos=c["pos"], mask=c["mask"], tool=c["tool"], thr=np.float64(c["thr"]), topk=np.int32(c["topk"]),
                            cta=np.bool_(c["cta"]), recv=recv, send=send)
        print(f"{name}: {len(c['pos'])} rows, {len(recv)} edges, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
