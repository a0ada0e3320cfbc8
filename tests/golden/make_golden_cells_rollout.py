#!/usr/bin/env python3
"""Generate the fixture of the rollout over cell-list graphs from the REAL reference (jhyau/AdaptiGraph): dynamics()
(src/planning/forward_dynamics.py:12-205) on a cloth ABOVE the LDS-resident builder's 4096 particles, CALLED, not restated.

Runs only where the reference checkout exists (the import recipe and the inert stand-ins of make_golden.py); the tests see only
the .npz file.  The reference pads every graph to max_nR dense one-hot rows - (B, max_nR, N) floats, about 0.5 GB per candidate and
matrix here - and broadcasts a (B, N, N, 3) difference: several GB of host memory in all.

  full_cloth_4097.npz   the 64 x 64 jittered cloth of make_golden_cells.cloth64 (all 4096 rows valid) + one gripper particle,
                        bench.random_weights(0), two candidates of bench.make_actions(2, 1, 3, ...): one look-ahead step x
                        repeat 3 = three forwards per candidate, max_nR = int(1.2 * 6 * 4097) + 64.  Layout of
                        full_cloth_a.npz (make_golden.gen_fullsize; tests/helpers.py: fullsize_records).

Stability precondition, asserted here on the reference's own records (and again by tests/test_rollout_cells_fixture.py): at every
recorded forward the oracle's edge builder returns the recorded list on state_last + u for three seeded draws of u uniform in
+-2 * POS_TOL per coordinate - so an engine that stays within POS_TOL of the reference builds the reference's graphs, and "both
candidates within POS_TOL, no tie excused" is a fair demand.  The action seed is advanced until it holds.

Also written, from the numpy oracle alone: cells_pile_rollout.npz (see pile()).

Usage:  python tests/golden/make_golden_cells_rollout.py [--pile-only]   (rewrites the files; a second run reproduces them bit for bit)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_cells as MC  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import adaptigraph_oracle as O  # noqa: E402
import helpers  # noqa: E402
import cells_rollout_cases as CR  # noqa: E402

POS_TOL = CR.POS_TOL

NAME = "full_cloth_4097"
FIRST_ACTION_SEED = 2501


def stable(g, task):
    """The stability precondition (tests/cells_rollout_cases.py: stable_records) on a fixture in gen_fullsize's layout."""
    return CR.stable_records(O, [recs for recs, _, _ in helpers.fullsize_records(g, task)], task, g["state0"].shape[0])


def drop_weights(W):
    """The 22 weight tensors are bench.random_weights(0), a megabyte of incompressible floats that the tests regenerate from the
    same repo code: checked equal here and left out - their SHA-256 stays in the file, and the tests hold what they regenerate to it -,
    which keeps the file under the repository's 1 MiB limit."""
    path = os.path.join(HERE, NAME + ".npz")
    g = np.load(path)
    for k, v in W.items():
        assert np.array_equal(g["w::" + k], v), k
    np.savez_compressed(path, weights_sha256=CR.weights_sha256(W), **{k: g[k] for k in g.files if not k.startswith("w::")})
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print(f"{NAME}: {size} bytes without the weights")


def pile():
    """cells_pile_rollout.npz: the oracle's rollout of the seeded granular pile (tests/cells_rollout_cases.py), recorded so that the
    GPU test need not run the oracle's dense builder; tests/test_rollout_cells_fixture.py holds the file to the oracle."""
    cloud, a = CR.pile_case()
    task = CR.pile_task()
    tr = []
    out = O.dynamics(O.random_weights(CR.PILE_WEIGHTS_SEED), 3, cloud, a, task, trace=tr)
    assert CR.stable_records(O, tr, task, cloud.shape[0])
    assert min(CR.tool_to_grain_edges(r, cloud.shape[0]) for t in tr for r in t) >= CR.PILE_MIN_TOOL_EDGES
    path = os.path.join(HERE, "cells_pile_rollout.npz")
    np.savez_compressed(path, state0=cloud, action=a, state_seqs=out["state_seqs"])
    print(f"cells_pile_rollout: {cloud.shape[0]} + {task['eef_num']} rows, {os.path.getsize(path)} bytes")


def main():
    pile()
    if "--pile-only" in sys.argv:                          # needs no reference checkout
        return
    refs = MG.import_reference()
    import bench as BN                                     # the benchmark's own input recipe (repo code, not the reference)
    W = BN.random_weights(0)
    cloud = MC.cloth64(np.random.default_rng(2401))["pos"][:-1]          # the 4096 cloth rows; the task's gripper is the tool
    max_nR = int(1.2 * 6 * (cloud.shape[0] + 1)) + 64
    for seed in range(FIRST_ACTION_SEED, FIRST_ACTION_SEED + 32):
        actions = BN.make_actions(2, 1, 3, cloud, np.random.default_rng(seed))
        MG.gen_fullsize(NAME, "cloth", cloud, actions, W, {"max_nR": max_nR}, refs, [0, 1])
        g = helpers.load_golden(NAME)
        if stable(g, helpers.task_of(g)):
            drop_weights(W)
            print(f"{NAME}: action seed {seed}, stable under +-{2 * POS_TOL:g} per coordinate at all {int(g['n_steps'])} forwards")
            return
        print(f"{NAME}: action seed {seed} is not stable, trying the next")
    raise SystemExit("no stable action seed found")


if __name__ == "__main__":
    main()
