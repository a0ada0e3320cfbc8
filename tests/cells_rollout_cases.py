"""Shared by tests/test_rollout_cells_fixture.py, tests/test_gpu_rollout_cells.py and tests/golden/make_golden_cells_rollout.py:
the stability precondition of a recorded rollout and the seeded granular pile above 4096 particles.  No test lives here."""
import hashlib

import numpy as np

POS_TOL = 1e-5                      # tests/test_gpu_parity.py
STABLE_DRAWS, STABLE_SEED = 3, 2500


def stable_records(O, traces, task, N_o, draws=STABLE_DRAWS, seed=STABLE_SEED):
    """The stability precondition.  traces: per candidate a list of per-forward records ('state_last' (N,3), 'recv', 'send').
    True when, at every forward, the oracle's edge builder returns the recorded list on state_last + u for `draws` seeded draws of
    u uniform in +-2 * POS_TOL per coordinate: a rollout that stays within POS_TOL of the recorded one then builds the recorded
    graphs, and no tie verdict is needed to explain a difference.  (O.selection_margin is not this test: its radius term counts
    pairs that the top-k never keeps.)"""
    N = traces[0][0]["state_last"].shape[0]
    mask = np.ones(N, bool)
    tool = np.zeros(N, bool)
    tool[N_o:] = True
    rng = np.random.default_rng(seed)
    for recs in traces:
        for rec in recs:
            for _ in range(draws):
                u = rng.uniform(-2 * POS_TOL, 2 * POS_TOL, rec["state_last"].shape).astype(np.float32)
                r, s = O.construct_edges_single(rec["state_last"] + u, task["adj_thresh"], mask, tool, task["topk"],
                                                task["connect_tools_all"])
                if not (np.array_equal(r, rec["recv"]) and np.array_equal(s, rec["send"])):
                    return False
    return True


def weights_sha256(W):
    """one SHA-256 over the weight tensors of a state dict (name -> float32 array), in the order of their names"""
    h = hashlib.sha256()
    for k in sorted(W):
        h.update(k.encode())
        h.update(np.ascontiguousarray(W[k], np.float32).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


# ---- granular pile above the limit: the 5-point pusher, top-k 20, radius 0.4, 125 grains per unit volume (the density of
# tests/golden/cells_pile.npz).  Size: the oracle's dense N x N builder costs seconds per forward (4.4 s at 5005 rows), and the
# precondition calls it for every forward and draw, so the pile has 4536 + 5 rows.
#
# Layout.  At this density a grain has about 33 others inside the radius, so with grains placed uniformly at random the top-k
# binds at nearly every row and the gap between a row's 20th and 21st nearest sender is below the 1e-4 that a +-2 * POS_TOL
# perturbation moves a squared distance for some twenty rows of every forward: no seed can satisfy the precondition.  So the
# grains sit in clumps on a lattice of pitch (14 / 125)^(1/3) = 0.482, 8 x 5 x 8 clumps, a clump's grains within +-0.02 of its
# centre (grains of different clumps are at least 0.44 apart, outside the radius):
#   * 312 ordinary clumps of 14 grains.  A grain row holds its clump and whatever tools are inside the radius - at most
#     14 + 5 = 19 senders, so a TOOL SENDER IS NEVER CUT by the top-k: the pushes run through the bottom layer, whose clump centres
#     are at most 0.35 from any point of the footprint, so every tool sends into grains at every forward and the tools' placement,
#     height and per-step delta all reach the result (tests/test_rollout_cells_fixture.py counts those edges per forward);
#   * 8 clumps of the top layer, out of the tools' reach, hold 21 grains: 20 on a short vertical line (spacing 0.004) and one 0.3
#     above it, more than 0.56 from every other clump.  All 21 are inside each other's radius, so the top-k BINDS at each of
#     these 168 rows, with a rank gap far above the perturbation: a line grain drops the far grain (squared distances <= 0.006 against >= 0.068), the far grain drops the
#     line's last grain (neighbouring squared distances differ by 2.4e-3).
# What decides a graph is then either out of a perturbation's reach or - the radius test between a tool and the grains around it -
# left to the seeds, which are chosen so that the precondition holds.  That goes for the seed of the random model weights too: a
# model that throws the grains a tool touches by more than the lattice's gaps merges clumps at the second forward, and merged clumps
# bind the top-k at random gaps; O.random_weights(5) moves a grain by at most 0.10 per forward.
PILE_GRID, PILE_K, PILE_BIG, PILE_SEED, PILE_WEIGHTS_SEED = (8, 5, 8), 14, 8, 2601, 5
PILE_N = PILE_GRID[0] * PILE_GRID[1] * PILE_GRID[2] * PILE_K + PILE_BIG * (21 - PILE_K)
PILE_MIN_TOOL_EDGES = 14                                     # tool -> grain edges per forward and candidate: a whole clump at least


def pile_task():
    return dict(sim_real_ratio=10, max_n=1, n_his=4, material="granular", material_dims={"granular": 1},
                material_indices={"granular": 0}, adj_thresh=0.4, topk=20, connect_tools_all=False, push_length=0.2,
                gripper_enable=False, eef_num=5, max_nR=120000,
                pusher_points=[[0, 0, 0.1], [0, 0.05, 0.1], [0, 0.025, 0.1], [0, -0.025, 0.1], [0, -0.05, 0.1]])


def pile_case(seed=PILE_SEED):
    """-> (cloud (PILE_N,3), actions (2,1,4)): B = 2, one look-ahead step x repeat 2, pushes that stay inside the footprint."""
    rng = np.random.default_rng(seed)
    pitch = (PILE_K / 125.0) ** (1.0 / 3.0)
    gx, gy, gz = PILE_GRID
    centres = np.stack(np.meshgrid(*[np.arange(n) * pitch for n in PILE_GRID], indexing="ij"), -1).reshape(-1, 3)
    layer = np.arange(len(centres)) // gz % gy
    top = np.nonzero(layer == gy - 1)[0]
    big = set(top[np.linspace(0, len(top) - 1, PILE_BIG).astype(int)].tolist())
    parts = []
    for c, centre in enumerate(centres):
        if c in big:
            u = np.array([0.0, 1.0, 0.0])                    # upwards: nothing of another clump comes inside the far grain's radius
            t = np.concatenate([(np.arange(20) - 9.5) * 0.004, [0.3]])
            parts.append(centre + t[:, None] * u + rng.uniform(-0.0005, 0.0005, (21, 3)))
        else:
            parts.append(centre + rng.uniform(-0.02, 0.02, (PILE_K, 3)))
    cloud = np.concatenate(parts).astype(np.float32)
    assert cloud.shape[0] == PILE_N
    cloud = cloud[rng.permutation(PILE_N)]                   # a clump's grains are not neighbours in memory
    mid = centres.mean(0)
    a = np.zeros((2, 1, 4), np.float32)
    a[..., 0] = mid[0] + rng.uniform(-0.5, 0.5, (2, 1))
    a[..., 1] = mid[2] + rng.uniform(-0.5, 0.5, (2, 1))
    a[..., 2] = rng.uniform(-3.1, 3.1, (2, 1))
    a[..., 3] = 2.5
    return cloud, a


def tool_to_grain_edges(rec, N_o):
    """edges of one recorded forward whose sender is a tool and whose receiver is a grain"""
    return int(((rec["send"] >= N_o) & (rec["recv"] < N_o)).sum())
