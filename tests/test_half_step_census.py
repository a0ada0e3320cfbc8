"""The half-dead column of tools/zero_skip_census.py (Options::half_step) on a tiny graph: activations of 70 rows - two full
wavefronts and a ragged one - with hand-set dead units.  CPU only; the oracle rollout is not run."""
import numpy as np

from test_edge_order_census import _census


def _acts():
    rng = np.random.default_rng(7)
    act = rng.uniform(0.1, 1.0, (70, 150)).astype(np.float32)
    act[rng.uniform(size=act.shape) < 0.3] = 0.0               # scattered zeros: a unit is rarely off in all 32 rows
    act[:32, [1, 5]] = 0.0                                      # wavefront 0: step (1, 5) dead, steps (2, 6) and (3, 7) half-dead
    act[:32, [2, 7]] = 0.0
    act[32:64, 16:24] = 0.0                                     # wavefront 1: a dead chunk
    act[32:64, 146] = 0.0                                       # ... and 146, whose partner is the bias slot: half-dead
    act[64:, 40:80] = 0.0                                       # the ragged wavefront
    return act


def test_the_columns_sum_to_one_and_the_dead_one_is_dead_share():
    C = _census()
    act = _acts()
    for first_row in (0, 13):                                   # rows that start inside a wavefront (propagate chains of candidate > 0)
        dead, half, live, pairs, c0, c1, b0, b1 = C.step_shares(act, first_row)
        ds, dc, ns, nc = C.dead_share(act, first_row)
        assert pairs == ns and dead == ds
        assert dead + half + live == pairs
        assert c0 == C.CYC_FULL * (half + live) and c1 == C.CYC_FULL * live + C.CYC_HALF * half
        assert b0 >= c0 and b1 >= c1 and c1 < c0


def test_the_crafted_steps_land_in_their_columns():
    C = _census()
    act = _acts()
    dead, half, live, pairs, *_ = C.step_shares(act[:32])
    # wavefront 0 alone: (1, 5) dead; (2, 6), (3, 7) half; (147, 151) half with the padding slot; everything else live
    assert (dead, half, live, pairs) == (1, 3, 72, 76)
    dead, half, live, pairs, *_ = C.step_shares(act[32:64])
    # wavefront 1: units 16..23 are the four steps of chunk 2; (146, 150) and (147, 151) half
    assert (dead, half, live, pairs) == (4, 2, 70, 76)
    assert C.dead_share(act[32:64])[1] == 1


def test_the_tile_mask_selects_whole_tiles():
    C = _census()
    act = np.concatenate([_acts()] * 4)                         # 280 rows: tiles of 128, 128 and 24 rows
    every = C.step_shares(act)
    first = C.step_shares(act, 0, lambda e0: e0 < 128)
    rest = C.step_shares(act, 0, lambda e0: e0 >= 128)
    assert first[3] == 4 * 76 and first[3] + rest[3] == every[3]
    assert all(a + b == c for a, b, c in zip(first, rest, every))
