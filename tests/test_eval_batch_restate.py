"""CPU checks of the batched eval rollout's host side: eval_schedule against the reference's idx_list, eval_draws, EvalResult's
statistics, and the numpy restatement of the step (tests/eval_restate.py) against the reference's own rollouts
(tests/golden/eval_batch_*.npz)."""
import numpy as np
import pytest
import torch

import eval_restate as ER
from adaptigraph_amd.dataset import frame_table, parse_config

FIXTURES = ["eval_batch_rope", "eval_batch_rest"]


def _tables(fx):
    spec = parse_config(fx["dataset_config"], fx["material_config"], "valid")
    frames = frame_table(spec, fx["pair_lists"])
    episode = np.asarray(fx["pair_lists"])[:, 0]
    return spec, frames, episode


@pytest.mark.parametrize("name", FIXTURES)
def test_eval_schedule_equals_the_references_idx_list(name):
    from adaptigraph_amd import eval_schedule
    fx = ER.load_fixture(name)
    spec, frames, episode = _tables(fx)
    assert spec.store_rest_state == (name == "eval_batch_rest") and frames.shape[1] == spec.n_his + spec.n_future
    lengths = []
    for j, i in enumerate(fx["samples"]):
        rows = frames[episode == episode[i]]
        n_frames = fx["obj_pos"][int(episode[i])].shape[0]
        want = [tuple(int(v) for v in p) for p in fx["runs"][j]["idx_list"]]
        got = eval_schedule(rows, frames[i], spec.n_his, n_frames)
        assert got == want, (j, got, want)
        # every chain here ends because no pair follows its last frame: one more step is not there to take
        assert not ((rows[:, spec.n_his - 1] == want[-1][1]) & (rows[:, spec.n_his] > want[-1][1])).any()
        assert eval_schedule(rows, frames[i], spec.n_his, n_frames, rollout_steps=3) == want[:3]
        assert eval_schedule(rows, frames[i], spec.n_his, n_frames, rollout_steps=1) == want[:1]
        lengths.append(len(got))
    assert len(set(lengths)) == len(lengths) and min(lengths) >= 2 and max(lengths) <= 8


def test_eval_schedule_takes_the_middle_of_the_valid_rows():
    from adaptigraph_amd import eval_schedule
    fr = np.array([[0, 1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 4, 5, 6], [1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 6, 7, 8], [1, 2, 3, 4, 7, 8, 9],
                   [3, 4, 5, 6, 9, 9, 9], [3, 4, 5, 7, 8, 9, 9]])
    # after (3, 4): rows 2, 3, 4 start at 4 and move on (row 1 does not move: the loop guard) -> the middle one, row 3
    assert eval_schedule(fr, fr[0], 4, 10) == [(3, 4), (4, 6), (6, 9)]
    with pytest.raises(ValueError):
        eval_schedule(fr, fr[0], 4, 9)                       # a frame beyond the episode


def test_eval_draws_are_the_midpoints():
    from adaptigraph_amd.dataset import DeviceDynDataset
    fx = ER.load_fixture("eval_batch_rope")
    ds = object.__new__(DeviceDynDataset)                    # the host half only: no device, no library
    ds.spec, ds.device, ds.phys_dim = parse_config(fx["dataset_config"], fx["material_config"], "valid"), torch.device("cpu"), 1
    d = fx["dataset_config"]["datasets"][0]
    dr = ds.eval_draws([3, 1, 2])
    assert dr.fps_radius.dtype == torch.float32 and dr.fps_radius.tolist() == [np.float32(sum(d["fps_radius_range"]) / 2)] * 3
    assert dr.adj_thresh.dtype == torch.float64 and dr.adj_thresh.tolist() == [sum(d["adj_radius_range"]) / 2] * 3
    assert dr.knn_thresh.tolist() == [1.0] * 3
    assert dr.fps_start.tolist() == [0, 0, 0] and dr.rad_start.tolist() == [0, 0, 0] and dr.fps_start.dtype == torch.int32
    assert dr.state_noise is None and dr.rot is None and dr.phys_noise.shape == (3, 1) and not dr.phys_noise.any()
    dr = ds.eval_draws([3, 1, 2], fps_start=[5, 6, 7], rad_start=2)
    assert dr.fps_start.tolist() == [5, 6, 7] and dr.rad_start.tolist() == [2, 2, 2]


def test_eval_result_statistics_equal_numpy():
    from adaptigraph_amd import EvalResult
    nan = float("nan")
    table = np.array([[0.5, 0.1, 0.3, 0.9], [0.25, 0.2, 0.7, 0.1], [0.125, nan, 0.2, 0.4], [nan, nan, 0.6, 0.3]], np.float32)
    res = EvalResult(torch.from_numpy(table), np.array([3, 2, 4, 4]), [[]] * 4, [[]] * 4)
    se = res.step_error()
    assert se.shape == (2, 4) and se.dtype == np.float64 and np.array_equal(se, table[:2].astype(np.float64))
    s = res.summary()
    assert np.array_equal(s["median"], np.median(se, axis=1)) and np.array_equal(s["p25"], np.percentile(se, 25, axis=1))
    assert np.array_equal(s["p75"], np.percentile(se, 75, axis=1))


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_step_reproduces_the_references_rollouts(name):
    fx = ER.load_fixture(name)
    spec, _, episode = _tables(fx)
    assert fx["margin_radius"] >= 1e-4 and fx["margin_topk"] >= 1e-4
    backed = 0
    for j, (i, r) in enumerate(zip(fx["samples"], fx["runs"])):
        e = int(episode[i])
        obj, eef = fx["obj_pos"][e], fx["eef_pos"][e]
        L = len(r["idx_list"])
        assert r["pred"].shape == (L, spec.max_nobj, 3) and r["state"].shape == (L, spec.n_his, spec.max_nobj + eef.shape[1], 3)
        for s in range(L):
            end = int(r["idx_list"][s][1])
            err = ER.error64(r["pred"][s], obj[end], fx["fps_idx"][j], fx["n_obj"][j])
            assert err == r["error64"][s]
            assert abs(err - float(r["error_list"][s])) <= fx["ref_gap"]
            if s + 1 < L:
                ns, ne = (int(v) for v in r["idx_list"][s + 1])
                state, action = ER.advance(r["state"][s], r["pred"][s], eef[ns], eef[ne], spec.store_rest_state)
                assert np.array_equal(state, r["state"][s + 1]) and np.array_equal(action, r["action"][s + 1])
                assert np.array_equal(r["cloud"][s], state[-1])
            assert r["trail"][s][-1][2] == len(r["recv"][s]) <= spec.max_nR and r["trail"][s][0][1] == spec.topk
            backed += s > 0 and len(r["trail"][s]) > 1
    assert backed >= 1                                        # a rebuilt graph takes the top-k back-off
    assert len(set(fx["n_obj"].tolist())) >= 3 and fx["n_obj"].min() < spec.max_nobj
