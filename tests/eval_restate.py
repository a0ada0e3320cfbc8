"""The step of the open-loop eval rollout (reference src/dynamics/rollout/rollout.py:116-171, 224-233) restated in plain numpy:
the float64 error of a prediction against its ground-truth frame, and the next model input.  The CPU yardstick of
ag_eval_step's advance kernel, pinned to the reference's own rollouts by tests/test_eval_batch_restate.py (fixtures from
tests/golden/make_golden_eval_batch.py)."""
import json
import os

import numpy as np

F32 = np.float32


def error64(pred, gt_frame, fps_idx, n_obj):
    """rollout.py:116-147 in float64 over the fp32 inputs: mean over the n_obj sampled rows of |pred[n] - gt_frame[fps_idx[n]]|.
    pred (max_nobj, 3), gt_frame (N_e, 3) the episode's frame, fps_idx (max_nobj,)."""
    n = int(n_obj)
    d = np.asarray(pred, F32)[:n].astype(np.float64) - np.asarray(gt_frame, F32)[np.asarray(fps_idx[:n], np.int64)].astype(np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).mean() if n else np.float64("nan")


def advance(state, pred, eef_start, eef_end, rest):
    """rollout.py:163-171, 224-233.  state (n_his, N, 3), pred (max_nobj, 3) - ALL rows, padded ones included -, eef_start / eef_end
    (n_eef, 3) the tool points of the next pair's frames -> (state_next (n_his, N, 3), action_next (N, 3)), fp32."""
    state, pred = np.asarray(state, F32), np.asarray(pred, F32)
    es, ee = np.asarray(eef_start, F32), np.asarray(eef_end, F32)
    last = np.concatenate([pred, es], 0)
    action = np.zeros_like(last)
    action[len(pred):] = ee - es
    hist = np.concatenate([state[:1], state[2:], last[None]], 0) if rest else np.concatenate([state[1:], last[None]], 0)
    return hist, action


def load_fixture(name):
    """tests/golden/<name>.npz (make_golden_eval_batch.py) -> dict: the constructor arguments of a dataset, samples (the start
    pairs), w_seed, fps_start / rad_start, fps_idx / n_obj, ref_gap, margins, and per rollout (list `runs`): idx_list, error_list,
    error64, pred, state, action, cloud, recv / send (per step lists), trail (per step, [(kNN, topk, n_rel)])."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    dcfg = json.loads(bytes(g["dataset_config_json"]).decode())
    mcfg = json.loads(bytes(g["material_config_json"]).decode())
    material = dcfg["materials"][0]
    n = int(g["n_episodes"])
    runs = []
    for j in range(len(g["samples"])):
        pre = f"r{j}::"
        r = {k: g[pre + k] for k in ("idx_list", "error_list", "error64", "pred", "state", "action", "cloud")}
        off = np.concatenate([[0], np.cumsum(g[pre + "n_edges"])])
        r["recv"] = [g[pre + "recv"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
        r["send"] = [g[pre + "send"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
        toff = np.concatenate([[0], np.cumsum(g[pre + "trail"])])
        r["trail"] = [[(float(a[0]), int(a[1]), int(a[2])) for a in g[pre + "trail::rows"][toff[i]:toff[i + 1]]] for i in range(len(toff) - 1)]
        runs.append(r)
    return dict(dataset_config=dcfg, material_config=mcfg, pair_lists=g["pair_lists"], material=material,
                physics_params=[{material: g[f"ep{e}::phys"]} for e in range(n)], obj_pos=[g[f"ep{e}::obj"] for e in range(n)],
                eef_pos=[g[f"ep{e}::eef"] for e in range(n)], samples=g["samples"], w_seed=int(g["w_seed"]),
                fps_start=g["draw::fps_start"], rad_start=g["draw::rad_start"], fps_idx=g["fps_idx"], n_obj=g["n_obj"],
                ref_gap=float(g["ref_gap"]), margin_radius=float(g["margin_radius"]), margin_topk=float(g["margin_topk"]), runs=runs)


def dataset_args(fx):
    return (fx["dataset_config"], fx["material_config"], fx["pair_lists"], fx["physics_params"], fx["obj_pos"], fx["eef_pos"])
