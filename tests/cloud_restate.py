"""perception.construct_graph (reference src/planning/perception.py:259-315) and the array half of get_state_cur
(perception.py:335-341) restated in plain numpy as functions of (points, draws): the CPU yardstick of adaptigraph_amd.perception.

The sampling is dataset_restate.fps_indices, whose stage 1 is dgl's CPU farthest-point sampler as remembered - dgl is not installed
where this project is developed, and the reference's construct_graph imports dgl and open3d, so nothing here could be run against
the reference's own function.  The padding below follows the reference line by line."""
import numpy as np

import dataset_restate as DR

F32 = np.float32


def construct_graph(obj_kps, fps_radius, draws, max_nobj=100, max_neef=8, eef_kps=None):
    """draws: one (fps_start, rad_start) per object.  Arrays are float32 (the reference's `state` is float64 holding these values)."""
    if eef_kps is None:
        eef_kps = np.zeros((0, 3), F32)
    if not isinstance(obj_kps, list):
        obj_kps = [obj_kps]
    fps_idx_list = [DR.fps_indices(obj_kps[j], max_nobj, draws[j][0], fps_radius, draws[j][1]).astype(np.int32)
                    for j in range(len(obj_kps))]
    obj = np.concatenate([np.asarray(obj_kps[j], F32)[idx] for j, idx in enumerate(fps_idx_list)], axis=0)
    obj_kp_num, eef_kp_num = obj.shape[0], eef_kps.shape[0]
    state_mask = np.zeros(max_nobj + max_neef, bool)
    state_mask[max_nobj:max_nobj + eef_kp_num] = True
    state_mask[:obj_kp_num] = True
    eef_mask = np.zeros(max_nobj + max_neef, bool)
    eef_mask[max_nobj:max_nobj + eef_kp_num] = True
    state = np.zeros((max_nobj + max_neef, 3), F32)
    state[:obj_kp_num] = obj                               # (the reference fails here when the objects exceed max_nobj)
    state[max_nobj:max_nobj + eef_kp_num] = eef_kps
    return dict(obj_state=obj, obj_state_raw=obj[:obj_kp_num], eef_state=np.asarray(eef_kps, F32), state=state,
                state_mask=state_mask, eef_mask=eef_mask, fps_idx_list=fps_idx_list)


def transform(points, sim_real_ratio):
    """perception.py:335-337."""
    obj_kps = np.array(points).astype(F32) * sim_real_ratio
    obj_kps = obj_kps[:, [0, 2, 1]].copy()
    obj_kps[:, 1] *= -1
    return obj_kps
