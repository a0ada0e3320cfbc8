"""DynDataset.__getitem__ (reference src/dynamics/dataset/dataset.py:117-383) restated in plain numpy as a function of
(sample, draws): the CPU yardstick of adaptigraph_amd.dataset, pinned to the reference's own output by
tests/test_dataset_restate.py (fixtures from tests/golden/make_golden_dataset.py).

The farthest-point stage 1 below is dgl.geometry.farthest_point_sampler restated from its CPU implementation as remembered; dgl is
not installed anywhere this project runs, so that one function is a specification, not a verified copy.  Everything else ran
against the reference's own code when the fixtures were made.
"""
import numpy as np

from adaptigraph_amd.dataset import frame_table, parse_config, plane_bounds
from oracle import adaptigraph_oracle as O

F32 = np.float32


def sq_dist(p, c):
    """fp32 ((dx*dx + dy*dy) + dz*dz), separate products and sums."""
    d = p - c
    s = d * d
    return (s[:, 0] + s[:, 1]) + s[:, 2]


def fps_stage1(points, n_sample, start):
    """Farthest-point sampling as dgl's CPU kernel does it: running minimum of the squared distance initialised to 1e10, the next
    point is the strict-greater argmax (np.argmax: the lowest index among equals)."""
    p = np.ascontiguousarray(points, F32)
    md = np.full(len(p), F32(1e10))
    idx = np.empty(n_sample, np.int64)
    idx[0] = cur = int(start)
    for t in range(1, n_sample):
        md = np.minimum(md, sq_dist(p, p[cur]))
        idx[t] = cur = int(np.argmax(md))
    return idx


def fps_stage2(points, radius, start):
    """fps_rad_idx (src/dynamics/utils.py:10-24) with its draw as an argument.  radius is compared as fp32."""
    p = np.ascontiguousarray(points, F32)
    r = F32(radius)
    lst = [int(start)]
    dist = np.sqrt(sq_dist(p, p[lst[0]]))
    while dist.max() > r and len(lst) < len(p):          # (the cap is unreachable for a radius >= 0: a chosen point is at 0)
        lst.append(int(dist.argmax()))
        dist = np.minimum(dist, np.sqrt(sq_dist(p, p[lst[-1]])))
    return np.array(lst, np.int64)


def fps_indices(cloud, max_nobj, fps_start, fps_radius, rad_start):
    """graph.py:8-36: stage1[stage2], in selection order."""
    cloud = np.ascontiguousarray(cloud, F32)
    i1 = fps_stage1(cloud, min(max_nobj, len(cloud)), fps_start)
    return i1[fps_stage2(cloud[i1], fps_radius, rad_start)]


def rotate(x, ang):
    """x @ rot_mat (dataset.py:277-285) on fp32 rows: two-term fp32 dot products, z untouched."""
    c, s = F32(np.cos(ang)), F32(np.sin(ang))
    out = x.copy()
    out[..., 0] = x[..., 0] * c + x[..., 1] * s
    out[..., 1] = x[..., 0] * (-s) + x[..., 1] * c
    return out


def restate_item(spec, frames, obj, eef, phys, draws, trail=None):
    """One sample.  frames: (n_his + n_future,) frame indices (frame_table's row); obj (T_e, N_e, 3), eef (T_e, n_eef, 3) the
    episode; phys: its stored parameter vector; draws: dict with fps_start, fps_radius, rad_start, phys_noise, state_noise, rot,
    adj_thresh, knn_thresh (None where the config draws nothing).  Returns numpy arrays under the reference's keys plus fps_idx,
    recv, send (the edges in nonzero order)."""
    nh, nf, No = spec.n_his, spec.n_future, spec.max_nobj
    obj_kps = np.asarray(obj, F32)[frames]
    eef_kps = np.asarray(eef, F32)[frames]
    n_eef = eef_kps.shape[1]
    N = No + n_eef
    idx = fps_indices(obj_kps[nh - 1], No, draws["fps_start"], draws["fps_radius"], draws["rad_start"])
    n = len(idx)
    kps = np.zeros((len(frames), No, 3), F32)
    kps[:, :n] = obj_kps[:, idx]
    state = np.zeros((nh, N, 3), F32)
    state[:, :No] = kps[:nh]
    state[:, No:] = eef_kps[:nh]
    bounds = plane_bounds(kps[nh - 1], spec.connect_tool_surface_ratio)
    action = np.zeros((N, 3), F32)
    action[No:] = eef_kps[nh] - eef_kps[nh - 1]
    state_future = kps[nh:nh + nf].copy()
    eef_future = np.zeros((nf - 1, N, 3), F32)
    action_future = np.zeros((nf - 1, N, 3), F32)
    for fi in range(nf - 1):
        eef_future[fi, No:] = eef_kps[nh + fi]
        action_future[fi, No:] = eef_kps[nh + fi + 1] - eef_kps[nh + fi]
    state_mask = np.zeros(N, bool)
    state_mask[:n] = True
    state_mask[No:] = True
    eef_mask = np.zeros(N, bool)
    eef_mask[No:] = True
    attrs = np.zeros((N, 2), F32)
    attrs[:n, 0] = 1
    attrs[No:, 1] = 1
    p_instance = np.zeros((No, 1), F32)
    p_instance[:n] = 1
    material_index = np.zeros((No, spec.n_mat), np.int64)
    material_index[:n, spec.mat_col] = 1
    pn = draws.get("phys_noise")
    physics_param = (np.asarray(phys, np.float64) + (0.0 if pn is None else np.asarray(pn, np.float64))).astype(F32)
    if spec.add_randomness:
        state += np.asarray(draws["state_noise"], np.float64)                        # fp32 += fp64: double sum, one rounding
        ang = float(draws["rot"])
        state, action, eef_future = rotate(state, ang), rotate(action, ang), rotate(eef_future, ang)
        action_future, state_future = rotate(action_future, ang), rotate(state_future, ang)
    cfg = dict(connect_tool_all=spec.connect_tool_all, connect_tool_surface=spec.connect_tool_surface,
               connect_tool_all_non_fixed=spec.connect_tool_all_non_fixed, knn_thresh=float(draws["knn_thresh"]), topk=spec.topk,
               adj_thresh=float(draws["adj_thresh"]), max_nR=spec.max_nR, min_kNN=spec.min_kNN, knn_increment=spec.knn_increment)
    recv, send = O.edges_with_backoff(state[-1], cfg, state_mask, eef_mask, bounds, trail=trail)
    obj_mask = np.zeros(No, bool)
    obj_mask[:n] = True
    return dict(state=state, action=action, eef_future=eef_future, action_future=action_future, state_future=state_future,
                attrs=attrs, p_rigid=np.zeros(1, F32), p_instance=p_instance, obj_mask=obj_mask, material_index=material_index,
                physics_param=physics_param, fps_idx=idx.astype(np.int32), recv=recv, send=send)


def restate_batch(dataset_config, material_config, pair_lists, physics_params, obj_pos, eef_pos, idx, draws, phase="train"):
    """The collated batch of samples idx.  draws: dict of (B, ...) arrays (None entries allowed).  Returns (dict of stacked arrays,
    with recv / send / fps_idx as per-sample lists, and trail = the back-off attempts per sample)."""
    spec = parse_config(dataset_config, material_config, phase)
    frames = frame_table(spec, pair_lists)
    episode = np.asarray(pair_lists).astype(np.int64)[:, 0]
    items, trails = [], []
    for b, i in enumerate(idx):
        e = int(episode[i])
        d = {k: (None if v is None else v[b]) for k, v in draws.items()}
        trail = []
        items.append(restate_item(spec, frames[i], obj_pos[e], eef_pos[e], physics_params[e][spec.material], d, trail))
        trails.append(trail)
    out = {k: np.stack([it[k] for it in items]) for k in items[0] if k not in ("recv", "send", "fps_idx")}
    for k in ("recv", "send", "fps_idx"):
        out[k] = [it[k] for it in items]
    out["trail"] = trails
    return out


# ---------------------------------------------------------------------------------------------- fixtures
DRAW_KEYS = ("fps_start", "fps_radius", "rad_start", "phys_noise", "state_noise", "rot", "adj_thresh", "knn_thresh")


def load_fixture(name):
    """tests/golden/<name>.npz (make_golden_dataset.py) -> dict: the constructor arguments of a dataset (dataset_config,
    material_config, pair_lists, physics_params, obj_pos, eef_pos), samples, draws (dict of (B, ...) arrays, None where nothing
    was drawn), want (the reference's collated tensors, with recv / send as per-sample lists), trail (per sample, the
    (kNN, topk, n_rel) of every back-off attempt)."""
    import json
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    dcfg = json.loads(bytes(g["dataset_config_json"]).decode())
    mcfg = json.loads(bytes(g["material_config_json"]).decode())
    material = dcfg["materials"][0]
    n = int(g["n_episodes"])
    want = {k[5:]: g[k] for k in g.files if k.startswith("out::")}
    off = np.concatenate([[0], np.cumsum(want["n_edges"])])
    want["recv"] = [want["recv"][off[b]:off[b + 1]] for b in range(len(off) - 1)]
    want["send"] = [want["send"][off[b]:off[b + 1]] for b in range(len(off) - 1)]
    toff = np.concatenate([[0], np.cumsum(g["trail"])])
    trail = [[(float(r[0]), int(r[1]), int(r[2])) for r in g["trail::rows"][toff[b]:toff[b + 1]]] for b in range(len(toff) - 1)]
    return dict(dataset_config=dcfg, material_config=mcfg, pair_lists=g["pair_lists"], material=material,
                physics_params=[{material: g[f"ep{e}::phys"]} for e in range(n)], obj_pos=[g[f"ep{e}::obj"] for e in range(n)],
                eef_pos=[g[f"ep{e}::eef"] for e in range(n)], samples=g["samples"],
                draws={k: (g["draw::" + k] if "draw::" + k in g.files else None) for k in DRAW_KEYS}, want=want, trail=trail)


def dataset_args(fx):
    return (fx["dataset_config"], fx["material_config"], fx["pair_lists"], fx["physics_params"], fx["obj_pos"], fx["eef_pos"])


def rotation_bound(x_ref):
    """Bound on |x' - x'_ref| and |y' - y'_ref| of a rotated row, per component: both sides form a two-term fp32 dot product of
    the row with (c, s); they may differ by a contraction (one rounding of a product, 2^-24 relative to that product) and by one
    ulp of cos / sin (2^-23 relative to each product), and |product| <= |x| + |y| of the rotated row's own length up to a factor
    below sqrt(2): 5e-7 * (|x'| + |y'|) + 1e-9 covers 1.5 * 2^-23 * sqrt(2) = 2.6e-7 twice over."""
    a = np.abs(x_ref[..., 0]) + np.abs(x_ref[..., 1])
    return (5e-7 * a + 1e-9)[..., None]
