"""The array half of the reference's perception step on the device: construct_graph (src/planning/perception.py:259-315) and the
part of get_state_cur that follows pm.get_tabletop_points (perception.py:335-341).

A perceived tabletop cloud has 10^4 - 10^6 points, far above what ag_fps_batch keeps in LDS; ag_fps_cloud samples it from global
memory (include/adaptigraph_amd.h), every object of a scene in ONE launch.  The gather stage1[stage2], the concatenation over
objects and the zero-padded state are formed on the device; one read-back (the per-object counts) sizes obj_state.  Segmentation
and camera I/O are not part of this package: the functions start at the (P, 3) point array.

Every random number is an explicit input (`draws`).  Without it the starts come from numpy's global generator in the reference's
own order - per object np.random.randint(0, n) (perception.py:271), then fps_rad_idx's np.random.randint(n1) (utils.py:14) - so a
caller that seeds numpy as it did for the reference gets the reference's sequence of draws.

What the sampling is pinned on: stage 1 is dgl.geometry.farthest_point_sampler restated from its CPU implementation as remembered
(see dataset.py); dgl is not installed where this project is developed, and perception.construct_graph imports dgl and open3d, so
no fixture could be recorded from the reference's function itself.  The tests compare with a numpy restatement of construct_graph
over that restated sampler.  Two deliberate differences: tensors are float32 (the reference's `state` is a float64 array holding
float32 values), and an object with fewer than max_nobj points is sampled down to all of its points (dgl is not defined there).
"""
from __future__ import annotations

import numpy as np
import torch

from .context import default_engine, ptr, current_stream, _require_gpu
from . import _lib
from .dataset import FPS_MAX_NOBJ

CLOUD_MAX_POINTS = 1 << 20       # ag_fps_cloud's limit on one cloud
CLOUD_WG = 1024                  # threads of its workgroup (one workgroup per cloud)
CLOUD_SWITCH_POINTS = 32768      # running minima of the points behind these live in workspace, not in registers
GRID_MAX_NOBJ = 65536            # ag_fps_cloud_grid's limit on the samples per cloud (its limit on one cloud is CLOUD_MAX_POINTS)
GRID_CELL_POINTS = 64            # its default cell policy: a power-of-two cell count with about this many points per cell,
GRID_MAX_CELLS = 16384           # at most this many cells per cloud


def _check_limits(max_nobj, max_pts, nobj_limit=FPS_MAX_NOBJ):
    if int(max_pts) > CLOUD_MAX_POINTS:
        raise NotImplementedError(f"a cloud of {int(max_pts)} points; the farthest-point sampler takes at most {CLOUD_MAX_POINTS}")
    if int(max_nobj) > nobj_limit:
        raise NotImplementedError(f"max_nobj {int(max_nobj)} exceeds {nobj_limit}")
    if int(max_nobj) < 1 or int(max_pts) < 1:
        raise ValueError(f"max_nobj {int(max_nobj)} and max_pts {int(max_pts)} must be positive")


def _check_limits_grid(max_nobj, max_pts):
    _check_limits(max_nobj, max_pts, GRID_MAX_NOBJ)


def fps_cloud(pos, pt_off, npts, fps_start, fps_radius, rad_start, max_nobj, max_pts, engine=None):
    """ag_fps_cloud: dataset.fps_batch's contract (same arguments, same outputs, bit for bit where both apply) for clouds of up to
    CLOUD_MAX_POINTS points.  NotImplementedError above that or above FPS_MAX_NOBJ samples, before the device is touched."""
    _check_limits(max_nobj, max_pts)
    return _fps_call(None, pos, pt_off, npts, fps_start, fps_radius, rad_start, max_nobj, max_pts, engine)


def fps_cloud_grid(pos, pt_off, npts, fps_start, fps_radius, rad_start, max_nobj, max_pts, cells=None, engine=None):
    """ag_fps_cloud_grid: fps_cloud's contract and outputs for up to GRID_MAX_NOBJ samples per cloud, by exact cell-pruned
    farthest-point sampling: the indices of the brute-force sweep (tests/dataset_restate.py), and fps_cloud's wherever fps_cloud
    gives those (its stage-2 square root is the native one, this one's is correctly rounded: DESIGN.md section 3.27).  cells: None for the default policy (about GRID_CELL_POINTS points per cell, at
    most GRID_MAX_CELLS cells), or a power of two that forces the cell count per cloud - 1 is the brute-force sweep through the same
    code; the outputs do not depend on it.  NotImplementedError above CLOUD_MAX_POINTS points or GRID_MAX_NOBJ samples, ValueError
    for a bad `cells`, before the device is touched."""
    _check_limits_grid(max_nobj, max_pts)
    if cells is not None and (int(cells) < 1 or int(cells) & (int(cells) - 1) or int(cells) > GRID_MAX_CELLS):
        raise ValueError(f"cells {cells} is not None or a power of two up to {GRID_MAX_CELLS}")
    cells = 0 if cells is None else int(cells)
    return _fps_call(cells, pos, pt_off, npts, fps_start, fps_radius, rad_start, max_nobj, max_pts, engine)


def _fps_call(cells, pos, pt_off, npts, fps_start, fps_radius, rad_start, max_nobj, max_pts, engine):
    """The marshalling both samplers share; cells None: ag_fps_cloud, else ag_fps_cloud_grid with that `cells`."""
    dev = _require_gpu(pos.device)
    eng = engine or default_engine(dev)
    B = fps_start.shape[0]
    assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[-1] == 3
    assert pt_off.dtype == torch.int64 and npts.dtype == torch.int64 and pt_off.shape == (B,) and npts.shape == (B,)
    stride = pt_off.stride(0) if B > 1 else 1
    assert B == 1 or npts.stride(0) == stride
    for t, dt in ((fps_start, torch.int32), (fps_radius, torch.float32), (rad_start, torch.int32)):
        assert t.dtype == dt and t.shape == (B,) and t.is_contiguous() and t.device == dev
    fps_idx = torch.empty((B, int(max_nobj)), dtype=torch.int32, device=dev)
    n_obj = torch.empty((B,), dtype=torch.int32, device=dev)
    head = (eng.ctx, current_stream(dev), ptr(pos), ptr(pt_off), ptr(npts), stride, ptr(fps_start), ptr(fps_radius), ptr(rad_start), B,
            int(max_nobj), int(max_pts))
    if cells is None:
        eng.check(eng.lib.ag_fps_cloud(*head, ptr(fps_idx), ptr(n_obj)))
    else:
        eng.check(_lib.load_cells().ag_fps_cloud_grid(*head, cells, ptr(fps_idx), ptr(n_obj)))
    return fps_idx, n_obj


# ------------------------------------------------------------------------------------------------ pure host helpers
def draw_starts(sizes, max_nobj):
    """[(fps_start, rad_start)] per object from numpy's global generator, in the reference's order: per object
    np.random.randint(0, n) (perception.py:271), then fps_rad_idx's np.random.randint(n1) on the n1 = min(max_nobj, n) stage-1
    points (utils.py:14)."""
    out = []
    for n in sizes:
        fps_start = int(np.random.randint(0, n))
        out.append((fps_start, int(np.random.randint(min(int(max_nobj), n)))))
    return out


def graph_layout(counts, n_eef, max_nobj=100, max_neef=8):
    """Where construct_graph puts what (perception.py:282-298).  counts: sampled points per object.  Returns dict(rows = [(first,
    end)] of each object's rows in `state`, obj_kp_num, state_mask, eef_mask - numpy bool (max_nobj + max_neef,)).  ValueError where
    the reference's array assignment fails: more object points than max_nobj, more end-effector points than max_neef."""
    total = int(sum(counts))
    if total > max_nobj:
        raise ValueError(f"the objects' {total} sampled points exceed max_nobj {max_nobj}")
    if n_eef > max_neef:
        raise ValueError(f"{n_eef} end-effector points exceed max_neef {max_neef}")
    ends = np.cumsum([0] + [int(c) for c in counts])
    state_mask = np.zeros(max_nobj + max_neef, bool)
    state_mask[max_nobj:max_nobj + n_eef] = True
    state_mask[:total] = True
    eef_mask = np.zeros(max_nobj + max_neef, bool)
    eef_mask[max_nobj:max_nobj + n_eef] = True
    return dict(rows=[(int(ends[j]), int(ends[j + 1])) for j in range(len(counts))], obj_kp_num=total, state_mask=state_mask,
                eef_mask=eef_mask)


def _check_graph_args(sizes, shapes, n_eef, max_nobj, max_neef, visualize, draws, check_limits=_check_limits):
    """Everything construct_graph can refuse from shapes alone; returns the starts."""
    if visualize:
        raise NotImplementedError("visualize=True needs open3d; draw the returned tensors yourself")
    for s in shapes:
        if len(s) != 2 or s[1] != 3 or s[0] < 1:
            raise ValueError(f"an object's points must be a non-empty (n, 3) array, got shape {tuple(s)}")
    if n_eef > max_neef:
        raise ValueError(f"{n_eef} end-effector points exceed max_neef {max_neef}")
    check_limits(max_nobj, max(sizes))
    if draws is None:
        return draw_starts(sizes, max_nobj)
    draws = [(int(a), int(b)) for a, b in draws]
    if len(draws) != len(sizes):
        raise ValueError(f"{len(draws)} (fps_start, rad_start) pairs for {len(sizes)} objects")
    for (a, b), n in zip(draws, sizes):
        if not (0 <= a < n and 0 <= b < min(max_nobj, n)):
            raise ValueError(f"starts ({a}, {b}) outside an object of {n} points sampled to {min(max_nobj, n)}")
    return draws


def _points_on(x, dev):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)) if isinstance(x, np.ndarray) else torch.as_tensor(x)
    return t.to(dev, torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------ the reference's calls
def construct_graph(obj_kps, fps_radius, max_nobj=100, max_neef=8, max_nR=500, eef_kps=None, visualize=False, *, device, draws=None,
                    engine=None):
    """perception.construct_graph (perception.py:259-315) with its arguments in its order.  obj_kps: an (n, 3) array or a list of
    them, one per object, numpy or torch, on the host or on `device`; eef_kps (m, 3) or None; draws: one (fps_start, rad_start)
    pair per object, or None for numpy's global generator (draw_starts).  max_nR is accepted and unused, as in the reference.

    Returns the reference's dict as float32 tensors on `device` - obj_state (K, 3), obj_state_raw (K, 3), eef_state (m, 3), state
    (max_nobj + max_neef, 3) - plus what the reference computes and drops: state_mask, eef_mask (bool) and fps_idx_list (int32
    indices into each object's points, in selection order).  ValueError / NotImplementedError for everything that can be told from
    the shapes are raised before the device is touched; the objects' sampled points exceeding max_nobj after the one read-back."""
    return _construct_graph(fps_cloud, _check_limits, obj_kps, fps_radius, max_nobj, max_neef, eef_kps, visualize, device, draws, engine)


def construct_graph_grid(obj_kps, fps_radius, max_nobj=100, max_neef=8, max_nR=500, eef_kps=None, visualize=False, *, device,
                         draws=None, engine=None):
    """construct_graph on fps_cloud_grid: the same arguments in the same order, the same returned dict, for any max_nobj up to
    GRID_MAX_NOBJ - the state of a graph for construct_edges_cells / dynamics_cells straight from a cloud."""
    return _construct_graph(fps_cloud_grid, _check_limits_grid, obj_kps, fps_radius, max_nobj, max_neef, eef_kps, visualize, device,
                            draws, engine)


def _construct_graph(sampler, check_limits, obj_kps, fps_radius, max_nobj, max_neef, eef_kps, visualize, device, draws, engine):
    """construct_graph's body over a sampler (fps_cloud's signature) and its limit check."""
    clouds = list(obj_kps) if isinstance(obj_kps, (list, tuple)) else [obj_kps]
    sizes = [int(c.shape[0]) for c in clouds]
    n_eef = 0 if eef_kps is None else int(eef_kps.shape[0])
    starts = _check_graph_args(sizes, [c.shape for c in clouds], n_eef, max_nobj, max_neef, visualize, draws, check_limits)
    dev = _require_gpu(device)
    B = len(clouds)
    pts = [_points_on(c, dev) for c in clouds]
    pos = pts[0] if B == 1 else torch.cat(pts)
    off = np.concatenate([[0], np.cumsum(sizes)])
    table = torch.tensor([off[:-1].tolist(), sizes], dtype=torch.int64).to(dev)            # rows: first point, count
    st = torch.tensor([[a for a, _ in starts], [b for _, b in starts]], dtype=torch.int32).to(dev)
    radius = torch.full((B,), float(fps_radius), dtype=torch.float32, device=dev)
    fps_idx, n_obj = sampler(pos, table[0], table[1], st[0], radius, st[1], max_nobj, max(sizes), engine=engine)
    counts = n_obj.cpu().tolist()                                                        # the one read-back
    lay = graph_layout(counts, n_eef, max_nobj, max_neef)
    fps_idx_list = [fps_idx[j, :counts[j]] for j in range(B)]
    rows = torch.cat([fps_idx_list[j].to(torch.int64) + int(off[j]) for j in range(B)])
    obj_state = pos.index_select(0, rows)
    eef_state = torch.zeros((0, 3), dtype=torch.float32, device=dev) if eef_kps is None else _points_on(eef_kps, dev)
    state = torch.zeros((max_nobj + max_neef, 3), dtype=torch.float32, device=dev)
    state[:lay["obj_kp_num"]] = obj_state
    state[max_nobj:max_nobj + n_eef] = eef_state
    return dict(obj_state=obj_state, obj_state_raw=obj_state[:lay["obj_kp_num"]], eef_state=eef_state, state=state,
                state_mask=torch.from_numpy(lay["state_mask"]).to(dev), eef_mask=torch.from_numpy(lay["eef_mask"]).to(dev),
                fps_idx_list=fps_idx_list)


def state_cur_from_points(points, sim_real_ratio, fps_radius=0.2, *, device, draws=None, engine=None):
    """get_state_cur from pm.get_tabletop_points' array on (perception.py:335-341): points (P, 3) in camera-world metres, times
    sim_real_ratio in fp32, (x, y, z) -> (x, -z, y), construct_graph with its defaults.  Returns (state_cur = obj_state_raw,
    float32 (K, 3) on `device`; the transformed cloud, float32 (P, 3) on `device`).  The elementwise part is plain torch: it runs
    once per MPC iteration."""
    return _state_cur(fps_cloud, _check_limits, points, sim_real_ratio, fps_radius, 100, device, draws, engine)


def state_cur_from_points_grid(points, sim_real_ratio, fps_radius=0.2, max_nobj=100, *, device, draws=None, engine=None):
    """state_cur_from_points on fps_cloud_grid, for any max_nobj up to GRID_MAX_NOBJ (the reference's get_state_cur never passes
    max_nobj, so here it is a keyword)."""
    return _state_cur(fps_cloud_grid, _check_limits_grid, points, sim_real_ratio, fps_radius, max_nobj, device, draws, engine)


def _state_cur(sampler, check_limits, points, sim_real_ratio, fps_radius, max_nobj, device, draws, engine):
    if len(points.shape) != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"points must be a non-empty (P, 3) array, got shape {tuple(points.shape)}")
    check_limits(max_nobj, points.shape[0])
    dev = _require_gpu(device)
    p = _points_on(points, dev) * torch.tensor(float(sim_real_ratio), dtype=torch.float32, device=dev)
    obj_kps = torch.stack([p[:, 0], -p[:, 2], p[:, 1]], 1).contiguous()
    graph = _construct_graph(sampler, check_limits, obj_kps, fps_radius, max_nobj, 8, None, False, dev, draws, engine)
    return graph["obj_state_raw"], obj_kps
