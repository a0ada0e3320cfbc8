"""DeviceDynDataset: the reference's training samples (src/dynamics/dataset/dataset.py:117-383, DynDataset.__getitem__) built a
batch at a time on the GPU.

A batch is three launches on flat, unpadded episode buffers that were uploaded once - ag_fps_batch (both farthest-point stages),
ag_dataset_assemble (every dense tensor, padding and augmentation included), ag_build_edges_graphs (B single-graph edge builds) -
and ONE read-back of the B edge counts for the max_nR back-off.  Configs with the tool-to-non-fixed rule (softbody) add one
launch, ag_edges_nonfixed_rule_graphs, on the B base graphs.  Every config backs off the same way (graph.attempt_with_backoff):
in rounds over the sub-batch that is still over max_nR, one read-back per round.  The dict that comes out goes unchanged into
TrainStep.step(data, max_edges=data['max_edges']), evaluate, accumulate and DynamicsPredictor(**data).

Every random number of a batch is an explicit input (BatchDraws): a batch is a pure function of (idx, draws).  The default draws
come from a torch.Generator; numpy's global stream, which the reference consumes, is not reproduced.

Two deliberate differences from the reference:
  * physics noise is added to a COPY of the stored parameter.  The reference adds it in place (dataset.py:261-266), so its
    stored parameters drift call by call; that is not reproduced.
  * farthest-point stage 1 is dgl.geometry.farthest_point_sampler restated from its CPU implementation as remembered (running
    minimum of the fp32 squared distance initialised to 1e10, strict-greater argmax, so the lowest index wins ties).  dgl was not
    available to verify this against; include/adaptigraph_amd.h (ag_fps_batch) is the specification.
Positions are kept in fp32: float64 arrays are rounded on upload (the reference would difference float64 tool positions in
double before its own rounding).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .context import default_engine, ptr, current_stream, _require_gpu
from .graph import (EdgeList, BackoffPlan, RuleConfig, attempt_with_backoff, construct_edges_graphs, construct_edges_with_backoff,
                    rule_graphs_limit, surface_graphs_limit)
from .rollout import surface_bounds

FPS_MAX_POINTS = 8192        # ag_fps_batch keeps a cloud in LDS (96 KB of the CU's 160 KB at this size)
FPS_MAX_NOBJ = 1024
EDGE_MAX_PARTICLES = 4096    # the LDS-resident edge builder's limit on max_nobj + n_eef


@dataclass
class DatasetSpec:
    """The keys dataset.py:26-66 reads, for one phase.  Pure host object."""
    n_his: int
    n_future: int
    store_rest_state: bool
    add_randomness: bool
    state_noise: float
    phys_noise: float
    max_nobj: int
    fps_radius_range: object
    max_nR: int
    adj_radius_range: tuple
    topk: int
    knn_range: tuple
    min_kNN: float
    knn_increment: float
    connect_tool_all: bool
    connect_tool_all_non_fixed: bool
    connect_tool_surface: bool
    connect_tool_surface_ratio: float
    material: str
    n_mat: int
    mat_col: int

    @property
    def batched_edges(self):
        """No tool rule and no kNN range (rope, cloth, granular, bunnybath, multiobj).  Every config builds its graphs through
        DeviceDynDataset._edges_batch; this selects what such a config is spared there: the kNN draws are not read back (the
        trails report 1.0), the rules' bounds source is not gathered, and per_sample_edges has nothing to switch to."""
        return not self.connect_tool_all_non_fixed and not self.connect_tool_surface and self.min_kNN >= 1.0


def parse_config(dataset_config, material_config, phase="train"):
    """dataset.py:18-66 without the loading.  Keys the upstream configs lack default to off / 1.0 / 0.1."""
    assert phase in ["train", "valid"]
    obj_config = dataset_config["datasets"]
    assert len(obj_config) == 1, "Only one object type is supported."                       # dataset.py:38
    assert len(dataset_config["materials"]) == 1, "only support single material"            # dataset.py:270
    d = obj_config[0]
    material = dataset_config["materials"][0]
    rnd = dataset_config["randomness"]
    fr = d["fps_radius_range"]
    if not isinstance(fr, float) and len(fr) != 2:
        raise ValueError(f"Invalid fps_radius_range: {fr}.")                                # graph.py:24
    if (fr if isinstance(fr, float) else min(fr)) < 0:
        raise ValueError(f"fps_radius_range {fr}: a negative radius never ends stage 2 (utils.py:18)")
    return DatasetSpec(
        n_his=int(dataset_config["n_his"]), n_future=int(dataset_config["n_future"]),
        store_rest_state=bool(dataset_config.get("store_rest_state", False)),
        add_randomness=bool(rnd["use"]), state_noise=float(rnd["state_noise"][phase]), phys_noise=float(rnd["phys_noise"][phase]),
        max_nobj=int(d["max_nobj"]), fps_radius_range=fr if isinstance(fr, float) else (float(fr[0]), float(fr[1])),
        max_nR=int(d["max_nR"]), adj_radius_range=(float(d["adj_radius_range"][0]), float(d["adj_radius_range"][1])),
        topk=int(d["topk"]), knn_range=tuple(float(v) for v in d.get("knn_range", (1.0, 1.0))),
        min_kNN=float(d.get("min_knn", 1.0)), knn_increment=float(d.get("knn_increment", 0.1)),
        connect_tool_all=bool(d["connect_tool_all"]), connect_tool_all_non_fixed=bool(d.get("connect_tool_all_non_fixed", False)),
        connect_tool_surface=bool(d.get("connect_tool_surface", False)),
        connect_tool_surface_ratio=float(d.get("connect_tool_surface_ratio", 1.0)),
        material=material, n_mat=len(material_config["material_index"]), mat_col=int(material_config["material_index"][material]))


def frame_table(spec, pair_lists):
    """(T_pairs, 1 + n_frames) pair list -> (T_pairs, n_his + n_future) frame indices.  A short pair under store_rest_state gets
    the rest frame (episode frame 0) in front (dataset.py:121-144); any other length is the reference's AssertionError."""
    pairs = np.asarray(pair_lists).astype(np.int64)
    if pairs.ndim != 2 or pairs.shape[0] < 1:
        raise ValueError(f"pair_lists must be (T, 1 + n_frames), got {pairs.shape}")
    n = pairs.shape[1] - 1
    T = spec.n_his + spec.n_future
    if n == T:
        return pairs[:, 1:].copy()
    assert spec.store_rest_state and n == T - 1, \
        f"a pair of {n} frames: expected n_his + n_future = {T}" + (f" or {T - 1} with the rest state" if spec.store_rest_state else "")
    return np.concatenate([np.zeros((pairs.shape[0], 1), np.int64), pairs[:, 1:]], 1)


def plane_bounds(obj_kp_padded, ratio):
    """The four bounds dataset.py:186-209, 310-314 hands the edge builder (min_x / min_z are computed there but not passed on):
    rollout.surface_bounds on the PADDED (max_nobj, 3) history frame n_his - 1, zero rows included as in the reference."""
    b = surface_bounds(np.asarray(obj_kp_padded, np.float32), ratio)
    return {k: b[k] for k in ("max_y", "min_y", "max_x", "max_z")}


def start_graph_bounds(obj_kp_padded, ratio):
    """The six bounds the eval script's construct_graph hands the edge builder (rollout/graph.py:446-458, 508-512), on the PADDED
    (max_nobj, 3) history frame n_his - 1, written as the reference writes them on numpy float32 scalars: min_x / min_z are formed
    from the UNSCALED maxima, then the maxima are scaled (rollout.surface_bounds scales first; the two agree at ratio 1)."""
    kp = np.asarray(obj_kp_padded, np.float32)
    max_y, min_y = np.max(kp[:, 1]), np.min(kp[:, 1])
    max_x, max_z = np.max(kp[:, 0]), np.max(kp[:, 2])
    min_x, min_z = np.min(kp[:, 0]), np.min(kp[:, 2])
    min_x = (max_x - min_x) * (1 - ratio) + min_x
    min_z = (max_z - min_z) * (1 - ratio) + min_z
    max_y = max_y * ratio
    max_x = max_x * ratio
    max_z = max_z * ratio
    return dict(max_y=max_y, min_y=min_y, max_x=max_x, max_z=max_z, min_x=min_x, min_z=min_z)


def fps_batch(pos, pt_off, npts, fps_start, fps_radius, rad_start, max_nobj, max_pts, engine=None):
    """ag_fps_batch: both farthest-point stages (graph.py:8-36) of B clouds.  pos: flat (P, 3) fp32 points on the GPU; cloud b is
    the npts[b] points from point pt_off[b] on (int64 vectors of one common stride, e.g. two columns of a table); fps_start /
    rad_start int32, fps_radius fp32, (B,) each; max_pts: the caller's bound on npts.  Returns (fps_idx (B, max_nobj) int32 in
    selection order, -1 behind the first n_obj[b] entries; n_obj (B,) int32).  NotImplementedError above FPS_MAX_POINTS points or
    FPS_MAX_NOBJ samples, before anything is enqueued."""
    dev = _require_gpu(pos.device)
    eng = engine or default_engine(dev)
    if int(max_pts) > FPS_MAX_POINTS:
        raise NotImplementedError(f"a cloud of {int(max_pts)} points; the LDS-resident farthest-point sampler takes at most {FPS_MAX_POINTS}")
    if int(max_nobj) > FPS_MAX_NOBJ:
        raise NotImplementedError(f"max_nobj {int(max_nobj)} exceeds {FPS_MAX_NOBJ}")
    B = fps_start.shape[0]
    assert pos.dtype == torch.float32 and pos.is_contiguous() and pos.shape[-1] == 3
    assert pt_off.dtype == torch.int64 and npts.dtype == torch.int64 and pt_off.shape == (B,) and npts.shape == (B,)
    stride = pt_off.stride(0) if B > 1 else 1
    assert B == 1 or npts.stride(0) == stride
    for t, dt in ((fps_start, torch.int32), (fps_radius, torch.float32), (rad_start, torch.int32)):
        assert t.dtype == dt and t.shape == (B,) and t.is_contiguous() and t.device == dev
    fps_idx = torch.empty((B, int(max_nobj)), dtype=torch.int32, device=dev)
    n_obj = torch.empty((B,), dtype=torch.int32, device=dev)
    eng.check(eng.lib.ag_fps_batch(eng.ctx, current_stream(dev), ptr(pos), ptr(pt_off), ptr(npts), stride, ptr(fps_start),
                                   ptr(fps_radius), ptr(rad_start), B, int(max_nobj), int(max_pts), ptr(fps_idx), ptr(n_obj)))
    return fps_idx, n_obj


@dataclass
class BatchDraws:
    """Every random number of one batch, in the order __getitem__ draws them (graph.py:12, 22, utils.py:14, dataset.py:265, 275,
    277, 304, 306).  B rows each."""
    fps_start: torch.Tensor            # int32, in [0, N_e)
    fps_radius: torch.Tensor           # float32
    rad_start: torch.Tensor            # int32, in [0, min(max_nobj, N_e))
    phys_noise: torch.Tensor           # float64 (B, phys_dim)
    state_noise: torch.Tensor | None   # float64 (B, n_his, N, 3)
    rot: torch.Tensor | None           # float64 angle
    adj_thresh: torch.Tensor           # float64
    knn_thresh: torch.Tensor           # float64


class DeviceDynDataset:
    """ds = DeviceDynDataset(dataset_config, material_config, pair_lists, physics_params, obj_pos, eef_pos, device);
    data = ds.batch(idx); loss = train_step.step(data, max_edges=data['max_edges']).

    pair_lists (T, 1 + n_frames): episode index, then frame indices; physics_params: list of {material: array}; obj_pos: list of
    (T_e, N_e, 3) arrays, ragged over episodes; eef_pos: list of (T_e, N_eef, 3) - what the reference's load_dataset /
    load_positions return.  Positions are uploaded once as flat buffers with per-episode offsets, not padded to the largest
    episode.  Every argument error is raised on the host before the device is touched."""

    def __init__(self, dataset_config, material_config, pair_lists, physics_params, obj_pos, eef_pos, device, phase="train"):
        sp = self.spec = parse_config(dataset_config, material_config, phase)
        self.phase = phase
        self._frames = frame_table(sp, pair_lists)
        self._episode = np.asarray(pair_lists).astype(np.int64)[:, 0].copy()
        n_epis = len(obj_pos)
        if n_epis < 1 or len(eef_pos) != n_epis or len(physics_params) < n_epis:
            raise ValueError(f"{n_epis} object episodes, {len(eef_pos)} end-effector episodes, {len(physics_params)} physics entries")
        shapes = [np.shape(o) for o in obj_pos]
        eshapes = [np.shape(e) for e in eef_pos]
        for e, (so, se) in enumerate(zip(shapes, eshapes)):
            if len(so) != 3 or so[2] != 3 or len(se) != 3 or se[2] != 3 or so[0] != se[0] or so[1] < 1:
                raise ValueError(f"episode {e}: obj_pos {so}, eef_pos {se}")
        self.n_eef = int(eshapes[0][1])                                                      # dataset.py:87
        if any(se[1] != self.n_eef for se in eshapes):
            raise NotImplementedError("episodes with different end-effector point counts")
        self._t_e = np.array([s[0] for s in shapes], np.int64)
        self._n_e = np.array([s[1] for s in shapes], np.int64)
        self.N = sp.max_nobj + self.n_eef
        if int(self._n_e.max()) > FPS_MAX_POINTS:
            raise NotImplementedError(f"an episode has {int(self._n_e.max())} object points; the LDS-resident farthest-point "
                                      f"sampler takes at most {FPS_MAX_POINTS}")
        if sp.max_nobj > FPS_MAX_NOBJ or self.N > EDGE_MAX_PARTICLES:
            raise NotImplementedError(f"max_nobj {sp.max_nobj} (limit {FPS_MAX_NOBJ}), max_nobj + n_eef {self.N} (limit {EDGE_MAX_PARTICLES})")
        if self._episode.min() < 0 or self._episode.max() >= n_epis:
            raise ValueError("pair_lists names an episode that is not there")
        if self._frames.min() < 0 or (self._frames >= self._t_e[self._episode][:, None]).any():
            raise ValueError("pair_lists names a frame beyond its episode")
        self.materials = {k: int(np.shape(v)[0]) for k, v in physics_params[0].items()}     # dataset.py:75-77
        for e in range(n_epis):
            if sp.material not in physics_params[e]:
                raise ValueError(f"Physics parameter {sp.material} not found in episode {e}")  # dataset.py:263-264
        self.phys_dim = self.materials[sp.material]
        self._obj_off = np.concatenate([[0], np.cumsum(self._t_e * self._n_e)[:-1]]).astype(np.int64)
        self._eef_off = np.concatenate([[0], np.cumsum(self._t_e * self.n_eef)[:-1]]).astype(np.int64)
        self._obj_host = obj_pos                                                             # the per-sample edge path's plane bounds
        # ---- the device from here on
        dev = _require_gpu(device)
        dev = self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.engine = default_engine(dev)
        flat = np.concatenate([np.asarray(o, np.float32).reshape(-1, 3) for o in obj_pos], 0)
        self._obj = torch.from_numpy(flat).to(dev)
        flat = np.concatenate([np.asarray(e, np.float32).reshape(-1, 3) for e in eef_pos] + [np.zeros((1, 3), np.float32)], 0)
        self._eef = torch.from_numpy(flat).to(dev)
        phys = np.stack([np.asarray(physics_params[e][sp.material], np.float64).reshape(-1) for e in range(n_epis)], 0)
        self._phys = torch.from_numpy(phys).to(dev)
        self._side = None
        self.last_trail = None
        self.last_waits = None               # read-backs of the last batch(): 1 + back-off rounds (None: the per-sample path)
        self._warned_rule_limit = False

    def __len__(self):
        return len(self._episode)

    # ------------------------------------------------------------------------------------------ draws
    def draws(self, idx, generator=None):
        """The random numbers of the batch `idx` as tensors on the dataset's device.  generator: a torch.Generator on the device or
        on the CPU (None: the device's default generator)."""
        sp, dev = self.spec, self.device
        idx = np.asarray(idx, np.int64).reshape(-1)
        B = len(idx)
        gdev = generator.device if generator is not None else dev
        n_e = torch.from_numpy(self._n_e[self._episode[idx]]).to(gdev)

        def u(*shape):
            return torch.rand(*shape, dtype=torch.float64, device=gdev, generator=generator)

        def uniform(lo, hi, *shape):
            return lo + (hi - lo) * u(*shape)

        def below(n):
            return torch.minimum((u(B) * n).floor().to(torch.int64), n - 1).to(torch.int32)

        fps_start = below(n_e)
        fr = sp.fps_radius_range
        fps_radius = (torch.full((B,), fr, dtype=torch.float64, device=gdev) if isinstance(fr, float) else uniform(fr[0], fr[1], B)).float()
        rad_start = below(torch.clamp(n_e, max=sp.max_nobj))
        phys_noise = uniform(-sp.phys_noise, sp.phys_noise, B, self.phys_dim)
        state_noise = rot = None
        if sp.add_randomness:
            state_noise = uniform(-sp.state_noise, sp.state_noise, B, sp.n_his, self.N, 3)
            rot = uniform(-math.pi, math.pi, B)
        adj = uniform(sp.adj_radius_range[0], sp.adj_radius_range[1], B)
        knn = uniform(sp.knn_range[0], sp.knn_range[1], B) if sp.min_kNN < 1.0 else torch.ones(B, dtype=torch.float64, device=gdev)
        mv = (lambda t: None if t is None else t.to(dev))
        return BatchDraws(mv(fps_start), mv(fps_radius), mv(rad_start), mv(phys_noise), mv(state_noise), mv(rot), mv(adj), mv(knn))

    def eval_draws(self, idx, fps_start=None, rad_start=None):
        """The BatchDraws of the eval rollout's construct_graph (rollout/graph.py:353-356): fps radius, adj threshold and kNN at
        the MIDPOINT of their ranges, zero physics noise, no state noise, no rotation.  fps_start / rad_start: the two
        farthest-point start indices, (B,) or one integer, default 0 (the reference draws them from numpy's global stream)."""
        sp, dev = self.spec, self.device
        B = len(np.asarray(idx).reshape(-1))
        fr = sp.fps_radius_range
        rad = fr if isinstance(fr, float) else (fr[0] + fr[1]) / 2
        adj = (sp.adj_radius_range[0] + sp.adj_radius_range[1]) / 2
        knn = (sp.knn_range[0] + sp.knn_range[1]) / 2

        def start(v):
            v = np.zeros(B, np.int32) if v is None else np.broadcast_to(np.asarray(v, np.int32), (B,)).copy()
            return torch.from_numpy(v).to(dev)

        full = (lambda v, dt: torch.full((B,), v, dtype=dt, device=dev))
        return BatchDraws(start(fps_start), full(float(np.float32(rad)), torch.float32), start(rad_start),
                          torch.zeros((B, self.phys_dim), dtype=torch.float64, device=dev), None, None,
                          full(adj, torch.float64), full(knn, torch.float64))

    # ------------------------------------------------------------------------------------------ one batch
    def _sample_table(self, idx):
        """(B, 5 + T) int64, ag_dataset_batch::d_sample: [first point of the sampled cloud, N_e, first object point of the episode,
        first end-effector point of the episode, episode, frames]."""
        sp = self.spec
        ep = self._episode[idx]
        fr = self._frames[idx]
        n_e = self._n_e[ep]
        tab = np.empty((len(idx), 5 + fr.shape[1]), np.int64)
        tab[:, 0] = self._obj_off[ep] + fr[:, sp.n_his - 1] * n_e                            # dataset.py:165
        tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 4] = n_e, self._obj_off[ep], self._eef_off[ep], ep
        tab[:, 5:] = fr
        return tab

    def _fps(self, tab, dr):
        return fps_batch(self._obj, tab[:, 0], tab[:, 1], dr.fps_start, dr.fps_radius, dr.rad_start, self.spec.max_nobj,
                         int(self._n_e.max()), engine=self.engine)

    def batch(self, idx, draws=None, generator=None, dense=False, with_fps=False, per_sample_edges=False, _eval_start=False):
        """The collated batch of the samples `idx` (a sequence of pair indices): state, action, eef_future, action_future,
        state_future, attrs, p_rigid, p_instance, obj_mask, material_index, <material>_physics_param as the reference's DataLoader
        collates them, plus edges (an EdgeList over the B graphs, every graph within max_nR) and max_edges (= max_nR).
        dense=True adds Rr / Rs, zero-padded to max_nR.  draws: a BatchDraws (default: self.draws(idx, generator)).
        with_fps=True adds fps_idx (B, max_nobj) int32 (-1 behind the first n_obj[b] entries) and n_obj (B,) int32.
        Waits once, on the current stream, for the B edge counts, and once more per back-off round (last_waits).
        per_sample_edges=True: configs with a tool rule or a kNN range build their graphs sample by sample through
        construct_edges_with_backoff, with several waits per sample - the A/B partner of the batched rule path, and what a config
        beyond ag_edges_nonfixed_rule_graphs' size limit falls back to (with one warning).
        _eval_start (private, rollout_eval_batch's): with connect_tool_surface the graphs get the eval script's own rule - both tool
        rules with construct_graph's six bounds (rollout/graph.py:446-458, 508-512) - where this, the training path, never passes
        min_x / min_z on and so never fires the surface rule (dataset.py:310-314).  Every other config: no effect."""
        sp, dev, eng = self.spec, self.device, self.engine
        idx = np.asarray(idx, np.int64).reshape(-1)
        if len(idx) < 1 or idx.min() < 0 or idx.max() >= len(self):
            raise IndexError(f"batch indices outside [0, {len(self)})")
        dr = draws if draws is not None else self.draws(idx, generator)
        B, N, No, nh, nf = len(idx), self.N, sp.max_nobj, sp.n_his, sp.n_future
        tab = torch.from_numpy(self._sample_table(idx)).to(dev)
        fps_idx, n_obj = self._fps(tab, dr)
        f32 = dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        out = dict(state=torch.empty((B, nh, N, 3), **f32), action=torch.empty((B, N, 3), **f32),
                   eef_future=torch.empty((B, nf - 1, N, 3), **f32), action_future=torch.empty((B, nf - 1, N, 3), **f32),
                   state_future=torch.empty((B, nf, No, 3), **f32), attrs=torch.empty((B, N, 2), **f32),
                   p_rigid=torch.zeros((B, 1), **f32), p_instance=torch.empty((B, No, 1), **f32))
        obj_mask, state_mask, eef_mask = torch.empty((B, No), **u8), torch.empty((B, N), **u8), torch.empty((B, N), **u8)
        material_index = torch.empty((B, No, sp.n_mat), dtype=torch.int64, device=dev)
        phys = torch.empty((B, self.phys_dim), **f32)
        thr2, cull = torch.empty((B,), **f32), torch.empty((B,), **f32)
        for t, shape in ((dr.phys_noise, (B, self.phys_dim)), (dr.state_noise, (B, nh, N, 3)), (dr.rot, (B,)), (dr.adj_thresh, (B,))):
            assert t is None or (t.dtype == torch.float64 and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev)
        a = _lib.AgDatasetBatch()
        for name, t in (("d_obj_pos", self._obj), ("d_eef_pos", self._eef), ("d_sample", tab), ("d_fps_idx", fps_idx), ("d_n_obj", n_obj),
                        ("d_phys", self._phys), ("d_phys_noise", dr.phys_noise), ("d_state_noise", dr.state_noise), ("d_rot", dr.rot),
                        ("d_adj_thresh", dr.adj_thresh), ("d_state", out["state"]), ("d_action", out["action"]),
                        ("d_eef_future", out["eef_future"]), ("d_action_future", out["action_future"]),
                        ("d_state_future", out["state_future"]), ("d_attrs", out["attrs"]), ("d_p_instance", out["p_instance"]),
                        ("d_obj_mask", obj_mask), ("d_state_mask", state_mask), ("d_eef_mask", eef_mask),
                        ("d_material_index", material_index), ("d_physics_param", phys), ("d_thr2", thr2), ("d_cull", cull)):
            setattr(a, name, t.data_ptr() if t is not None and t.numel() else None)
        a.B, a.n_his, a.n_future, a.max_nobj, a.n_eef = B, nh, nf, No, self.n_eef
        a.phys_dim, a.n_mat, a.mat_col = self.phys_dim, sp.n_mat, sp.mat_col
        eng.check(eng.lib.ag_dataset_assemble(eng.ctx, current_stream(dev), C.byref(a)))
        out["obj_mask"] = obj_mask.view(torch.bool)
        out["material_index"] = material_index
        for name, dim in self.materials.items():                                             # dataset.py:377-381
            out[name + "_physics_param"] = phys if name == sp.material else torch.zeros((B, dim), **f32)
        surface = bool(_eval_start and sp.connect_tool_surface)
        limit = rule_graphs_limit(N, self.n_eef) if sp.connect_tool_all_non_fixed else None
        if surface and limit is None:
            limit = surface_graphs_limit(N, self.n_eef)
        if limit is not None and not sp.batched_edges and not per_sample_edges:
            if not self._warned_rule_limit:
                import warnings
                warnings.warn(f"DeviceDynDataset: {limit}; the graphs of this config are built sample by sample", RuntimeWarning)
                self._warned_rule_limit = True
            per_sample_edges = True
        if per_sample_edges and not sp.batched_edges:
            edges, trail = self._edges_per_sample(idx, out["state"], state_mask, eef_mask, fps_idx, n_obj, dr, eval_start=surface)
            self.last_waits = None
        else:
            edges, trail = self._edges_batch(out["state"], state_mask, eef_mask, thr2, cull, tab, fps_idx, n_obj, dr,
                                             self._rule_config(surface, 1))
        self.last_trail = trail
        self._last_build = dict(state_mask=state_mask, eef_mask=eef_mask, thr2=thr2, cull=cull)   # rollout_eval_batch reads them
        out["edges"] = edges
        out["max_edges"] = sp.max_nR
        if dense:
            out["Rr"], out["Rs"] = edges.to_dense(sp.max_nR)
        if with_fps:
            out["fps_idx"], out["n_obj"] = fps_idx, n_obj
        return out

    # ------------------------------------------------------------------------------------------ edges
    def _edges_batch(self, state, mask, tool, thr2, cull, tab, fps_idx, n_obj, dr, cfg):
        """The one batched build (graph.attempt_with_backoff): all B base graphs at top-k in one launch, the
        config's rule launches on them (cfg, a RuleConfig; none for a config with neither rule), ONE read-back of the counts, then
        graph.BackoffPlan's rounds over the sub-batch that is still over max_nR, one read-back per round (dataset.py:317-349).
        With a rule the base graphs go into buffers of the structural bound (a rule removes edges as well as adding them, so
        max_nR is no capacity for its input) and the result into max_nR-wide ones; without, the base graphs are the result.  The
        bounds of the rules are the un-augmented rows of frame n_his - 1, padding zeros included (dataset.py:186-209).  The
        training path never passes min_x / min_z on (dataset.py:310-314), so connect_tool_surface fires only where cfg says so:
        the eval rollout's start graphs chain the surface rule behind the non-fixed one on the same bounds rows.  Without
        spec.batched_edges the kNN draws come back with the counts (a kNN range without the rule too: its trail reports them)."""
        sp, N, nh = self.spec, self.N, self.spec.n_his
        B, cap, ruled = mask.shape[0], max(1, sp.max_nR), cfg.rule or cfg.surface
        k = min(N, sp.topk)
        base_cap = max(1, N * (k + self.n_eef) if k < N else N * N) if ruled else cap
        last = state.data_ptr() + (nh - 1) * N * 3 * 4                                       # state[:, -1] in place
        bnd = (self._obj, tab[:, 0].contiguous(), fps_idx, n_obj, sp.max_nobj) if ruled else None
        base = construct_edges_graphs(last, nh * N * 3, mask, tool, thr2, cull, sp.topk, sp.connect_tool_all, edge_cap=base_cap,
                                      engine=self.engine)
        plan = BackoffPlan([1.0] * B, sp.topk, sp.max_nR, sp.min_kNN, sp.knn_increment, has_rule=cfg.rule)
        el = attempt_with_backoff(cfg, plan, last, nh * N * 3, base, dr.knn_thresh, state[:, -1], mask, tool, thr2, cull, bnd, cap,
                                  read_knn=not sp.batched_edges)
        self.last_waits = plan.rounds
        return el, plan.trail

    def _rule_config(self, surface=False, bounds_order=0):
        """The training path's RuleConfig; surface=True: the eval rollout's, with the surface rule chained on (bounds_order 1 for the
        start graphs, 0 inside the step loop)."""
        sp = self.spec
        return RuleConfig(sp.connect_tool_all_non_fixed, self.n_eef, sp.connect_tool_surface_ratio, sp.connect_tool_all, self.engine,
                          surface=bool(surface), bounds_order=int(bounds_order))

    def _edges_per_sample(self, idx, state, mask, tool, fps_idx, n_obj, dr, eval_start=False):
        """Configs with a tool rule or a kNN range: sample by sample through construct_edges_with_backoff, stitched into one
        EdgeList.  Correct and slow (several waits per sample).  eval_start: construct_graph's six bounds instead of the training
        path's four (the eval rollout's start graphs beyond the batched rules' size limits)."""
        sp, dev, N = self.spec, self.device, self.N
        B, cap = len(idx), max(1, sp.max_nR)
        recv = torch.zeros((B, cap), dtype=torch.int32, device=dev)
        send = torch.zeros((B, cap), dtype=torch.int32, device=dev)
        row_ptr = torch.empty((B, N + 1), dtype=torch.int32, device=dev)
        n_edges = torch.empty((B,), dtype=torch.int32, device=dev)
        h_idx, h_n = fps_idx.cpu().numpy(), n_obj.cpu().numpy()
        adj, knn = dr.adj_thresh.cpu().numpy(), dr.knn_thresh.cpu().numpy()
        trails = []
        for b, i in enumerate(idx):
            ep = int(self._episode[i])
            kp = np.zeros((sp.max_nobj, 3), np.float32)                                      # dataset.py:171-172, frame n_his - 1
            kp[:h_n[b]] = np.asarray(self._obj_host[ep][self._frames[i, sp.n_his - 1]], np.float32)[h_idx[b, :h_n[b]]]
            trail = []
            el = construct_edges_with_backoff(state[b, -1], float(adj[b]), mask[b].view(torch.bool), tool[b].view(torch.bool), sp.topk,
                                              sp.max_nR, knn_thresh=float(knn[b]), min_kNN=sp.min_kNN, knn_increment=sp.knn_increment,
                                              as_index=True, trail=trail, connect_tools_all=sp.connect_tool_all,
                                              connect_tools_surface=sp.connect_tool_surface,
                                              connect_tool_all_non_fixed=sp.connect_tool_all_non_fixed,
                                              **(start_graph_bounds if eval_start else plane_bounds)(kp, sp.connect_tool_surface_ratio))
            n = trail[-1][2]
            recv[b, :n], send[b, :n] = el.recv[0, :n], el.send[0, :n]
            row_ptr[b], n_edges[b] = el.row_ptr[0], el.n_edges[0]
            trails.append(trail)
        return EdgeList(recv, send, row_ptr, n_edges, N), trails

    # ------------------------------------------------------------------------------------------ loader
    def _order(self, batch_size, shuffle, generator):
        """Endless batches of pair indices (utils.py:136-142 over a DataLoader).  A device generator's permutation is drawn on
        the stream that is current when the next batch is ASKED for and read back there: the loader asks under its side stream."""
        n = len(self)
        while True:
            if shuffle:
                g = generator
                perm = torch.randperm(n, generator=g, device=g.device if g is not None else "cpu").cpu().numpy()
            else:
                perm = np.arange(n)
            for s in range(0, n, batch_size):
                yield perm[s:s + batch_size]

    def loader(self, batch_size, shuffle, generator=None, prefetch=True):
        """An endless iterator over batches, like the reference's dataloader_wrapper over a DataLoader (the last batch of an
        epoch may be short).  prefetch: batch k+1 is built on a side stream of the dataset's own while the caller works on
        batch k; the hand-over is an event the caller's current stream waits for on the DEVICE - the caller's stream never waits
        for the host.  (The host thread does wait, on the side stream only, for each batch's edge counts and - with a device generator and shuffle - for the
        epoch's permutation; without prefetch both waits are on the caller's stream.)  The batches are the same
        with and without prefetch for the same generator."""
        order = self._order(int(batch_size), bool(shuffle), generator)
        if not prefetch:
            for idx in order:
                yield self.batch(idx, generator=generator)
            return
        dev = self.device
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        side = self._side

        side.wait_stream(torch.cuda.current_stream(dev))                                     # the episode buffers' upload

        def build():
            with torch.cuda.stream(side):                                                    # the epoch's permutation too
                data = self.batch(next(order), generator=generator)
                ev = torch.cuda.Event()
                ev.record(side)
            return data, ev

        nxt = build()
        while True:
            data, ev = nxt
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(ev)
            for t in _tensors(data):
                t.record_stream(cur)
            yield data
            nxt = build()                      # while the caller's stream runs what it enqueued on batch k


def _tensors(data):
    for v in data.values():
        if torch.is_tensor(v):
            yield v
        elif isinstance(v, EdgeList):
            yield from (v.recv, v.send, v.row_ptr, v.n_edges)
