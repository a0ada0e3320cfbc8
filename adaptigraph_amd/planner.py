"""`Planner` behind the reference's class interface (src/planning/real_world/planner.py:38-323): MPPI, and a CMA-ES search.

Same config dictionary, same methods, same result dictionaries: plan.py:177-247 and random_interact.py:168-214 can
construct it and call `trajectory_optimization` / `merge_res` unchanged.  The class is host logic around the two
callables of the config (`model_rollout_fn` = forward_dynamics.dynamics, `evaluate_traj_fn` = running_cost): it owns no
arithmetic of the hot path.  What is new:

* `trajectory_optimization_chunked(state_cur, act_seq, n_chunk)` = the caller's loop
      for ci in range(n_chunk): res_all.append(planner.trajectory_optimization(state_cur, act_seq))
      res = planner.merge_res(res_all)                                               (plan.py:241-247)
  with ONE rollout call for the candidates of all chunks and ONE for the chunk winners.  The reference needs the
  chunks because its dense rollout does not fit 20,000 candidates; the engine does not, but the chunks are part of
  the semantics - `running_cost` normalises by maxima over the chunk it is given (plan.py:37, losses.py:62) and the
  winners are compared by a batch-of-one re-evaluation - so the chunked entry evaluates chunk by chunk and merges
  exactly like the loop.  Per-candidate rollouts do not depend on what else is in the batch, hence the
  result equals the loop's bit for bit (tests/test_gpu_more.py).
* `group` (config key, optional; r06): with a torch.distributed group and an announced loop (`planner.total_chunks = n_chunk`, what
  plan.py:210 and random_interact.py:188 do) the reference's UNCHANGED loop is dealt to the ranks: call ci of the series is evaluated
  by rank ci % world (on that rank's side streams), every other rank only draws the call's samples - so all generators stay in
  step - and gets a placeholder result (NaN `act_seq`, no outputs); `merge_res` all-gathers (error code, winner's score, winner's
  action sequence) per call - n_chunk x (2 + n_look_ahead x action_dim) numbers -, takes the reference's argmax on every rank and
  broadcasts the winning call's `best_model_output` / `best_eval_output` from its owner.  40 chunks on 8 ranks: 5 calls per rank.
  The two callables must be rank-local (no collective of their own: the ranks evaluate different calls); an error any rank meets
  ("Exceeds max dims", ...) is raised by `merge_res` on EVERY rank, after the exchange - never inside one rank's call, which would
  leave the others hanging in the collective.  `trajectory_optimization_chunked` deals contiguous chunk ranges the same way.
* `planner_type` 'CMA' (not in the reference's list): `trajectory_optimization_cma` - the MPPI round loop with a covariance-adapting
  search (cma.CmaSearch, csrc/ag_cma.hip) in place of the sampler and the softmax update; config keys `cma_sigma0` (0.25) and
  `cma_periodic` ([2] for 4-component actions).  Its calls are never dealt to side streams or ranks; a lone call waits once.
* `planner_type` 'GD' raises NotImplementedError: it differentiates through the rollout and the engine has no backward.
* The reference's own loop - 40 x `trajectory_optimization`, then `merge_res` - is served as it stands (r05): when
  `model_rollout_fn` is the engine's `dynamics` behind a `functools.partial` (what plan.py:190 builds), consecutive calls on
  the same `state_cur` / `act_seq` tensors are independent of each other, and the class deals them to `pipeline_chunks` (default
  6) side streams: each call's sampling, rollout, evaluation and update are enqueued on one of them without waiting for the GPU
  (the rollout's "Exceeds max dims" flag comes back through pinned memory), the caller's stream is made to wait (on the GPU) for
  the call's end before the result is handed back - so results are used in stream order as always - and the next call starts on
  another stream while this one still runs.  Same samples (the generator advances on the host, in call order), same per-candidate
  results (a rollout does not depend on its batch, stream or neighbours, bit for bit), so the same winner.  What changes:
  "Exceeds max dims" of call i surfaces at a later call, at the loop's last call or at `merge_res` - where the reference's loop
  first reads a result back (planner.py:312-314) - instead of inside call i.  r06: this deferral is tied to the caller having
  ANNOUNCED the loop (`planner.total_chunks = n_chunk > 1`, as both reference call sites do) or having put 'pipeline_chunks' into
  the config: a planner that is called once per control step and never merged raises inside the call, as the reference does.
  Dealing also needs push lengths that provably stay within the task config's bound (`_repeats_within_bound`: a call that does
  not wait cannot fall back to the host decode), and the series' other GPU inputs (cost targets, ...) must not change between
  its first call and `merge_res` (the side streams are ordered behind the caller's stream at the series' first call and whenever
  `state_cur` / `act_seq` change).  When calls are NOT dealt the class says why, once (logger `adaptigraph_amd.planner`).
  A call that is not dealt still waits only ONCE, at its end, for all its update rounds (`_one_wait_call`), and the best-so-far
  selection between rounds (planner.py:254-260) stays on the device.  `pipeline_chunks: 0` restores the strict behaviour: every
  rollout waits for its flags.  Also (r05) the winner's rollout is taken out of its batch (`reuse_best_rollout`) by default when
  the rollout is the engine's.

The progress lines the reference prints on every call go to stdout only with `verbose`.
"""
from __future__ import annotations

import logging

import numpy as np
import torch

log = logging.getLogger("adaptigraph_amd.planner")
_OWNER = "_chunk_owner"      # key of a result dictionary of a rank-dealt call: (index of the call in its series, owning rank)


def farthest_points(points, num, init_idx=-1):
    """Greedy farthest-point subset of `points` (n, c) -> (num, c), the rule of planner.py:15-36: start from the row
    whose second half differs most from its first half (or `init_idx`), then always take the row farthest from the
    chosen set; ties go to the lowest index (numpy argmax)."""
    pts = np.asarray(points)
    n, c = pts.shape
    assert n > 0
    if init_idx == -1:
        half = c // 2
        first = int(np.argmax(np.linalg.norm(pts[:, half:] - pts[:, :half], axis=1)))
    else:
        first = int(init_idx)
    chosen = [first]
    nearest = np.linalg.norm(pts - pts[first], axis=1)
    while len(chosen) < num:
        nxt = int(np.argmax(nearest))
        chosen.append(nxt)
        nearest = np.minimum(nearest, np.linalg.norm(pts - pts[nxt], axis=1))
    return pts[chosen]


def _engine_rollout(fn):
    """`fn` if it is the engine's dynamics() bound with keywords only, as plan.py:190 binds it - the callable whose calls may
    be issued without waiting (`_sync=False`) and whose per-candidate results do not depend on the batch - else None."""
    import functools
    from .forward_dynamics import dynamics
    from .model import DynamicsPredictor
    if not (isinstance(fn, functools.partial) and fn.func is dynamics and not fn.args):
        return None
    kw = fn.keywords or {}
    if "_sync" in kw or "_overflow_flag" in kw or not isinstance(kw.get("model"), DynamicsPredictor) or "ppm_optimizer" not in kw:
        return None
    return fn


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v)


def _require_rank_local(fn, what):
    """Raise if `fn` is a functools.partial (possibly nested, possibly around other partials in its keywords) that binds a
    non-None `group`: such a callable all-reduces inside every call."""
    import functools
    seen = []

    def walk(f):
        if isinstance(f, functools.partial):
            for k, v in (f.keywords or {}).items():
                if k == "group" and v is not None:
                    seen.append(k)
                walk(v)
            for v in f.args:
                walk(v)
            walk(f.func)
    walk(fn)
    if seen:
        raise ValueError(f"trajectory_optimization_chunked with a process group needs a rank-local {what}: it was built with "
                         "group=... and would issue a collective per call, but the ranks evaluate different numbers of chunks "
                         "(mismatched collectives hang). Build it with group=None; use mpc_iteration for one batch sharded "
                         "over the ranks with batch-global maxima.")


def _broadcast_result(obj, src, pg, device):
    """Nested dict / list / tuple result `obj` of rank `src` (global rank) -> the same structure on every rank of the group:
    the structure, shapes and dtypes travel as one small pickled object, the tensors as one broadcast each."""
    import torch.distributed as dist

    def spec_of(o):
        if isinstance(o, torch.Tensor):
            return ("__tensor__", tuple(o.shape), o.dtype)
        if isinstance(o, dict):
            return {k: spec_of(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return type(o)(spec_of(v) for v in o)
        return o

    box = [spec_of(obj) if obj is not None else None]
    dist.broadcast_object_list(box, src=src, group=pg)
    it = iter(list(_tensors(obj))) if obj is not None else None

    def build(sp):
        if isinstance(sp, tuple) and len(sp) == 3 and sp[0] == "__tensor__":
            t = next(it).contiguous() if it is not None else torch.empty(sp[1], dtype=sp[2], device=device)
            dist.broadcast(t, src=src, group=pg)
            return t
        if isinstance(sp, dict):
            return {k: build(v) for k, v in sp.items()}
        if isinstance(sp, (list, tuple)):
            return type(sp)(build(v) for v in sp)
        return sp
    return build(box[0])


class Planner(object):
    _REQUIRED = ("action_dim", "model_rollout_fn", "evaluate_traj_fn", "n_sample", "n_look_ahead", "n_update_iter",
                 "reward_weight", "action_lower_lim", "action_upper_lim", "planner_type")

    def __init__(self, config):
        """config keys: planner.py:40-76 (required) and :89-112 (optional), plus the optional `group`."""
        for k in self._REQUIRED:
            if k not in config:
                raise KeyError(k)
        self.config = config
        self.action_dim = config["action_dim"]
        self.model_rollout = config["model_rollout_fn"]
        self.evaluate_traj = config["evaluate_traj_fn"]
        self.n_sample = config["n_sample"]
        self.n_look_ahead = config["n_look_ahead"]
        self.n_update_iter = config["n_update_iter"]
        self.reward_weight = config["reward_weight"]
        self.action_lower_lim = config["action_lower_lim"]
        self.action_upper_lim = config["action_upper_lim"]
        self.planner_type = config["planner_type"]
        assert self.planner_type in ["GD", "MPPI", "MPPI_GD", "CMA"]
        assert type(self.action_lower_lim) == torch.Tensor and type(self.action_upper_lim) == torch.Tensor
        assert self.action_lower_lim.shape == (self.action_dim,)
        assert self.action_upper_lim.shape == (self.action_dim,)
        self.device = config.get("device", "cuda")
        self.verbose = config.get("verbose", False)
        self.sample_action_sequences = config.get("sampling_action_seq_fn", self.sample_action_sequences_default)
        self.clip_action_sequences = config.get("clip_action_seq_fn", self.clip_actions_default)
        self.optimize_action_mppi = config.get("optimize_action_mppi_fn", self.optimize_action_mppi_default)
        self.noise_type = config.get("noise_type", "normal")
        assert self.noise_type in ["normal", "fps"]
        self.noise_level = config.get("noise_level", 0.1)
        self.n_his = config.get("n_his", 1)
        self.rollout_best = config.get("rollout_best", True)
        self.lr = config.get("lr", 1e-3)
        self.group = config.get("group", None)
        # planner_type 'CMA' (trajectory_optimization_cma): the start step as a fraction of each coordinate's range - a default
        # argument, not a tuned value - and the action components that wrap (the push angle of an (x, z, theta, length) action)
        self.cma_sigma0 = float(config.get("cma_sigma0", 0.25))
        self.cma_periodic = [int(k) for k in config.get("cma_periodic", [2] if self.action_dim == 4 else [])]
        self.last_cma = None         # the CmaSearch of the last 'CMA' call
        self._cma_limits = None
        # Optional, off by default (the reference's call pattern): the rollout of the best sampled sequence is taken from the
        # batch it was sampled in instead of being computed again with a batch of one (planner.py:268-271).  Exact on this
        # engine - a candidate's rollout does not depend on its batch, bit for bit - and NOT in general (a BLAS-backed
        # rollout may round differently at another batch size), so it is the caller's statement about model_rollout_fn.
        # r05: default ON when model_rollout_fn is the engine's own dynamics() (then the statement is the engine's, tested by
        # test_dynamics_chunking_is_bit_invariant), OFF for any other callable.
        self._eng_rollout = _engine_rollout(self.model_rollout)
        self.reuse_best_rollout = bool(config.get("reuse_best_rollout", self._eng_rollout is not None))
        # Side streams the independent calls of the caller's chunk loop are dealt to (module docstring); 0 / 1: every call on
        # the caller's stream, waiting for its rollout's flags (the strict per-call error behaviour).
        # (6: measured on the shipped 40 x 500 configuration, tools/probe_loop_host.py - rope 161 / 151 / 159 ms per planner call
        # with 4 / 6 / 8 streams and eight hardware queues, granular 241 / 225 / 227, cloth 212 / 217 / 219)
        self.pipeline_chunks = int(config.get("pipeline_chunks", 6 if self._eng_rollout is not None else 0))
        # Dealing defers a call's "Exceeds max dims" to merge_res, so it is tied to the caller having announced a chunk loop the
        # way both reference call sites do - `planner.total_chunks = n_chunk` (plan.py:210, random_interact.py:188) - or having
        # put 'pipeline_chunks' into the config itself.  A planner that is called once per MPC step and never merged
        # (total_chunks 1) runs every call strictly: the exception is raised inside the call, as in the reference.
        self._pipe_explicit = "pipeline_chunks" in config
        self._side = None            # (device, [streams])
        self._pipe_in = None         # (state_cur, act_seq, (versions, caller stream), entry event): inputs of the running series
        self._pipe_i = 0
        self._call_flags = None      # flag tensors of the rollouts of the call being enqueued
        self._call_one_stream = True # the call being enqueued keeps the engine on its one stream (dealt calls)
        self._dealt_prefix_later = False   # True: dealt calls keep the contact-free prefix in update rounds >= 1 too (A/B switch, _rollout)
        self._bound_ok = None        # (_repeats_within_bound's verdict,) once decided
        self._pending = []           # (pinned flag copy, done event) of calls whose flags have not been looked at
        self._series_i = 0           # calls since the last merge_res = index of the next call in the caller's chunk loop
        self._series_err = None      # what a rank-dealt call raised: kept for merge_res, where all ranks agree on it
        self._said = set()           # reasons already logged
        self.chunk_id = 0
        self.total_chunks = 1
        why = self._pipeline_off_static()
        if why and str(self.device) != "cpu":
            self._say("planner: calls are not dealt to side streams (every call waits for its rollout) because " + why)

    def _say(self, msg):
        if msg not in self._said:
            self._said.add(msg)
            log.warning(msg)

    def _pipeline_off_static(self):
        """why the chunk loop cannot be dealt to side streams whatever the caller does later, or None"""
        if self.planner_type != "MPPI":
            return f"planner_type is {self.planner_type!r}"
        if self._eng_rollout is None:
            return ("model_rollout_fn is not functools.partial(adaptigraph_amd.dynamics, model=<DynamicsPredictor>, device=..., "
                    "ppm_optimizer=...) with keyword arguments only (plan.py:190): a lambda, a positional argument or another "
                    "callable is run as given")
        if self.pipeline_chunks < 2:
            return f"config['pipeline_chunks'] is {self.pipeline_chunks}"
        if self.verbose:
            return "config['verbose'] is set"
        return None

    # ------------------------------------------------------------------------------------------ defaults of the config
    def sample_action_sequences_default(self, act_seq, iter_index=None):
        """planner.py:118-166 -> (n_sample, n_look_ahead, action_dim).  'normal': low-pass filtered Gaussian
        perturbations of the nominal sequence (filter 0.7, one torch.normal draw per look-ahead step), clamped to the
        limits; 'fps': farthest-point subset of a 0.02 grid over the action box, repeated along the horizon.
        (`iter_index` is accepted because the MPPI loop passes it to whatever sampler is configured.)"""
        assert type(act_seq) == torch.Tensor and act_seq.shape == (self.n_look_ahead, self.action_dim)
        if self.noise_type == "fps":
            lo, hi = self.action_lower_lim.cpu().numpy(), self.action_upper_lim.cpu().numpy()
            axes = [np.arange(lo[d], hi[d], 0.02) for d in range(self.action_dim)]
            grid = np.stack(np.meshgrid(*axes), axis=-1).reshape(-1, self.action_dim)
            picked = torch.from_numpy(farthest_points(grid, self.n_sample)).to(self.device).float()
            return picked.unsqueeze(1).repeat(1, self.n_look_ahead, 1)
        if self.noise_type != "normal":
            raise ValueError("unknown noise type: %s" % self.noise_type)
        keep = 0.7
        out = act_seq.clone().unsqueeze(0).repeat(self.n_sample, 1, 1)
        drift = torch.zeros((self.n_sample, self.action_dim), dtype=out.dtype, device=self.device)
        for t in range(self.n_look_ahead):
            noise = torch.normal(0, self.noise_level, (self.n_sample, self.action_dim), device=self.device)
            drift = keep * noise + drift * (1. - keep)
            out[:, t] += drift
            out[:, t] = torch.clamp(out[:, t], self.action_lower_lim, self.action_upper_lim)
        return out

    def clip_actions_default(self, act_seqs):
        """planner.py:226-230: clamp in place, return the same tensor."""
        act_seqs.data.clamp_(self.action_lower_lim, self.action_upper_lim)
        return act_seqs

    def optimize_action_mppi_default(self, act_seqs, reward_seqs):
        """planner.py:204-206: softmax(reward * reward_weight)-weighted mean of the sampled sequences, clipped."""
        w = torch.softmax(reward_seqs * self.reward_weight, dim=0)
        return self.clip_action_sequences(torch.sum(act_seqs * w[:, None, None], dim=0))

    def optimize_action(self, act_seqs, reward_seqs, optimizer=None):
        assert type(act_seqs) == torch.Tensor and type(reward_seqs) == torch.Tensor
        assert act_seqs.shape == (self.n_sample, self.n_look_ahead, self.action_dim)
        assert reward_seqs.shape == (self.n_sample,)
        if self.planner_type == "MPPI":
            return self.optimize_action_mppi(act_seqs, reward_seqs)
        if self.planner_type == "GD":
            raise NotImplementedError("planner_type 'GD' differentiates through the rollout; the HIP engine is inference-only")
        if self.planner_type == "MPPI_GD":
            raise NotImplementedError
        raise ValueError("unknown planner type: %s" % self.planner_type)

    # ------------------------------------------------------------------------------------------------- optimisation
    def trajectory_optimization(self, state_cur, act_seq):
        """planner.py:185-202.  -> {'act_seq', 'model_outputs', 'eval_outputs', 'best_model_output', 'best_eval_output'}"""
        assert type(state_cur) == torch.Tensor and type(act_seq) == torch.Tensor
        assert act_seq.shape == (self.n_look_ahead, self.action_dim)
        if self.planner_type == "MPPI":
            k = self._series_i
            self._series_i += 1
            world, rank, _ = self._loop_world()
            if world > 1:
                return self._rank_dealt(state_cur, act_seq, k, world, rank)
            if self._can_pipeline(state_cur):
                res = self._pipelined(state_cur, act_seq)
                if self.total_chunks > 1 and k == self.total_chunks - 1:
                    self.check_pending(block=True)           # the loop's last call: merge_res would wait here anyway
                return res
            self.check_pending(block=True)                   # (a strict call: nothing of earlier calls stays unreported)
            if self._can_wait_once(state_cur):
                return self._one_wait_call(state_cur, act_seq)
            return self.trajectory_optimization_mppi(state_cur, act_seq)
        if self.planner_type == "CMA":
            # never dealt to side streams or ranks (_pipeline_off_static); a caller's chunk loop + merge_res = independent restarts
            self.check_pending(block=True)
            if self._can_wait_once(state_cur):
                return self._one_wait_call(state_cur, act_seq, self.trajectory_optimization_cma)
            return self.trajectory_optimization_cma(state_cur, act_seq)
        if self.planner_type == "GD":
            return self.trajectory_optimization_gd(state_cur, act_seq)
        if self.planner_type == "MPPI_GD":
            raise NotImplementedError
        raise ValueError("unknown planner type: %s" % self.planner_type)

    # ---------------------------------------------------------------- independent calls dealt to side streams (module docstring)
    def _loop_world(self):
        """(world, rank, process group) the caller's chunk loop is dealt over: more than one rank only with config['group'], an
        initialised torch.distributed and an announced loop (`planner.total_chunks = n_chunk`, plan.py:210)."""
        if self.group is None or self.total_chunks <= 1 or self.verbose or not self.rollout_best:
            return 1, 0, None
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return 1, 0, None
        pg = None if self.group is True else self.group
        return dist.get_world_size(pg), dist.get_rank(pg), pg

    def _can_pipeline(self, state_cur, rank_dealt=False):
        if self._pipeline_off_static() is not None:
            return False
        why = None
        if not state_cur.is_cuda:
            return False
        if torch.cuda.is_current_stream_capturing():
            return False
        if self.group is not None and not rank_dealt:
            # (an evaluation that issues collectives keeps its issue order on the caller's stream)
            why = ("config['group'] is set but no chunk loop was announced: set planner.total_chunks = n_chunk (plan.py:210) and the "
                   "calls are dealt to the ranks, chunk ci to rank ci % world")
        elif self._repeats_within_bound() is not None:
            why = self._repeats_within_bound() + ": every call waits for its rollout so that it can fall back to the host decode"
        elif self.total_chunks <= 1 and not self._pipe_explicit:
            why = ("planner.total_chunks is 1: a lone call raises its own errors, as in the reference; announce the chunk loop with "
                   "planner.total_chunks = n_chunk (plan.py:210, random_interact.py:188) or put 'pipeline_chunks' into the config")
        if why:
            self._say("planner: calls are not dealt to side streams because " + why)
            return False
        return True

    # ------------------------------------------------- the caller's chunk loop dealt to the ranks of config['group'] (r06)
    def _rank_dealt(self, state_cur, act_seq, k, world, rank):
        """Call k of the announced loop (plan.py:241-247) on a multi-rank group: rank k % world evaluates it - on its side streams,
        like a one-rank planner - and every other rank only draws the call's samples, so that all generators stay in step, and hands
        back a placeholder.  merge_res all-gathers the winners.  Nothing is raised here (a rank that left the loop alone would
        leave the others hanging in merge_res's collective): errors are kept for merge_res."""
        if k == 0:
            # the ranks evaluate different calls, so the callables must not issue collectives of their own (same config on every
            # rank: every rank raises here, before any of them has entered anything)
            try:
                _require_rank_local(self.evaluate_traj, "evaluate_traj_fn")
                _require_rank_local(self.model_rollout, "model_rollout_fn")
            except ValueError:
                self._series_i = 0
                raise
        owner = k % world
        if k >= self.total_chunks and self._series_err is None:
            self._series_err = RuntimeError(f"call {k + 1} of a chunk loop announced with planner.total_chunks = {self.total_chunks}: "
                                            "merge_res must close a series before the next one starts")
        if owner == rank and self._series_err is None:
            try:
                if self._can_pipeline(state_cur, rank_dealt=True):
                    res = self._pipelined(state_cur, act_seq, raise_early=False)
                elif self._can_wait_once(state_cur):
                    res = self._one_wait_call(state_cur, act_seq)
                else:
                    res = self.trajectory_optimization_mppi(state_cur, act_seq)
                res[_OWNER] = (k, owner)
                return res
            except Exception as e:  # noqa: BLE001 - re-raised by merge_res on every rank
                self._series_err = e
        else:
            for i in range(self.n_update_iter):              # same draws as the owner: shapes alone decide what a draw consumes
                self.sample_action_sequences(act_seq, iter_index=i)
        return {"act_seq": torch.full_like(act_seq, float("nan")), "model_outputs": None, "eval_outputs": None,
                "best_model_output": None, "best_eval_output": None, _OWNER: (k, owner)}

    def _limits_of_rollout(self):
        from .forward_dynamics import _repeat_bound
        task = self._eng_rollout.keywords["ppm_optimizer"].task_config
        return int(task["max_nR"]), _repeat_bound(task)

    def _rollout(self, state_cur, act_seqs, update_round=0):
        """model_rollout_fn; inside a pipelined call the engine's dynamics() is told not to wait for its flags"""
        if self._call_flags is None:
            return self.model_rollout(state_cur, act_seqs)
        flags = torch.zeros(2, dtype=torch.int32, device=state_cur.device)
        self._call_flags.append(flags)
        if update_round > 0 and self._call_one_stream and not self._dealt_prefix_later:
            # A dealt call's LATER update rounds (n_update_iter > 1, random_interact.py:172) run without the contact-free prefix:
            # prefix sharing plans its launches on the host from a census of the batch, i.e. the call waits for that census - and
            # round i + 1's samples come out of round i's rewards, so the wait is for the whole of round i and the next dealt call
            # cannot be enqueued before this one has all but finished on the GPU.  Without it the device-planned rollout needs no
            # answer from the GPU.  Round 0 keeps it: uniform samples over the action box mostly never touch (its census sits at
            # the head of the side stream), later rounds sample around the best push so far.  Same results either way, bit for bit.
            kw = self._eng_rollout.keywords
            eng = kw["model"].engine(torch.device(kw["device"]))
            with eng.options(streams=1, share_prefix=0):
                return self._eng_rollout(state_cur, act_seqs, _sync=False, _overflow_flag=flags)
        # a dealt call stays on its one stream (option streams = 1 for the duration of the enqueue): six of them already run side
        # by side, and a fork inside each doubles the launches and lets in-library streams share hardware queues with the side
        # streams (rope planner call 168 +- 10 ms with the engine's by-size fork, 147 without, run after run)
        if not self._call_one_stream:                        # a lone call on the caller's stream: the engine forks by size as always
            return self._eng_rollout(state_cur, act_seqs, _sync=False, _overflow_flag=flags)
        kw = self._eng_rollout.keywords
        eng = kw["model"].engine(torch.device(kw["device"]))
        with eng.options(streams=1):
            return self._eng_rollout(state_cur, act_seqs, _sync=False, _overflow_flag=flags)

    def _repeats_within_bound(self):
        """None if no sampled action can carry an action_repeat beyond what the engine's device-planned rollout serves
        (task_config['action_upper_lim'][3]), else why that cannot be ruled out.  Only then may a rollout be enqueued without
        waiting for it: a call that waits (`dynamics(_sync=True)`) falls back to the host decode for such an action, as the
        reference accepts any push length (forward_dynamics.py:156), and a call that does not wait could only raise.  Decided
        once, from the limits the sampler and the MPPI update clamp to (read back once: this is not the hot path)."""
        if self._bound_ok is not None:
            return self._bound_ok[0]
        import functools
        from .forward_dynamics import _repeat_bound
        from . import mppi as _mppi
        why = None
        bound = _repeat_bound(self._eng_rollout.keywords["ppm_optimizer"].task_config)
        uppers = []
        # 'CMA': every sample is folded into the planner's own limits (CmaSearch), whatever sampler and update are configured
        for what, fn, mine, theirs in (() if self.planner_type == "CMA" else
                                      (("sampling_action_seq_fn", self.sample_action_sequences, self.sample_action_sequences_default, _mppi.sample_action_seq),
                                       ("optimize_action_mppi_fn", self.optimize_action_mppi, self.optimize_action_mppi_default, _mppi.optimize_action_mppi))):
            if getattr(fn, "__func__", None) is getattr(mine, "__func__", object()) and getattr(fn, "__self__", None) is self:
                if what == "optimize_action_mppi_fn" and self.clip_action_sequences != self.clip_actions_default and not (
                        isinstance(self.clip_action_sequences, functools.partial) and self.clip_action_sequences.func is _mppi.clip_actions):
                    why = "clip_action_seq_fn is not the planner's own clamp or adaptigraph_amd.clip_actions"
                uppers.append(self.action_upper_lim)
            elif isinstance(fn, functools.partial) and fn.func is theirs and fn.keywords.get("action_upper_lim") is not None:
                uppers.append(fn.keywords["action_upper_lim"])
            else:
                why = f"{what} is neither the planner's default nor functools.partial(adaptigraph_amd.{theirs.__name__}, action_upper_lim=...)"
        if self.planner_type == "CMA":
            uppers.append(self.action_upper_lim)
        elif isinstance(self.clip_action_sequences, functools.partial) and self.clip_action_sequences.func is _mppi.clip_actions \
                and self.clip_action_sequences.keywords.get("action_upper_lim") is not None:
            uppers.append(self.clip_action_sequences.keywords["action_upper_lim"])
        if bound is None:
            why = "task_config has no 'action_upper_lim' (planning/*.yaml:28-29) to bound action_repeat with"
        elif why is None:
            try:
                top = max(float(torch.as_tensor(u).reshape(-1)[3]) for u in uppers) if self.action_dim == 4 else None
            except (IndexError, TypeError, ValueError):
                top = None
            if top is None or not int(top) <= bound:
                why = (f"the planner's limits allow a push length of {top} but task_config['action_upper_lim'][3] bounds action_repeat "
                       f"by {bound}")
        if why is not None:
            why = "an action_repeat beyond the task config's bound cannot be ruled out (" + why + ")"
        self._bound_ok = (why,)
        return why

    def check_pending(self, block=True):
        """Look at the flags of the pipelined calls that have finished (block: wait for all of them): raises what their
        dynamics() would have raised.  Called by every trajectory_optimization (non-blocking) and by merge_res (blocking)."""
        if not self._pending:
            return
        max_nR, bound = self._limits_of_rollout()
        keep = []
        err = None
        for host, done in self._pending:
            if block:
                done.synchronize()
            elif not done.query():
                keep.append((host, done))
                continue
            for seen_nR, seen_rep in host.tolist():           # pinned host memory, written before `done`: no device access
                if seen_nR > max_nR:
                    err = Exception("Exceeds max dims")        # utils.py:63-65
                elif bound is not None and seen_rep > bound and err is None:
                    err = ValueError(f"an action's repeat count {seen_rep} exceeds the task config's action_upper_lim[3] = {bound}: "
                                     "a pipelined planner call cannot fall back to the host decode (planner config "
                                     "'pipeline_chunks': 0 restores the per-call behaviour)")
        self._pending = keep
        if err is not None:
            self._pending = []
            raise err

    def _can_wait_once(self, state_cur):
        """A call that is not dealt (a lone call, or config['pipeline_chunks'] = 1) still need not wait after EVERY rollout of its
        n_update_iter rounds: with the engine's own dynamics() and repeats that cannot leave the bound it enqueues all rounds on the
        caller's stream and reads all flags once, before it returns - "Exceeds max dims" is raised by the call itself, as in the
        reference (utils.py:63-65), only after the later rounds were enqueued.  config['pipeline_chunks'] = 0: off."""
        return (self._eng_rollout is not None and self.pipeline_chunks != 0 and not self.verbose and state_cur.is_cuda
                and not torch.cuda.is_current_stream_capturing() and self._repeats_within_bound() is None)

    def _one_wait_call(self, state_cur, act_seq, optimise=None):
        self._call_flags, self._call_one_stream = [], False
        try:
            res = (optimise or self.trajectory_optimization_mppi)(state_cur, act_seq)
            flags = self._call_flags
        finally:
            self._call_flags, self._call_one_stream = None, True
        if flags:
            max_nR, bound = self._limits_of_rollout()
            for seen_nR, seen_rep in torch.stack(flags).tolist():          # the one wait of the call
                if seen_nR > max_nR:
                    raise Exception("Exceeds max dims")                    # utils.py:63-65
                assert bound is None or seen_rep <= bound, "an action_repeat beyond the bound (_repeats_within_bound said it cannot happen)"
        return res

    def _pipelined(self, state_cur, act_seq, raise_early=True):
        dev = state_cur.device
        cur = torch.cuda.current_stream(dev)
        if raise_early:
            self.check_pending(block=False)
        # Are these the inputs of the previous call, untouched?  (same tensor objects, same version counters, same caller
        # stream.)  Then they were ready where that series started and this call need not queue up behind the previous one.
        tag = (state_cur._version, act_seq._version, cur.cuda_stream)
        pin = self._pipe_in
        if pin is None or pin[0] is not state_cur or pin[1] is not act_seq or pin[2] != tag:
            entry = torch.cuda.Event()
            entry.record(cur)
            self._pipe_in = pin = (state_cur, act_seq, tag, entry)
        if self._side is None or self._side[0] != dev or len(self._side[1]) != self.pipeline_chunks:
            self._side = (dev, [torch.cuda.Stream(dev) for _ in range(self.pipeline_chunks)])
        side = self._side[1][self._pipe_i % len(self._side[1])]
        self._pipe_i += 1
        side.wait_event(pin[3])
        self._call_flags = []
        try:
            with torch.cuda.stream(side):
                res = self.trajectory_optimization_mppi(state_cur, act_seq)
                flags = self._call_flags
                host = torch.empty((len(flags), 2), dtype=torch.int32, pin_memory=True)
                if flags:
                    host.copy_(torch.stack(flags), non_blocking=True)
        finally:
            self._call_flags = None
        done = torch.cuda.Event()
        done.record(side)
        cur.wait_event(done)                                 # the caller uses the result in stream order, as always
        for t in _tensors(res):
            t.record_stream(cur)
        self._pending.append((host, done))
        return res

    def _evaluate(self, model_out, act_seqs, state_cur):
        return self.evaluate_traj(model_out["state_seqs"], act_seqs, state_cur=state_cur,
                                  weights=model_out["weights"] if "weights" in model_out else None)

    @torch.no_grad()
    def trajectory_optimization_mppi(self, state_cur, act_seq):
        """planner.py:234-277: n_update_iter rounds of sample -> rollout -> evaluate -> MPPI update; the best sampled
        sequence over all rounds is returned (not the MPPI mean) and, with rollout_best, rolled out once more."""
        model_outputs, eval_outputs = [], []
        best_act_seq = best_reward = best_rows = None
        for i in range(self.n_update_iter):
            if self.verbose:
                print(f"chunk: {self.chunk_id}/{self.total_chunks}, iter: {i}/{self.n_update_iter}")
            act_seqs = self.sample_action_sequences(act_seq, iter_index=i)
            assert type(act_seqs) == torch.Tensor
            assert act_seqs.shape == (self.n_sample, self.n_look_ahead, self.action_dim)
            model_out = self._rollout(state_cur, act_seqs, update_round=i)
            assert type(model_out["state_seqs"]) == torch.Tensor
            eval_out = self._evaluate(model_out, act_seqs, state_cur)
            reward_seqs = eval_out["reward_seqs"]
            act_seq = self.optimize_action(act_seqs, reward_seqs)
            top = torch.argmax(reward_seqs)
            # planner.py:254-260 `if i == 0 or reward_seqs[top] > best_reward: keep this round's best` without turning a 0-d GPU
            # tensor into a Python bool (a wait for the whole rollout and evaluation, once per update iteration - five per call in
            # random_interact.py's configuration): index_select instead of act_seqs[top], and the comparison stays on the device
            # as the condition of torch.where.  Same values, same winner.
            sel = top.reshape(1)
            round_act, round_reward = torch.index_select(act_seqs, 0, sel)[0], torch.index_select(reward_seqs, 0, sel)[0]
            round_rows = self._pick(model_out, top, act_seqs.shape[0]) if self.reuse_best_rollout else None
            if i == 0:
                best_act_seq, best_reward, best_rows = round_act, round_reward, round_rows
            else:
                better = round_reward > best_reward                                  # 0-d bool, stays where the rewards are
                best_act_seq = torch.where(better, round_act, best_act_seq)
                if round_rows is not None:
                    best_rows = {key: (torch.where(better.to(v.device), v, best_rows[key])
                                       if isinstance(v, torch.Tensor) and isinstance(best_rows[key], torch.Tensor)
                                       and v.shape == best_rows[key].shape else v) for key, v in round_rows.items()}
                best_reward = torch.where(better, round_reward, best_reward)
            if self.verbose:
                model_outputs.append(model_out)
                eval_outputs.append(eval_out)
        act_seq = best_act_seq
        best_model_out = best_eval_out = None
        if self.rollout_best:
            best_model_out = best_rows if best_rows is not None else self._rollout(state_cur, act_seq.unsqueeze(0))
            best_eval_out = self.evaluate_traj(best_model_out["state_seqs"], act_seq.unsqueeze(0), state_cur=state_cur)
        return {"act_seq": act_seq,
                "model_outputs": model_outputs if self.verbose else None,
                "eval_outputs": eval_outputs if self.verbose else None,
                "best_model_output": best_model_out,
                "best_eval_output": best_eval_out}

    @torch.no_grad()
    def trajectory_optimization_cma(self, state_cur, act_seq):
        """The round loop of trajectory_optimization_mppi with a CMA-ES search (cma.CmaSearch) in place of the sampler and the MPPI
        update: the mean starts at `act_seq`, a generation is n_sample candidates, there are n_update_iter generations, rewards are
        maximised.  The search runs over the flattened (n_look_ahead x action_dim) sequence inside the planner's limits (folded;
        `cma_periodic` components wrap with period 2 pi), start step `cma_sigma0` of each coordinate's range.  Same result dictionary:
        'act_seq' is the best SAMPLED sequence over all generations.  The winner's rows are picked with the tell's device-side
        `order` / `improved` - no Python bool of a device value, no wait between generations."""
        from .cma import CmaSearch
        H, A = self.n_look_ahead, self.action_dim
        if self._cma_limits is None:                         # host copies of the limits, read back once
            self._cma_limits = (self.action_lower_lim.detach().to("cpu", torch.float64).repeat(H),
                                self.action_upper_lim.detach().to("cpu", torch.float64).repeat(H))
        lo, hi = self._cma_limits
        search = CmaSearch(act_seq.detach().reshape(-1), self.cma_sigma0, lo, hi, popsize=self.n_sample, device=self.device,
                           periodic=[h * A + k for h in range(H) for k in self.cma_periodic], maximize=True)
        self.last_cma = search
        model_outputs, eval_outputs = [], []
        best_act_seq = best_rows = None
        for i in range(self.n_update_iter):
            if self.verbose:
                print(f"chunk: {self.chunk_id}/{self.total_chunks}, iter: {i}/{self.n_update_iter}")
            act_seqs = search.ask().reshape(self.n_sample, H, A)
            model_out = self._rollout(state_cur, act_seqs, update_round=i)
            assert type(model_out["state_seqs"]) == torch.Tensor
            eval_out = self._evaluate(model_out, act_seqs, state_cur)
            reward_seqs = eval_out["reward_seqs"]
            assert reward_seqs.shape == (self.n_sample,)
            search.tell(reward_seqs)
            top, better = search.order[:1], search.improved
            round_act = torch.index_select(act_seqs, 0, top)[0]
            round_rows = self._pick(model_out, top, act_seqs.shape[0]) if self.reuse_best_rollout else None
            if i == 0:
                best_act_seq, best_rows = round_act, round_rows
            else:
                best_act_seq = torch.where(better, round_act, best_act_seq)
                if round_rows is not None:
                    best_rows = {key: (torch.where(better.to(v.device), v, best_rows[key])
                                       if isinstance(v, torch.Tensor) and isinstance(best_rows[key], torch.Tensor)
                                       and v.shape == best_rows[key].shape else v) for key, v in round_rows.items()}
            if self.verbose:
                model_outputs.append(model_out)
                eval_outputs.append(eval_out)
        act_seq = best_act_seq
        best_model_out = best_eval_out = None
        if self.rollout_best:
            best_model_out = best_rows if best_rows is not None else self._rollout(state_cur, act_seq.unsqueeze(0))
            best_eval_out = self.evaluate_traj(best_model_out["state_seqs"], act_seq.unsqueeze(0), state_cur=state_cur)
        return {"act_seq": act_seq,
                "model_outputs": model_outputs if self.verbose else None,
                "eval_outputs": eval_outputs if self.verbose else None,
                "best_model_output": best_model_out,
                "best_eval_output": best_eval_out}

    def trajectory_optimization_gd(self, state_cur, act_seq):
        raise NotImplementedError("planner_type 'GD' differentiates through the rollout; the HIP engine is inference-only")

    def trajectory_optimization_mppi_gd(self, state_cur, act_seq=None):
        pass

    def merge_res(self, res_list):
        """planner.py:311-323: the chunk whose winner scores best in its own batch-of-one re-evaluation."""
        assert not self.verbose and self.rollout_best
        self._series_i = 0
        self._pipe_in = None                                  # the next series records its own entry event
        if any(isinstance(res, dict) and _OWNER in res for res in res_list):
            return self._merge_rank_dealt(res_list)
        self.check_pending(block=True)                        # flags of the pipelined calls: here the reference's loop syncs too
        # (one read-back for all chunks; .mean() of the (1,) reward and the Python float are the reference's, planner.py:312-314)
        scores = torch.stack([res["best_eval_output"]["reward_seqs"].mean() for res in res_list]).tolist()
        win = res_list[int(np.argmax(scores))]
        return {"act_seq": win["act_seq"], "model_outputs": None, "eval_outputs": None,
                "best_model_output": win["best_model_output"], "best_eval_output": win["best_eval_output"]}

    def _merge_rank_dealt(self, res_list):
        """merge_res of a loop whose calls were dealt to the ranks (_rank_dealt): one all-gather of (error code, winner's score,
        winner's action sequence) per call - n_chunk x (2 + n_look_ahead x action_dim) numbers -, the reference's argmax over the
        scores on every rank, and the winning call's best_model_output / best_eval_output broadcast from its owner.  An error
        any rank met during the series ("Exceeds max dims", ...) is raised here on EVERY rank, after the exchange."""
        import torch.distributed as dist
        world, rank, pg = self._loop_world()
        err, self._series_err = self._series_err, None
        n, H, A = len(res_list), self.n_look_ahead, self.action_dim
        try:
            self.check_pending(block=True)
        except Exception as e:  # noqa: BLE001
            err = err or e
        if world <= 1:                                        # (the group went away between the calls and the merge)
            raise err or RuntimeError("merge_res: results of a rank-dealt chunk loop, but no multi-rank group")
        like = res_list[0]["act_seq"]
        per = (n + world - 1) // world
        table = torch.zeros((per, 2 + H * A), dtype=like.dtype, device=like.device)
        table[:, 1] = float("-inf")
        if err is None:
            try:
                for k, res in enumerate(res_list):
                    assert res.get(_OWNER) == (k, k % world), "merge_res needs the results of ALL calls of the series, in call order"
                    if k % world == rank:
                        table[k // world, 1] = res["best_eval_output"]["reward_seqs"].mean().to(like.dtype)
                        table[k // world, 2:] = res["act_seq"].reshape(-1)
            except Exception as e:  # noqa: BLE001
                err = e
        table[:, 0] = 0.0 if err is None else (1.0 if str(err) == "Exceeds max dims" else 2.0)
        gathered = torch.empty((world * per, 2 + H * A), dtype=like.dtype, device=like.device)
        dist.all_gather_into_tensor(gathered, table, group=pg)
        host = gathered.cpu()                                 # the one wait of the loop, where the reference's first .item() is
        codes = host[:, 0]
        if float(codes.max()) > 0:
            if err is not None:
                raise err
            if float(codes.max()) == 1.0 and not bool((codes == 2.0).any()):
                raise Exception("Exceeds max dims")           # utils.py:63-65, met by another rank
            bad = sorted({int(i) // per for i in torch.nonzero(codes).reshape(-1)})
            raise RuntimeError(f"planner: rank(s) {bad} failed during the chunk loop (their own exception says why)")
        row = lambda k: (k % world) * per + k // world
        scores = [float(host[row(k), 1]) for k in range(n)]   # planner.py:312-314: Python floats, first maximum wins
        win = int(np.argmax(scores))
        owner = win % world
        src = owner if pg is None else dist.get_global_rank(pg, owner)
        act = gathered[row(win), 2:].reshape(H, A).clone()
        mine = (res_list[win]["best_model_output"], res_list[win]["best_eval_output"]) if rank == owner else None
        best_model, best_eval = _broadcast_result(mine, src, pg, like.device)
        return {"act_seq": act, "model_outputs": None, "eval_outputs": None, "best_model_output": best_model, "best_eval_output": best_eval}

    # ---------------------------------------------------------------------------------- all chunks in two rollout calls
    @staticmethod
    def _rows(out, lo, hi, total):
        """rows [lo, hi) of every per-candidate tensor of a rollout / evaluation result"""
        return {k: (v[lo:hi] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == total else v)
                for k, v in out.items()}

    @staticmethod
    def _pick(out, index, total):
        """row `index` (a 0-d index tensor: no host sync) of every per-candidate tensor of a rollout result, as a batch of one"""
        idx = index.reshape(1)
        return {k: (torch.index_select(v, 0, idx.to(v.device)) if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == total
                    else v) for k, v in out.items()}

    @torch.no_grad()
    def trajectory_optimization_chunked(self, state_cur, act_seq, n_chunk):
        """The loop of plan.py:241-247 (`trajectory_optimization` per chunk, then `merge_res`) with one rollout call for
        all chunks' candidates and one for the chunk winners; see the module docstring.  Needs planner_type 'MPPI',
        n_update_iter == 1 (what plan.py configures), rollout_best and not verbose; anything else takes the loop."""
        n_chunk = int(n_chunk)
        assert type(state_cur) == torch.Tensor and type(act_seq) == torch.Tensor
        assert act_seq.shape == (self.n_look_ahead, self.action_dim)
        if self.planner_type != "MPPI" or self.n_update_iter != 1 or not self.rollout_best or self.verbose or n_chunk < 1:
            res_all, announced = [], self.total_chunks
            self.total_chunks = n_chunk                       # the loop as plan.py:210, 241-247 announces and runs it
            try:
                for ci in range(n_chunk):
                    self.chunk_id = ci
                    res_all.append(self.trajectory_optimization(state_cur, act_seq))
                return self.merge_res(res_all)
            finally:
                self.total_chunks = announced
        import torch.distributed as dist
        from .sharding import shard_bounds, all_gather_costs
        sharded = self.group is not None and dist.is_available() and dist.is_initialized()
        if sharded:
            # chunks are dealt to the ranks, so the ranks call the evaluation a DIFFERENT number of times (zero for some when
            # n_chunk < world): an evaluation that issues a collective per call (running_cost / cloth_penalty built with
            # group=..., as mpc_iteration wants them) would leave the ranks in mismatched collectives - a hang.  Chunk
            # maxima are chunk-local by the reference's own semantics (plan.py:37, losses.py:62 see one chunk), so the
            # callables handed to this entry must be rank-local.
            _require_rank_local(self.evaluate_traj, "evaluate_traj_fn")
            _require_rank_local(self.model_rollout, "model_rollout_fn")
        pg = None if self.group in (None, True) else self.group
        world = dist.get_world_size(pg) if sharded else 1
        rank = dist.get_rank(pg) if sharded else 0
        # every rank draws every chunk's samples, in the loop's order: the generator ends in the same state as after the
        # reference's loop and the winners can be compared anywhere
        samples = [self.sample_action_sequences(act_seq, iter_index=0) for _ in range(n_chunk)]
        S, H, A = self.n_sample, self.n_look_ahead, self.action_dim
        for s in samples:
            assert type(s) == torch.Tensor and s.shape == (S, H, A)
        c_lo, c_hi = shard_bounds(n_chunk, world, rank)
        winners = torch.zeros((c_hi - c_lo, H, A), dtype=samples[0].dtype, device=samples[0].device)
        reuse = self.reuse_best_rollout and world == 1           # (sharded: the winners' rollouts live on other ranks)
        picked = []
        if c_hi > c_lo:
            mine = torch.cat(samples[c_lo:c_hi], dim=0)
            model_out = self.model_rollout(state_cur, mine)
            total = mine.shape[0]
            for j in range(c_hi - c_lo):
                part = self._rows(model_out, j * S, (j + 1) * S, total)
                reward_seqs = self._evaluate(part, samples[c_lo + j], state_cur)["reward_seqs"]
                assert reward_seqs.shape == (S,)
                top = torch.argmax(reward_seqs)
                winners[j] = torch.index_select(samples[c_lo + j], 0, top.reshape(1))[0]      # (no read-back of `top`)
                if reuse:
                    picked.append(self._pick(part, top, S))
        if world > 1:
            k = H * A
            bounds = [tuple(k * b for b in shard_bounds(n_chunk, world, r)) for r in range(world)]
            winners = all_gather_costs(winners.reshape(-1).contiguous(), n_chunk * k, pg, bounds=bounds).reshape(n_chunk, H, A)
        best_out = None if reuse else self.model_rollout(state_cur, winners)
        res_all = []
        for ci in range(n_chunk):
            one = picked[ci] if reuse else self._rows(best_out, ci, ci + 1, n_chunk)
            ev = self.evaluate_traj(one["state_seqs"], winners[ci:ci + 1], state_cur=state_cur)
            res_all.append({"act_seq": winners[ci], "model_outputs": None, "eval_outputs": None,
                            "best_model_output": one, "best_eval_output": ev})
        return self.merge_res(res_all)
