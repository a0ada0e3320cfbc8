"""dynamics_error: the objective the online physics-parameter optimiser evaluates for every BO / CMA-ES proposal
(reference src/planning/physics_param_optimizer.py:178-226) = masked rollout of the past interactions + mean chamfer
to what really happened.  Same signature; dynamics_masked and mean_chamfer run on the HIP engine.  The host optimisers
(skopt.gp_minimize / cma) stay in the reference.  r05: dynamics_error_sweep evaluates a population / sweep of
parameters in one go (independent evaluations dealt to streams, one read-back).  optimize_grad fits the parameter by Adam on
the autograd path; PhysParamFit / optimize_grad_device run the same fit resident on the GPU (ag_ppm_grad_step +
ag_ppm_adam_step: an iteration only enqueues, one read-back at the end)."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import torch

from .context import side_streams as _sweep_streams, ptr, current_stream, _require_gpu, _vp_array
from .forward_dynamics import dynamics_masked, dynamics_masked_diff, _tool_layout, _rollout_params
from .model import DynamicsPredictor
from .plan_utils import decode_action
from .losses import mean_chamfer, chamfer_diff


def _pad_clouds(clouds, rows, device):
    """list of (n_i, 3) arrays -> ((len, rows, 3) float32, (len, rows) bool) on `device`: cloud i in the first n_i rows"""
    pad = np.zeros((len(clouds), rows, 3), np.float32)
    valid = np.zeros((len(clouds), rows), bool)
    for i, cloud in enumerate(clouds):
        pad[i, :len(cloud)] = cloud
        valid[i, :len(cloud)] = True
    return torch.from_numpy(pad).to(device), torch.from_numpy(valid).to(device)


def _problem(ppm_optimizer, state_init_list, state_real_list, actions):
    """the padded clouds, masks and pushes of :187-215, uploaded once"""
    device = ppm_optimizer.device
    rows = ppm_optimizer.task_config["max_nobj"]
    before, before_valid = _pad_clouds(state_init_list[:len(actions)], rows, device)
    after, after_valid = _pad_clouds(state_real_list[:len(actions)], rows, device)
    pushes = torch.from_numpy(np.stack(actions, axis=0).astype(np.float32))     # CPU: the decode runs on the host (bit-equal cos / sin)
    return before, before_valid, after, after_valid, pushes


def _as_param_dict(physics_param, ppm_optimizer):
    if isinstance(physics_param, (list, np.ndarray)):
        names = list(ppm_optimizer.material_dims.keys())
        assert len(names) == 1, "only support single material now"
        return {names[0]: torch.tensor(np.asarray(physics_param), dtype=torch.float32)}
    return copy.deepcopy(physics_param)


def dynamics_error(physics_param, ppm_optimizer, state_init_list, state_real_list, actions):
    """physics_param: a list / array of values for the single material (what gp_minimize / cma hand over, :183-186) or a
    {material: tensor} dict; state_*_list: per past interaction the observed cloud before / after the push; actions: the pushes.
    -> mean over the interactions of the masked chamfer distance between the predicted and the observed cloud (:219-226)."""
    device = ppm_optimizer.device
    physics_param = _as_param_dict(physics_param, ppm_optimizer)
    before, before_valid, after, after_valid, pushes = _problem(ppm_optimizer, state_init_list, state_real_list, actions)
    rolled = dynamics_masked(before, before_valid, pushes, ppm_optimizer.model, device, ppm_optimizer, physics_param=physics_param)
    return mean_chamfer(rolled["state_seqs"].detach(), after, before_valid, after_valid).mean()


@torch.no_grad()
def dynamics_error_sweep(physics_params, ppm_optimizer, state_init_list, state_real_list, actions, streams=4):
    """dynamics_error for a LIST of physics parameters - a CMA-ES population (`es.ask()` of optimize_cma's strategy, :125-175:
    its members are independent) or a sweep - in one go: (K,) float64 numpy, element k equal to
    dynamics_error(physics_params[k], ...) bit for bit.  The problem (padded clouds, masks, pushes) is uploaded once; evaluation k
    is enqueued on side stream k % streams without waiting for anything (dynamics_masked(_sync=False): an evaluation is <= 20
    small graphs, i.e. a chain of latency-bound launches that leaves the chip mostly idle - several of them run side by side on
    the context's per-stream call slots); one read-back at the end brings all chamfer values and overflow flags.  Raises
    Exception("Exceeds max dims") if any evaluation's graph exceeded max_nR, as the reference's dynamics_masked would have."""
    from .losses import chamfer
    device = torch.device(ppm_optimizer.device)
    before, before_valid, after, after_valid, pushes = _problem(ppm_optimizer, state_init_list, state_real_list, actions)
    K, n = len(physics_params), before.shape[0]
    if K == 0:
        return np.zeros(0, np.float64)
    errs = torch.empty((K, n), device=device, dtype=torch.float32)
    flags = torch.zeros((K, 2), device=device, dtype=torch.int32)
    cur = torch.cuda.current_stream(device)
    entry = torch.cuda.Event()
    entry.record(cur)
    side = _sweep_streams(device, max(1, min(int(streams), K)))
    for k, pp in enumerate(physics_params):
        st = side[k % len(side)]
        if k < len(side):
            st.wait_event(entry)
        with torch.cuda.stream(st):
            rolled = dynamics_masked(before, before_valid, pushes, ppm_optimizer.model, device, ppm_optimizer,
                                     physics_param=_as_param_dict(pp, ppm_optimizer), _sync=False, _overflow_flag=flags[k])
            errs[k] = chamfer(rolled["state_seqs"], after, before_valid, after_valid)
            rolled["state_seqs"].record_stream(st)
    for st in side:
        done = torch.cuda.Event()
        done.record(st)
        cur.wait_event(done)
    host = torch.cat([errs, flags.to(torch.float32)], 1).cpu().numpy()           # the one wait
    if (host[:, n] > float(ppm_optimizer.task_config["max_nR"])).any():
        raise Exception("Exceeds max dims")                                      # utils.py:63-65
    return host[:, :n].astype(np.float64).mean(1)                                # :225 on mean_chamfer's float64 array


PARAM_BOUNDS = (-0.2, 1.2)        # the reference's search space and clamp (physics_param_optimizer.py:69,103)


def _stacked_eval(params, ppm_optimizer, problem, want_grad=True):
    """The objective (and its gradient) at K parameter vectors at once.  params (K,dim) float array -> (errors (K,) float64,
    grads (K,dim) float64 or None).  The K evaluations are stacked into ONE batch of K * n rows (n = interactions) with a
    per-row parameter, so this is one masked rollout and one backward whatever K is.  Rows do not interact anywhere on the
    way (per-row kernels, fixed-order sums), and the per-start reductions below run in a fixed order on the host in float64:
    entry k carries the bits of evaluating params[k] alone."""
    device = torch.device(ppm_optimizer.device)
    before, before_valid, after, after_valid, pushes = problem
    names = list(ppm_optimizer.material_dims.keys())
    assert len(names) == 1, "only support single material now"
    params = np.asarray(params, np.float32)
    K, dim = params.shape
    assert dim == 1, "one value per start: the model takes one physics parameter per particle (model.py:92-95)"
    n = before.shape[0]
    rows = torch.from_numpy(np.repeat(params, n, axis=0)).to(device).requires_grad_(want_grad)      # (K*n, 1), start-major
    rep = lambda t: t.repeat(K, *([1] * (t.dim() - 1)))
    with torch.set_grad_enabled(want_grad):
        rolled = dynamics_masked_diff(rep(before), rep(before_valid), rep(pushes), ppm_optimizer.model, device, ppm_optimizer,
                                      physics_param={names[0]: rows})
        dist = chamfer_diff(rolled["state_seqs"], rep(after), rep(before_valid), rep(after_valid))   # (K*n,)
        if want_grad:
            dist.backward(torch.full_like(dist, 1.0 / n))                                   # d(mean over the interactions)
    errors = dist.detach().cpu().numpy().astype(np.float64).reshape(K, n).mean(1)          # :225 on mean_chamfer's float64 array
    if not want_grad:
        return errors, None
    g = rows.grad.cpu().numpy().astype(np.float64).reshape(K, n, dim)
    grads = g[:, 0].copy()
    for i in range(1, n):                                                                   # fixed order, whatever K
        grads += g[:, i]
    return errors, grads


def dynamics_error_grad(physics_param, ppm_optimizer, state_init_list, state_real_list, actions):
    """dynamics_error with its gradient: the arguments of dynamics_error -> (error, grad).  error: what dynamics_error returns
    (the step-by-step differentiable rollout instead of the fused one computes it: equal to rounding); grad: d error /
    d physics_param, float64 numpy, shaped like the parameter.  Beyond dynamics_error's list / (dim,) parameter, a (B,1) or
    (B,n_p) array or tensor gives every interaction / every particle its own value (B = len(actions), n_p = max_nobj).  Edges
    are constants of the gradient, as under the reference's autograd through its own dynamics_masked."""
    device = torch.device(ppm_optimizer.device)
    problem = _problem(ppm_optimizer, state_init_list, state_real_list, actions)
    physics_param = _as_param_dict(physics_param, ppm_optimizer)
    (name, value), = physics_param.items()
    value = value.detach().to("cpu", torch.float32)
    if value.dim() <= 1:
        errors, grads = _stacked_eval(value.reshape(1, -1).numpy(), ppm_optimizer, problem)
        return errors[0], grads[0].reshape(tuple(value.shape))
    before, before_valid, after, after_valid, pushes = problem
    n = before.shape[0]
    p = value.to(device).requires_grad_(True)
    rolled = dynamics_masked_diff(before, before_valid, pushes, ppm_optimizer.model, device, ppm_optimizer, physics_param={name: p})
    dist = chamfer_diff(rolled["state_seqs"], after, before_valid, after_valid)
    dist.backward(torch.full_like(dist, 1.0 / n))
    return dist.detach().cpu().numpy().astype(np.float64).mean(), p.grad.cpu().numpy().astype(np.float64)


def _starting_points(current, n_starts):
    """(n_starts, dim): the current parameter (clamped to the bounds) first, the rest at the centres of n_starts - 1 equal cells
    of the bounds, the same value in every dimension."""
    lo, hi = PARAM_BOUNDS
    cur = np.clip(np.asarray(current, np.float64).reshape(1, -1), lo, hi)
    k = max(0, int(n_starts) - 1)
    rest = lo + (hi - lo) * (np.arange(k) + 0.5) / max(k, 1)
    return np.concatenate([cur, np.repeat(rest[:, None], cur.shape[1], axis=1)], 0)


def optimize_grad(ppm_optimizer, actions, state_init_list, state_pred_list, state_real_list, iterations=50, n_starts=8, lr=0.05,
                  return_res=False):
    """Gradient counterpart of the reference's optimize (physics_param_optimizer.py:76-122): same argument order (state_pred_list
    is unused there too) and the same return tuple (physics_param (dim,) float32, error, init_error[, res]).  Adam (beta 0.9 /
    0.999, eps 1e-8) on the physics parameter, clamped after every step to the reference's bounds [-0.2, 1.2], from n_starts
    starting points at once (_starting_points: the current parameter first).  All starts are stacked into one batch
    (_stacked_eval), so an iteration is one rollout and one backward whatever n_starts is.  Every parameter it evaluates competes
    for the result, the starting points included, so the returned error never exceeds the lowest error among them (nor
    init_error, the current parameter's).

    lr = 0.05: Adam's step is about lr per iteration whatever the gradient's scale, so 50 iterations can cross the whole 1.4-wide
    interval (2.5) and the last steps, with the momentum averaged out, resolve a few 1e-3 - below what the objective distinguishes.
    res (return_res): {'params': (iterations+1, n_starts, dim), 'errors': (iterations+1, n_starts), 'best_start': k}."""
    if iterations < 0:
        iterations = 200                                                         # :78-79
    names = list(ppm_optimizer.material_dims.keys())
    assert len(names) == 1, "only support single material now"
    problem = _problem(ppm_optimizer, state_init_list, state_real_list, actions)
    current = ppm_optimizer.physics_param[names[0]].detach().to("cpu", torch.float64).numpy().reshape(-1)
    x = _starting_points(current, n_starts)
    if iterations == 0:
        return _stacked_eval(x[:1], ppm_optimizer, problem, want_grad=False)[0][0]   # :87-88
    m, v = np.zeros_like(x), np.zeros_like(x)
    best_x, best_err, best_k, init_error = None, np.inf, 0, None
    hist_x, hist_e = [], []
    for it in range(iterations + 1):
        last = it == iterations
        xe = x.astype(np.float32)                                                # what the engine evaluates is what is kept
        errors, grads = _stacked_eval(xe, ppm_optimizer, problem, want_grad=not last)
        if it == 0:
            init_error = errors[0]
        hist_x.append(xe.copy())
        hist_e.append(errors.copy())
        k = int(np.argmin(errors))
        if errors[k] < best_err:
            best_x, best_err, best_k = xe[k].copy(), errors[k], k
        if last:
            break
        m = 0.9 * m + 0.1 * grads
        v = 0.999 * v + 0.001 * grads * grads
        step = lr * (m / (1 - 0.9 ** (it + 1))) / (np.sqrt(v / (1 - 0.999 ** (it + 1))) + 1e-8)
        x = np.clip(xe.astype(np.float64) - step, *PARAM_BOUNDS)
    if return_res:
        return best_x, best_err, init_error, {"params": np.stack(hist_x), "errors": np.stack(hist_e), "best_start": best_k}
    return best_x, best_err, init_error


def adam_best_update(x32, errors, grads, m, v, it, lr, best):
    """One iteration of optimize_grad's loop body as the device kernel states it (ag_ppm_adam_step), on the host in float64:
    x32 (K,dim) float32 evaluated parameters, their errors (K,) and gradients (K,dim), Adam moments m, v, iteration it (0-based),
    best = (x, err, k) so far -> (new x32, m, v, best).  Pure host function (tests restate optimize_grad against it)."""
    errors = np.asarray(errors, np.float64)
    bx, be, bk = best
    for k in range(len(errors)):                                                 # ascending k: the first minimum wins
        if errors[k] < be:
            bx, be, bk = np.array(x32[k], np.float32, copy=True), errors[k], k
    m = 0.9 * m + 0.1 * grads
    v = 0.999 * v + 0.001 * grads * grads
    step = lr * (m / (1 - 0.9 ** (it + 1))) / (np.sqrt(v / (1 - 0.999 ** (it + 1))) + 1e-8)
    x = np.clip(np.asarray(x32, np.float32).astype(np.float64) - step, *PARAM_BOUNDS)
    return x.astype(np.float32), m, v, (bx, be, bk)


class _DeviceProblem:
    """The fit's problem on the device in the form ag_ppm_grad_step takes: K copies of the n interactions, interaction-major
    (row = i * K + k) with the interactions in descending order of action_repeat, so that every step of the call runs over
    exactly the rows that still have a forward left.  Uploaded once."""

    def __init__(self, ppm_optimizer, state_init_list, state_real_list, actions, K, sort=True):
        self.ppm, self.K = ppm_optimizer, int(K)
        task = ppm_optimizer.task_config
        self.dev = dev = _require_gpu(ppm_optimizer.device)
        model = ppm_optimizer.model
        if not isinstance(model, DynamicsPredictor):
            raise TypeError("model must be an adaptigraph_amd.DynamicsPredictor")
        assert int(task["n_his"]) == model.n_his, "task_config['n_his'] (forward_dynamics.py:16) must be the model's n_his"
        names = list(ppm_optimizer.material_dims.keys())
        assert len(names) == 1, "only support single material now"
        self.name = names[0]
        before, before_valid, after, after_valid, pushes = _problem(ppm_optimizer, state_init_list, state_real_list, actions)
        action_cpu = pushes[:, None]                                             # forward_dynamics.py:218
        decoded, repeat = decode_action(action_cpu, push_length=task["push_length"])
        xz, delta = _tool_layout(decoded, action_cpu[:, :, 2], task)
        self.n, self.N_o, self.M = before.shape[0], before.shape[1], ppm_optimizer.eef_num
        assert xz.shape[2] == self.M
        rep = repeat[:, 0].to(torch.int64).numpy()
        self.order = np.argsort(-rep, kind="stable") if sort else np.arange(self.n)   # row block j holds interaction order[j]
        idx = torch.from_numpy(np.repeat(self.order, self.K))
        take = lambda t: t.to(dev)[idx.to(dev)].contiguous()                      # noqa: E731
        self.state0, self.obs = take(before), take(after)
        self.obj_mask, self.obs_mask = take(before_valid).view(torch.uint8), take(after_valid).view(torch.uint8)
        self.xz, self.delta = take(xz[:, 0].to(torch.float32)), take(delta[:, 0].to(torch.float32))
        self.h_repeat = np.ascontiguousarray(rep[np.repeat(self.order, self.K)].astype(np.int32))
        self.d_repeat = torch.from_numpy(self.h_repeat).to(dev)
        self.R, self.N_t = self.n * self.K, after.shape[1]
        self.row_w = torch.full((self.R,), 1.0 / self.n, device=dev, dtype=torch.float32)   # d(mean over the interactions)
        self.w = [p.detach() for p in model.ordered_parameters()]
        for t in self.w:
            assert t.device == dev and t.dtype == torch.float32 and t.is_contiguous(), "model parameters must be fp32 on the device"
        self._w_arr = _vp_array(self.w)
        self.seqs = torch.empty((self.R, self.N_o, 3), device=dev, dtype=torch.float32)
        self.err = torch.empty((self.R,), device=dev, dtype=torch.float32)
        self.grad = torch.zeros((self.R, self.N_o), device=dev, dtype=torch.float32)
        self.max_nR = int(task["max_nR"])
        self.edge_rows = None

    def run(self, phys, status, want_grad):
        """enqueue ag_ppm_grad_step on the current stream: phys (R,N_o) device fp32 -> self.seqs, self.err, self.grad"""
        ppm, task, dev = self.ppm, self.ppm.task_config, self.dev
        eng = ppm.model.engine(dev)
        N = self.N_o + self.M
        k = min(N, int(task["topk"]))
        bound = N * (k + self.M) if k < N else N * N                              # the builder's structural bound
        edge_rows = int(self.edge_rows) if self.edge_rows is not None else bound
        p = _rollout_params(task, ppm, ppm.model, self.R, 1, self.N_o, 1, 0.0)
        p.max_nR = int(self.max_nR)                                               # the attribute, which may have moved since
        eng.check(eng.lib.ag_ppm_grad_step(
            eng.ctx, current_stream(dev), C.byref(p), ptr(self.state0), ptr(self.obj_mask), ptr(self.xz), ptr(self.delta),
            C.c_void_p(self.h_repeat.ctypes.data), ptr(self.d_repeat), ptr(phys), ptr(self.obs), ptr(self.obs_mask), self.N_t,
            ptr(self.row_w), self._w_arr, max(1, edge_rows), int(want_grad), ptr(self.seqs), ptr(self.err), ptr(self.grad),
            ptr(status)))
        return eng


class PhysParamFit:
    """optimize_grad's iteration resident on the GPU.  fit = PhysParamFit(ppm_optimizer, actions, state_init_list,
    state_real_list, n_starts=8, lr=0.05); fit.step() x iterations; fit.evaluate(); best, err, init_err = fit.result().

    The problem is uploaded and stacked n_starts-fold once.  step() enqueues ag_ppm_grad_step (masked rollout, chamfer, backward
    toward the parameter) and ag_ppm_adam_step (per-start reduction, history, best-so-far, Adam in double, clamp) and returns:
    nothing between two iterations waits for the GPU, neither the parameter nor its gradient passes through the host.  Parameter,
    Adam moments, history and the status words live on the device for the life of the object.  iterations: rows of the device
    history beyond the first (evaluations past it still compete for the result, they are just not recorded).  starts: (K,dim)
    starting points instead of optimize_grad's _starting_points.  max_nR (attribute, from the task config) may be changed between
    steps; edge_rows (attribute, None = the builder's structural bound) bounds the edge rows of the backward workspace."""

    def __init__(self, ppm_optimizer, actions, state_init_list, state_real_list, n_starts=8, lr=0.05, iterations=50, starts=None):
        names = list(ppm_optimizer.material_dims.keys())
        assert len(names) == 1, "only support single material now"
        if starts is None:
            current = ppm_optimizer.physics_param[names[0]].detach().to("cpu", torch.float64).numpy().reshape(-1)
            starts = _starting_points(current, n_starts)
        x = np.asarray(starts, np.float64).astype(np.float32)
        assert x.ndim == 2 and x.shape[1] == 1, "one value per start: the model takes one physics parameter per particle (model.py:92-95)"
        self.K, self.dim, self.lr = x.shape[0], x.shape[1], float(lr)
        self.problem = pr = _DeviceProblem(ppm_optimizer, state_init_list, state_real_list, actions, self.K)
        dev = self.device = pr.dev
        self.hist_cap = max(1, int(iterations) + 1)
        self.x = torch.from_numpy(x[:, 0].copy()).to(dev)
        self.exp_avg = torch.zeros(self.K, device=dev, dtype=torch.float64)
        self.exp_avg_sq = torch.zeros(self.K, device=dev, dtype=torch.float64)
        self.hist_x = torch.zeros((self.hist_cap, self.K), device=dev, dtype=torch.float32)
        self.hist_err = torch.zeros((self.hist_cap, self.K), device=dev, dtype=torch.float64)
        self.best = torch.tensor([np.inf, 0.0, 0.0, np.inf], device=dev, dtype=torch.float64)
        self.last_grad = torch.zeros(self.K, device=dev, dtype=torch.float64)      # per start, of the latest step()
        self.phys = self.x[None, :, None].expand(pr.n, self.K, pr.N_o).reshape(pr.R, pr.N_o).contiguous()
        self._status = torch.zeros(4, dtype=torch.int32, device=dev)               # [0] overflow flag, [1] evaluations, [2] updates
        self._step = 0                                                              # host counter of enqueued evaluations
        self._updates = 0                                                           # ... of enqueued Adam updates (bias corrections)

    max_nR = property(lambda self: self.problem.max_nR, lambda self, v: setattr(self.problem, "max_nR", int(v)))
    edge_rows = property(lambda self: self.problem.edge_rows, lambda self, v: setattr(self.problem, "edge_rows", v))

    def _run(self, apply):
        pr = self.problem
        eng = pr.run(self.phys, self._status, want_grad=apply)
        it = self._updates                                                          # evaluate() in between does not count
        eng.check(eng.lib.ag_ppm_adam_step(
            eng.ctx, current_stream(self.device), ptr(pr.err), ptr(pr.grad) if apply else None, self.K, pr.n, pr.N_o, 0, int(apply),
            self.lr, 1.0 - 0.9 ** (it + 1), 1.0 - 0.999 ** (it + 1), PARAM_BOUNDS[0], PARAM_BOUNDS[1], ptr(self.x), ptr(self.exp_avg),
            ptr(self.exp_avg_sq), self.hist_cap, ptr(self.hist_x), ptr(self.hist_err), ptr(self.best), ptr(self.last_grad),
            ptr(self.phys), ptr(self._status)))
        self._step += 1
        self._updates += int(apply)

    def step(self):
        """One iteration: evaluate the current parameters with their gradient, record, Adam.  Enqueue only.  An iteration with a
        graph beyond max_nR is skipped on the device - parameters, moments and history stay - as is every following one until
        result() has reported it."""
        self._run(True)

    def evaluate(self):
        """Forward and loss only at the current parameters: recorded and competing for the result, no update.  Enqueue only."""
        self._run(False)

    def result(self, return_res=False):
        """The one read-back (waits for what was enqueued): (physics_param (dim,) float32, error, init_error[, res]) as
        optimize_grad returns them.  Raises Exception("Exceeds max dims"), as the reference's dynamics_masked does, when an
        evaluation since the last result() was skipped; the counters are then back at the recorded evaluations and applied
        updates and the flag is cleared, so the object is where it was before the first skipped step."""
        host = torch.cat([self._status.to(torch.float64), self.best, self.hist_x.reshape(-1).to(torch.float64),
                          self.hist_err.reshape(-1)]).cpu().numpy()
        if host[0] != 0:
            self._step, self._updates = int(host[1]), int(host[2])
            self._status[0] = 0
            raise Exception("Exceeds max dims")                                   # src/dynamics/utils.py:63-65
        n = min(int(host[1]), self.hist_cap)
        best_x = np.full((self.dim,), host[5], np.float32)
        if not return_res:
            return best_x, host[4], host[7]
        hk = self.hist_cap * self.K
        params = host[8:8 + hk].astype(np.float32).reshape(self.hist_cap, self.K, 1)[:n]
        errors = host[8 + hk:8 + 2 * hk].reshape(self.hist_cap, self.K)[:n].copy()
        return best_x, host[4], host[7], {"params": params, "errors": errors, "best_start": int(host[6])}


def optimize_grad_device(ppm_optimizer, actions, state_init_list, state_pred_list, state_real_list, iterations=50, n_starts=8,
                         lr=0.05, return_res=False):
    """optimize_grad on PhysParamFit: the same arguments, starting points, Adam, clamp, rule that every evaluated parameter
    competes for the result, and return tuple - but an iteration only enqueues and the result is read back once at the end."""
    if iterations < 0:
        iterations = 200                                                         # :78-79
    if iterations == 0:
        fit = PhysParamFit(ppm_optimizer, actions, state_init_list, state_real_list, n_starts=1, lr=lr, iterations=0)
        fit.evaluate()
        return fit.result()[1]                                                   # :87-88
    fit = PhysParamFit(ppm_optimizer, actions, state_init_list, state_real_list, n_starts=n_starts, lr=lr, iterations=iterations)
    for _ in range(iterations):
        fit.step()
    fit.evaluate()
    return fit.result(return_res)


def dynamics_error_grad_device(physics_param, ppm_optimizer, state_init_list, state_real_list, actions, _out=None):
    """dynamics_error_grad through ONE ag_ppm_grad_step: the same arguments ((dim,), (B,1) or (B,n_p) parameter) and the same
    (error, grad) - float64, the gradient shaped like the parameter.  Raises Exception("Exceeds max dims") like it.
    _out: a dict that receives the captured 'state_seqs' (B,n_p,3) and the per-row 'chamfer' (B,) as device tensors (tests)."""
    pr = _DeviceProblem(ppm_optimizer, state_init_list, state_real_list, actions, 1, sort=False)
    physics_param = _as_param_dict(physics_param, ppm_optimizer)
    (name, value), = physics_param.items()
    value = value.detach().to("cpu", torch.float32)
    shape = tuple(value.shape)
    if value.dim() <= 1:
        assert value.numel() == 1, "one value: the model takes one physics parameter per particle (model.py:92-95)"
        rows = value.reshape(1, 1).expand(pr.n, pr.N_o)
    else:
        assert value.shape[0] == pr.n and value.shape[1] in (1, pr.N_o), \
            f"physics parameter of shape {shape}: expected (dim,), ({pr.n}, 1) or ({pr.n}, {pr.N_o})"
        rows = value.expand(pr.n, pr.N_o)
    phys = rows.contiguous().to(pr.dev)
    status = torch.zeros(4, dtype=torch.int32, device=pr.dev)
    pr.run(phys, status, want_grad=True)
    host = torch.cat([status.to(torch.float32), pr.err, pr.grad.reshape(-1)]).cpu().numpy()   # the one wait
    if host[0] != 0:
        raise Exception("Exceeds max dims")                                       # utils.py:63-65
    if _out is not None:
        _out.update(state_seqs=pr.seqs, chamfer=pr.err)
    error = host[4:4 + pr.n].astype(np.float64).mean()
    g = host[4 + pr.n:].astype(np.float64).reshape(pr.n, pr.N_o)
    if value.dim() <= 1:
        col = g[:, 0].copy()
        for i in range(1, pr.N_o):                                               # fixed order
            col += g[:, i]
        total = col[0]
        for i in range(1, pr.n):
            total += col[i]
        return error, np.full(shape, total, np.float64)
    if value.shape[1] == 1:
        col = g[:, 0].copy()
        for i in range(1, pr.N_o):
            col += g[:, i]
        return error, col.reshape(pr.n, 1)
    return error, g
