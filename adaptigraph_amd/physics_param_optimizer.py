"""dynamics_error: the objective the online physics-parameter optimiser evaluates for every BO / CMA-ES proposal
(reference src/planning/physics_param_optimizer.py:178-226) = masked rollout of the past interactions + mean chamfer
to what really happened.  Same signature; dynamics_masked and mean_chamfer run on the HIP engine.  The host optimisers
(skopt.gp_minimize / cma) stay in the reference.  r05: dynamics_error_sweep evaluates a population / sweep of
parameters in one go (independent evaluations dealt to streams, one read-back)."""
from __future__ import annotations

import copy

import numpy as np
import torch

from .context import side_streams as _sweep_streams
from .forward_dynamics import dynamics_masked, dynamics_masked_diff
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
