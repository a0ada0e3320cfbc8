"""Differentiable DynamicsPredictor forward: a torch.autograd.Function around ag_forward / ag_backward.

The forward is ag_forward itself (same kernels, same bits as the no-grad path).  The backward (ag_backward, ag_train.hip)
recomputes the activations it needs and returns dLoss/dstate and the gradients of the 22 parameters, exact fp32 whatever the
forward precision.  attrs, action, p_instance and the physics parameter are data: the model refuses them with requires_grad.

DynamicsDiffFunction (DynamicsPredictor.forward_diff) is the same forward with ag_backward_inputs as its backward: it also
returns dLoss/daction and dLoss/dphys, the two data gradients the physics-parameter fit needs.  attrs and p_instance stay data.
"""
from __future__ import annotations

import torch

from .context import ptr, current_stream, _vp_array
from .marshal import ModelInputs


def forward_call(eng, inp):
    """ag_forward on a ModelInputs -> (pred_pos, pred_motion), both (B, n_p, 3)."""
    dev = inp.state.device
    pred_pos = torch.empty((inp.B, inp.n_p, 3), device=dev, dtype=torch.float32)
    pred_motion = torch.empty((inp.B, inp.n_p, 3), device=dev, dtype=torch.float32)
    eng.check(eng.lib.ag_forward(eng.ctx, current_stream(dev), *inp.c_args(), ptr(pred_pos), ptr(pred_motion)))
    return pred_pos, pred_motion


def _backward(ctx, g_pos, g_motion, inputs):
    """ag_backward; inputs: ag_backward_inputs, which also returns the gradients toward action and phys where they are needed."""
    state, attrs, action, phys, group, *params = ctx.saved_tensors
    inp = ModelInputs(state, attrs, action, phys, group, ctx.edges, ctx.n_p)
    eng, dev, need = ctx.eng, state.device, ctx.needs_input_grad
    w_dev = [p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in params]
    g_w = [torch.empty_like(w) if n else None for w, n in zip(w_dev, need[8:])]
    g_state = torch.empty_like(state) if need[3] else None
    g_action = torch.empty_like(action) if inputs and need[5] else None
    g_phys = torch.empty_like(phys) if inputs and need[6] else None
    g_pos = g_pos.to(torch.float32).contiguous() if g_pos is not None else None
    g_motion = g_motion.to(torch.float32).contiguous() if g_motion is not None else None
    args = (eng.ctx, current_stream(dev), *inp.c_args(), _vp_array(w_dev), ptr(g_pos), ptr(g_motion), ptr(g_state), _vp_array(g_w))
    eng.check(eng.lib.ag_backward_inputs(*args, ptr(g_phys), ptr(g_action)) if inputs else eng.lib.ag_backward(*args))
    g_params = [g.to(p.device) if g is not None else None for g, p in zip(g_w, params)]
    return (None, None, None, g_state, None, g_action, g_phys, None, *g_params)


class DynamicsFunction(torch.autograd.Function):
    """apply(eng, edges, n_p, state, attrs, action, phys, group, *params) -> (pred_pos, pred_motion).

    params: the 22 parameter tensors in ag_ctx_load_weights order (context.STATE_DICT_ORDER, weight then bias); the engine
    must already hold exactly these values (DynamicsPredictor.engine() uploads them)."""

    @staticmethod
    def forward(ctx, eng, edges, n_p, state, attrs, action, phys, group, *params):
        out = forward_call(eng, ModelInputs(state, attrs, action, phys, group, edges, n_p))
        ctx.eng, ctx.edges, ctx.n_p = eng, edges, n_p
        ctx.save_for_backward(state, attrs, action, phys, group, *params)
        return out

    @staticmethod
    def backward(ctx, g_pos, g_motion):
        return _backward(ctx, g_pos, g_motion, inputs=False)


class DynamicsDiffFunction(torch.autograd.Function):
    """DynamicsFunction with gradients toward action (B,N,3) and phys (B,N) as well (ag_backward_inputs).  Same arguments."""

    @staticmethod
    def forward(ctx, eng, edges, n_p, state, attrs, action, phys, group, *params):
        return DynamicsFunction.forward(ctx, eng, edges, n_p, state, attrs, action, phys, group, *params)

    @staticmethod
    def backward(ctx, g_pos, g_motion):
        return _backward(ctx, g_pos, g_motion, inputs=True)
