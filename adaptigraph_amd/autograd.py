"""Differentiable DynamicsPredictor forward: a torch.autograd.Function around ag_forward / ag_backward.

The forward is ag_forward itself (same kernels, same bits as the no-grad path).  The backward (ag_backward, ag_train.hip)
recomputes the activations it needs and returns dLoss/dstate and the gradients of the 22 parameters, exact fp32 whatever the
forward precision.  attrs, action, p_instance and the physics parameter are data: the model refuses them with requires_grad.

DynamicsDiffFunction (DynamicsPredictor.forward_diff) is the same forward with ag_backward_inputs as its backward: it also
returns dLoss/daction and dLoss/dphys, the two data gradients the physics-parameter fit needs.  attrs and p_instance stay data.
"""
from __future__ import annotations

import ctypes as C

import torch

from .context import ptr, current_stream


def _vp_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else 0 for t in ts])


class DynamicsFunction(torch.autograd.Function):
    """apply(eng, edges, n_p, state, attrs, action, phys, group, *params) -> (pred_pos, pred_motion).

    params: the 22 parameter tensors in ag_ctx_load_weights order (context.STATE_DICT_ORDER, weight then bias); the engine
    must already hold exactly these values (DynamicsPredictor.engine() uploads them)."""

    @staticmethod
    def forward(ctx, eng, edges, n_p, state, attrs, action, phys, group, *params):
        dev = state.device
        B, N = attrs.shape[0], attrs.shape[1]
        n_inst = group.shape[2]
        pred_pos = torch.empty((B, n_p, 3), device=dev, dtype=torch.float32)
        pred_motion = torch.empty((B, n_p, 3), device=dev, dtype=torch.float32)
        eng.check(eng.lib.ag_forward(eng.ctx, current_stream(dev), ptr(state), ptr(attrs), ptr(action), ptr(phys),
                                     ptr(group), n_inst, ptr(edges.recv), ptr(edges.send), ptr(edges.row_ptr),
                                     ptr(edges.n_edges), edges.edge_cap, B, N, n_p, ptr(pred_pos), ptr(pred_motion)))
        ctx.eng, ctx.edges, ctx.n_p = eng, edges, n_p
        ctx.save_for_backward(state, attrs, action, phys, group, *params)
        return pred_pos, pred_motion

    @staticmethod
    def backward(ctx, g_pos, g_motion):
        state, attrs, action, phys, group, *params = ctx.saved_tensors
        eng, edges, n_p = ctx.eng, ctx.edges, ctx.n_p
        dev = state.device
        B, N = attrs.shape[0], attrs.shape[1]
        need_state = ctx.needs_input_grad[3]
        need_w = ctx.needs_input_grad[8:]
        w_dev = [p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in params]
        g_w = [torch.empty_like(w) if need else None for w, need in zip(w_dev, need_w)]
        g_state = torch.empty_like(state) if need_state else None
        g_pos = g_pos.to(torch.float32).contiguous() if g_pos is not None else None
        g_motion = g_motion.to(torch.float32).contiguous() if g_motion is not None else None
        eng.check(eng.lib.ag_backward(eng.ctx, current_stream(dev), ptr(state), ptr(attrs), ptr(action), ptr(phys),
                                      ptr(group), group.shape[2], ptr(edges.recv), ptr(edges.send), ptr(edges.row_ptr),
                                      ptr(edges.n_edges), edges.edge_cap, B, N, n_p, _vp_array(w_dev), ptr(g_pos),
                                      ptr(g_motion), ptr(g_state), _vp_array(g_w)))
        g_params = [g.to(p.device) if g is not None else None for g, p in zip(g_w, params)]
        return (None, None, None, g_state, None, None, None, None, *g_params)


class DynamicsDiffFunction(torch.autograd.Function):
    """DynamicsFunction with gradients toward action (B,N,3) and phys (B,N) as well (ag_backward_inputs).  Same arguments."""

    @staticmethod
    def forward(ctx, eng, edges, n_p, state, attrs, action, phys, group, *params):
        return DynamicsFunction.forward(ctx, eng, edges, n_p, state, attrs, action, phys, group, *params)

    @staticmethod
    def backward(ctx, g_pos, g_motion):
        state, attrs, action, phys, group, *params = ctx.saved_tensors
        eng, edges, n_p = ctx.eng, ctx.edges, ctx.n_p
        dev = state.device
        B, N = attrs.shape[0], attrs.shape[1]
        need_state, need_action, need_phys = ctx.needs_input_grad[3], ctx.needs_input_grad[5], ctx.needs_input_grad[6]
        need_w = ctx.needs_input_grad[8:]
        w_dev = [p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in params]
        g_w = [torch.empty_like(w) if need else None for w, need in zip(w_dev, need_w)]
        g_state = torch.empty_like(state) if need_state else None
        g_action = torch.empty_like(action) if need_action else None
        g_phys = torch.empty_like(phys) if need_phys else None
        g_pos = g_pos.to(torch.float32).contiguous() if g_pos is not None else None
        g_motion = g_motion.to(torch.float32).contiguous() if g_motion is not None else None
        eng.check(eng.lib.ag_backward_inputs(eng.ctx, current_stream(dev), ptr(state), ptr(attrs), ptr(action), ptr(phys),
                                             ptr(group), group.shape[2], ptr(edges.recv), ptr(edges.send), ptr(edges.row_ptr),
                                             ptr(edges.n_edges), edges.edge_cap, B, N, n_p, _vp_array(w_dev), ptr(g_pos),
                                             ptr(g_motion), ptr(g_state), _vp_array(g_w), ptr(g_phys), ptr(g_action)))
        g_params = [g.to(p.device) if g is not None else None for g, p in zip(g_w, params)]
        return (None, None, None, g_state, None, g_action, g_phys, None, *g_params)
