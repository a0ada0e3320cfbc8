"""DynamicsPredictor with the reference's constructor / forward / state_dict surface
(src/dynamics/gnn/model.py:64-342), executing on the HIP engine.

The nn.Module tree exists only so that state_dict keys, load_state_dict, .to() and .eval() behave like the reference;
no torch op of it is ever run - forward() hands raw device pointers to the C-ABI.  With grad enabled and the parameters or
`state` requiring grad, forward() runs through autograd.DynamicsFunction (ag_forward + ag_backward); otherwise it is the
inference path.  forward_diff() is the same forward, differentiable toward `action` and the physics parameter as well
(ag_backward_inputs): the entry of the gradient-based physics-parameter fit; forward() keeps refusing data gradients.  Parameters are frozen after construction; train(True) unfreezes them and train(False) / eval() freezes them.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .autograd import DynamicsFunction, DynamicsDiffFunction, forward_call
from .context import Engine, _require_gpu, STATE_DICT_ORDER
from .graph import EdgeList
from .marshal import ModelInputs


def _mlp3(n_in, n_hidden, n_out):
    # same parameter names as the reference's Encoder.model (indices 0, 2, 4 are the Linear layers)
    return nn.Sequential(nn.Linear(n_in, n_hidden), nn.ReLU(), nn.Linear(n_hidden, n_hidden), nn.ReLU(),
                         nn.Linear(n_hidden, n_out), nn.ReLU())


class _ExpandRows(torch.autograd.Function):
    """(B,1) -> (B,n_p), model.py:191-197.  Backward: the sum over the n_p columns in float64, rounded once - a row's gradient
    then does not depend on how torch would tile an fp32 reduction for the batch the row sits in."""

    @staticmethod
    def forward(ctx, pp, n_p):
        return pp.expand(pp.shape[0], n_p).contiguous()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.float64).sum(1, keepdim=True).to(torch.float32), None


class _Holder(nn.Module):
    pass


class DynamicsPredictor(nn.Module):
    def __init__(self, model_config, material_config, dataset_config, device):
        super().__init__()
        self.model_config = model_config
        self.material_config = material_config
        self.dataset_config = dataset_config
        self.device = torch.device(device)
        self.n_his = dataset_config["n_his"]
        self.nf_particle = model_config["nf_particle"]
        self.nf_relation = model_config["nf_relation"]
        self.nf_effect = model_config["nf_effect"]
        self.eps = 1e-6
        self.motion_clamp = 100
        self.num_materials = len(material_config["material_index"])
        assert self.num_materials == 1, "Only support single material."          # model.py:89
        material_params = material_config[dataset_config["materials"][0]]["physics_params"]
        material_dim = sum(1 for p in material_params if p["use"])               # model.py:92-95
        input_dim = (self.n_his * model_config["state_dim"] + self.n_his * model_config["offset_dim"] +
                     model_config["attr_dim"] + model_config["action_dim"] + model_config["density_dim"] +
                     material_dim)                                               # model.py:97-102
        rel_particle_dim = model_config["rel_particle_dim"]
        if rel_particle_dim == -1:
            rel_particle_dim = input_dim
        rel_input_dim = (rel_particle_dim * 2 + model_config["rel_attr_dim"] * 2 + model_config["rel_group_dim"] +
                         model_config["rel_distance_dim"] * self.n_his + model_config["rel_density_dim"])
        if model_config["offset_dim"] > 0:
            raise NotImplementedError                                            # model.py:181-182
        unsupported = (model_config["state_dim"] != 0 or model_config["density_dim"] != 0 or
                       rel_particle_dim != 0 or model_config["rel_density_dim"] != 0 or
                       model_config["attr_dim"] != 2 or model_config["action_dim"] != 3 or material_dim != 1 or
                       model_config["rel_attr_dim"] != 2 or model_config["rel_group_dim"] != 1 or
                       model_config["rel_distance_dim"] != 3)
        if unsupported or input_dim != 6 or self.n_his not in (4, 5) or rel_input_dim != 5 + 3 * self.n_his or \
                not (self.nf_particle == self.nf_relation == self.nf_effect == 150):
            raise NotImplementedError(
                "the HIP kernels are built for input_dim 6, nf 150 and n_his 4 (rel_input_dim 17: config/dynamics/"
                "{rope,granular,cloth,...}.yaml) or n_his 5 (rel_input_dim 20: softbody.yaml) - got "
                f"{input_dim}, {self.nf_effect}, {self.n_his}, {rel_input_dim}")
        self.input_dim, self.rel_input_dim = input_dim, rel_input_dim

        nf = self.nf_effect
        self.particle_encoder = _Holder()
        self.particle_encoder.model = _mlp3(input_dim, self.nf_particle, nf)
        self.relation_encoder = _Holder()
        self.relation_encoder.model = _mlp3(rel_input_dim, self.nf_relation, nf)
        self.particle_propagator = _Holder()
        self.particle_propagator.linear = nn.Linear(nf * 2, nf)
        self.relation_propagator = _Holder()
        self.relation_propagator.linear = nn.Linear(nf * 3, nf)
        self.non_rigid_predictor = _Holder()
        self.non_rigid_predictor.linear_0 = nn.Linear(nf, nf)
        self.non_rigid_predictor.linear_1 = nn.Linear(nf, nf)
        self.non_rigid_predictor.linear_2 = nn.Linear(nf, 3)
        for p in self.parameters():
            p.requires_grad_(False)
        self._engine = None
        self._uploaded_key = None
        self._precision = None       # None: the engine default (exact fp32, or AG_PRECISION)

    def train(self, mode=True):
        """nn.Module.train, and also requires_grad = mode on the 22 parameters (the reference's train.py calls model.train()
        before each train phase and model.eval() before each valid phase).  requires_grad_() keeps working directly."""
        super().train(mode)
        for p in self.parameters():
            p.requires_grad_(bool(mode))
        return self

    def ordered_parameters(self):
        """The 22 parameters in ag_ctx_load_weights order."""
        mods = dict(self.named_modules())
        return [getattr(mods[base], s) for base in STATE_DICT_ORDER for s in ("weight", "bias")]

    # ------------------------------------------------------------------ engine / weights
    def set_precision(self, mode):
        """'fp32': exact fp32 MFMA (default).  'bf16x3': 3-way bf16 split on the bf16 matrix pipe with fp32 accumulation
        - fp32-grade accuracy (same 1e-5 parity bar, tests/test_gpu_more.py), 1.32x faster end to end (BENCH_r02: 360.6 vs
        476.8 ms per 1024 x 20 cloth rollout)."""
        assert mode in ("fp32", "bf16x3")
        self._precision = mode
        if self._engine is not None:
            self._engine.set_precision(mode)

    def engine(self, device=None):
        dev = _require_gpu(device if device is not None else self.device)
        if self._engine is None or self._engine.device != dev:
            self._engine = Engine(dev, pstep=self.model_config["pstep"], n_his=self.n_his, rel_dim=self.rel_input_dim,
                                  motion_clamp=float(self.motion_clamp))
            self._uploaded_key = None
            if self._precision is not None:
                self._engine.set_precision(self._precision)
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if key != self._uploaded_key:
            self._engine.load_state_dict_tensors(self.state_dict())
            self._uploaded_key = key
        return self._engine

    # ------------------------------------------------------------------ forward (model.py:130-342)
    def forward(self, state, attrs, Rr=None, Rs=None, p_instance=None, action=None, particle_den=None, obj_mask=None,
                edges: EdgeList | None = None, **kwargs):
        params = self.ordered_parameters()
        data = [attrs, p_instance, action, Rr, Rs] + [v for k, v in kwargs.items() if k.endswith("_physics_param")]
        if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in [state, *params, *data]):
            return self._forward_grad(state, attrs, Rr, Rs, p_instance, action, edges, params, kwargs)
        with torch.no_grad():
            return self._forward_nograd(state, attrs, Rr, Rs, p_instance, action, edges, kwargs)

    def _inputs(self, dev, state, attrs, Rr, Rs, p_instance, action, edges, kwargs, diff=False):
        """ModelInputs from forward()'s arguments (model.py:152-282 on the host side): the physics parameter per particle, the
        group matrix, dense Rr / Rs as an EdgeList, all fp32 and contiguous on `dev`.  diff: action and the physics parameter stay
        under the caller's autograd ((B,1) expands through _ExpandRows); else they are data, like attrs, p_instance and the edges.
        state follows the caller's autograd either way."""
        B, N = attrs.size(0), attrs.size(1)
        n_p, n_inst = p_instance.size(1), p_instance.size(2)
        n_s = N - n_p
        with torch.set_grad_enabled(diff and torch.is_grad_enabled()):
            physics_keys = [k for k in kwargs.keys() if k.endswith("_physics_param")]
            assert len(physics_keys) == 1                                        # model.py:186-187
            pp = kwargs[physics_keys[0]].to(device=dev, dtype=torch.float32)
            if pp.size(-1) == 1:                                                 # model.py:191-197
                pp = _ExpandRows.apply(pp.reshape(B, 1), n_p) if diff else pp.reshape(B, 1).repeat(1, n_p)
            else:
                pp = pp.reshape(B, n_p)                                          # model.py:204
            phys = torch.cat([pp, torch.zeros(B, n_s, device=dev)], 1).contiguous()   # model.py:206-207
            assert action is not None                                            # model.py:222
            action = action.to(device=dev, dtype=torch.float32).contiguous()
        with torch.no_grad():
            group = torch.cat([p_instance.to(torch.float32), torch.zeros(B, n_s, n_inst, device=dev)], 1).contiguous()
            if edges is None:
                assert Rr is not None and Rs is not None
                edges = EdgeList.from_dense(Rr, Rs)
            attrs = attrs.to(torch.float32).contiguous()
        assert edges.N == N
        state = state.to(device=dev, dtype=torch.float32).contiguous()
        assert state.shape == (B, self.n_his, N, 3)
        return ModelInputs(state, attrs, action, phys, group, edges, n_p)

    def _forward_grad(self, state, attrs, Rr, Rs, p_instance, action, edges, params, kwargs):
        data = [("attrs", attrs), ("p_instance", p_instance), ("action", action), ("Rr", Rr), ("Rs", Rs)]
        data += [(k, v) for k, v in kwargs.items() if k.endswith("_physics_param")]
        for name, t in data:
            if torch.is_tensor(t) and t.requires_grad:
                raise NotImplementedError(f"DynamicsPredictor: gradient with respect to {name} is not implemented (gradients "
                                          "reach state and the parameters only)")
        dev = _require_gpu(state.device)
        eng = self.engine(dev)
        inp = self._inputs(dev, state, attrs, Rr, Rs, p_instance, action, edges, kwargs)
        return DynamicsFunction.apply(eng, inp.edges, inp.n_p, inp.state, inp.attrs, inp.action, inp.phys, inp.group, *params)

    def forward_diff(self, state, attrs, Rr=None, Rs=None, p_instance=None, action=None, particle_den=None, obj_mask=None,
                     edges: EdgeList | None = None, **kwargs):
        """forward() with gradients toward state, action, the physics parameter ((B,1) or (B,n_p), model.py:186-207) and, where
        they require grad, the parameters: same kernels and bits forward, ag_backward_inputs backward.  The (B,N) gradient of the
        per-particle parameter comes back in the caller's shape: (B,1) is the sum over the n_p object rows in a fixed order.
        attrs and p_instance are data: NotImplementedError if they require grad.  Edges are constants."""
        for name, t in (("attrs", attrs), ("p_instance", p_instance), ("Rr", Rr), ("Rs", Rs)):
            if torch.is_tensor(t) and t.requires_grad:
                raise NotImplementedError(f"DynamicsPredictor.forward_diff: gradient with respect to {name} is not implemented "
                                          "(gradients reach state, action, the physics parameter and the parameters)")
        params = self.ordered_parameters()
        dev = _require_gpu(state.device)
        eng = self.engine(dev)
        inp = self._inputs(dev, state, attrs, Rr, Rs, p_instance, action, edges, kwargs, diff=True)
        return DynamicsDiffFunction.apply(eng, inp.edges, inp.n_p, inp.state, inp.attrs, inp.action, inp.phys, inp.group, *params)

    def _forward_nograd(self, state, attrs, Rr, Rs, p_instance, action, edges, kwargs):
        dev = _require_gpu(state.device)
        eng = self.engine(dev)
        return forward_call(eng, self._inputs(dev, state, attrs, Rr, Rs, p_instance, action, edges, kwargs))
