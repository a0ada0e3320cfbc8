"""TrainStep: the reference's training iteration (src/dynamics/train/train.py:86-124) resident on the GPU.

step() enqueues ag_train_step (n_future chained forwards, MSE, next-state assembly, backward through the chain) and ag_adam_step
(torch.optim.Adam's formula over the 22 tensors, then the device re-pack of the engine's weight images) and returns: nothing
between two iterations waits for the GPU, no weight travels through the host.  Master weights, Adam's m and v, the gradients and
the status words live on the device for the life of the object.  The autograd path (DynamicsPredictor.forward + loss.backward()
+ torch.optim) is untouched; this is a second way next to it.

One optimiser step may also be built from PARTS (accumulate ... apply, or step_parts): micro-batches of one rank, buckets of a
mixed-size batch with a tight max_edges each, or the shards of a data-parallel batch (group=).  Every part runs
ag_train_step_part with the row count of the WHOLE step as the MSE denominator, so its loss and gradients are its share of the
full batch's (MSELoss is a mean over B * n_p * 3 and n_p is the same in every part: loss = sum over parts of B_part / B_total *
loss_part, exactly); the shares are summed on the device in call order and Adam is applied once.

losses=[(term, weight), ...] replaces the hard-wired MSE by the reference's loss list (train.py:65, 100-102): "mse", "chamfer"
and "hausdorff" (or torch.nn.MSELoss, ChamferLoss, HausdorffLoss instances; set_losses.py), up to four terms, run by
ag_train_step_losses inside the same device-resident step.  Chamfer is a batch mean like MSE and splits into parts the same way;
Hausdorff is a batch max and is refused with accumulate, step_parts or a group.  An EarthMoverLoss() instance (set_losses.py) adds
the Earth-mover term: its assignment is solved on the device inside the step, and being a mean it splits into parts as well.
"""
from __future__ import annotations

import ctypes as C

import torch

from .context import Engine, ptr, current_stream, _require_gpu, _vp_array
from .set_losses import LossSpec

_ADAM_FIXED = {"amsgrad": False, "maximize": False}


def adam_state_to_torch(step, exp_avg, exp_avg_sq, hyper, order):
    """torch.optim.Adam(model.parameters()).state_dict() from TrainStep's state.  Pure host function.
    step: applied steps; exp_avg / exp_avg_sq: 22 tensors in ag_ctx_load_weights order; hyper: lr, betas, eps, weight_decay;
    order[i] = position in ag_ctx_load_weights order of the optimiser's parameter i (model.parameters() order)."""
    dummies = [torch.zeros(1, requires_grad=True) for _ in order]
    group = torch.optim.Adam(dummies, lr=hyper["lr"], betas=tuple(hyper["betas"]), eps=hyper["eps"],
                             weight_decay=hyper["weight_decay"]).state_dict()["param_groups"][0]   # the installed torch's keys
    group["params"] = list(range(len(order)))
    state = {}
    if step > 0:
        for i, k in enumerate(order):
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": exp_avg[k].detach().clone(),
                        "exp_avg_sq": exp_avg_sq[k].detach().clone()}
    return {"state": state, "param_groups": [group]}


def adam_state_from_torch(sd, order):
    """Inverse of adam_state_to_torch: (step, exp_avg[22] or None, exp_avg_sq[22] or None, hyper).  Pure host function."""
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(order):
        raise ValueError("TrainStep: expected one param group over the model's 22 parameters")
    g = groups[0]
    for k, v in _ADAM_FIXED.items():
        if g.get(k, v) != v:
            raise NotImplementedError(f"TrainStep: Adam with {k}={g[k]} is not implemented")
    hyper = dict(lr=float(g["lr"]), betas=(float(g["betas"][0]), float(g["betas"][1])), eps=float(g["eps"]),
                 weight_decay=float(g["weight_decay"]))
    state = sd["state"]
    if not state:
        return 0, None, None, hyper
    if sorted(state.keys()) != list(range(len(order))):
        raise ValueError("TrainStep: optimizer state does not cover the 22 parameters")
    steps = {int(float(state[i]["step"])) for i in range(len(order))}
    if len(steps) != 1:
        raise ValueError(f"TrainStep: parameters at different steps {sorted(steps)}")
    m, v = [None] * len(order), [None] * len(order)
    for i, k in enumerate(order):
        m[k], v[k] = state[i]["exp_avg"], state[i]["exp_avg_sq"]
    return steps.pop(), m, v, hyper


class StepParts:
    """Host bookkeeping of one optimiser step built from parts: which total the parts were promised, how many rows came.  Pure
    host object (no device, no library): every argument error of accumulate / apply / step is raised here, before anything is
    enqueued.  spans_ranks: the parts of this rank are only a share of `total` (the other ranks hold the rest; nobody exchanges
    counts, which would be a host wait), so the rows of this rank may stay below it."""

    def __init__(self, spans_ranks=False):
        self.spans_ranks = bool(spans_ranks)
        self.total, self.rows, self.parts = None, 0, 0

    @property
    def open(self):
        return self.parts > 0

    def add(self, rows, total=None):
        """Admit a part of `rows` graphs.  Returns (total, accumulate): accumulate is False for the first part of a step (it
        overwrites), True after it."""
        rows = int(rows)
        if rows < 1:
            raise ValueError(f"TrainStep.accumulate: a part of {rows} rows")
        if not self.open:
            total = rows if total is None else int(total)
        else:
            if total is None:
                raise ValueError("TrainStep.accumulate: total is required from the second part of a step on")
            if int(total) != self.total:
                raise ValueError(f"TrainStep.accumulate: total {int(total)} differs from the {self.total} of this step's earlier parts")
            total = self.total
        if self.rows + rows > total:
            raise ValueError(f"TrainStep.accumulate: {self.rows + rows} rows given, the step's total is {total}")
        self.total, self.rows, self.parts = total, self.rows + rows, self.parts + 1
        return total, self.parts > 1

    def close(self):
        """apply(): the rows must add up to the total (on one rank; at most the total when the step spans ranks)."""
        if not self.open:
            raise ValueError("TrainStep.apply: no part was accumulated")
        if self.rows != self.total and not (self.spans_ranks and self.rows < self.total):
            raise ValueError(f"TrainStep.apply: the parts hold {self.rows} rows, the step's total is {self.total}")
        self.total, self.rows, self.parts = None, 0, 0

    def forbid_open(self, what):
        if self.open:
            raise RuntimeError(f"TrainStep.{what} inside an open step: {self.parts} part(s) accumulated, apply() not called")


class TrainStep:
    """ts = TrainStep(model, lr=1e-3, n_future=3); loss = ts.step(data, max_edges=k); ...; ts.check(); ts.sync_to_module().

    group: a torch.distributed process group (True = the default group) makes the object data-parallel.  Every rank constructs it
    from the same weights and feeds its own shard; `total` of accumulate() is then the GLOBAL row count of the step (global_rows
    is its default, and what step() / step_parts() use).  apply() sums the gradients and the loss vector over the ranks
    (all_reduce SUM) and takes the MAX of the overflow word, so a graph that overflowed on one rank skips the step on every rank:
    weights, m and v stay identical everywhere, and check() raises on every rank.  No count is exchanged behind the caller's
    back.  With the nccl (RCCL) backend the three collectives are enqueued on the current stream and apply() still does not wait
    for the GPU; with gloo torch stages the tensors through the host, so apply() waits (a rehearsal backend).

    losses: None (MSE x 1, the step as it always was, through ag_train_step / ag_train_step_part) or the reference's loss list
    [(term, weight), ...] of up to four terms, a term being "mse", "chamfer", "hausdorff" or an instance of torch.nn.MSELoss,
    ChamferLoss, HausdorffLoss, EarthMoverLoss (LossSpec checks it on the host).  step, evaluate, accumulate, apply and step_parts then run
    ag_train_step_losses; .last_loss_terms holds every step's terms before weighting, (n_future, n_terms) on the device.  A
    Hausdorff term is a max over the whole batch: accumulate, step_parts and group= raise ValueError with one.
    real_rows=True: every set term of the list runs over each graph's real rows - its live prefix, the first i with
    attrs[b, i, 0] <= 0 - on the prediction and the label alike (set_losses.py, REAL ROWS); the batches DeviceDynDataset builds
    are padded, and the set losses must not see the padding.  An MSE term keeps running over all rows, as in train.py."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, n_future=3, store_rest_state=False,
                 group=None, global_rows=None, losses=None, real_rows=False):
        self.losses = LossSpec(losses, real_rows=real_rows)   # host checks first: nothing below runs for a bad list
        if group is not None:
            self.losses.forbid_parts("__init__(group=...)")
        params = model.ordered_parameters()
        dev = _require_gpu(params[0].device)                     # no CPU fallback, as every other op
        self.model, self.device = model, dev
        self.hyper = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay))
        self.n_future, self.store_rest_state = int(n_future), bool(store_rest_state)
        assert self.n_future >= 1
        ids = {id(p): k for k, p in enumerate(params)}
        self._order = [ids[id(p)] for p in model.parameters()]  # optimiser index -> ag_ctx_load_weights position
        # an engine of its own: model.engine() keeps serving every other caller from the nn.Parameters
        self.engine = Engine(dev, pstep=model.model_config["pstep"], n_his=model.n_his, rel_dim=model.rel_input_dim,
                             motion_clamp=float(model.motion_clamp))
        if model._precision is not None:
            self.engine.set_precision(model._precision)
        self.w = [p.detach().to(dev, torch.float32).clone().contiguous() for p in params]
        self.exp_avg = [torch.zeros_like(w) for w in self.w]
        self.exp_avg_sq = [torch.zeros_like(w) for w in self.w]
        # the 22 gradients are views into ONE buffer (a data-parallel step moves it in one collective); every view starts on a
        # 512-byte boundary, as a tensor of its own would
        offs, n = [], 0
        for w in self.w:
            offs.append(n)
            n += (w.numel() + 127) // 128 * 128
        self._grad_flat = torch.zeros(n, device=dev)
        self.grad = [self._grad_flat[o:o + w.numel()].view_as(w) for o, w in zip(offs, self.w)]
        self._status = torch.zeros(4, dtype=torch.int32, device=dev)   # [0] overflow flag, [1] applied steps
        # second buffer of a data-parallel step: the loss vector, then the copy of _status[0] that travels
        self._small = torch.zeros(self.n_future + 2, dtype=torch.int32, device=dev)
        self._loss = self._small[:self.n_future + 1].view(torch.float32)
        self._flag = self._small[self.n_future + 1:]
        # every step's terms before weighting, (n_future, n_terms); None on the default path, which never forms them
        self.last_loss_terms = None if self.losses.default else torch.zeros(self.n_future, self.losses.n_terms, device=dev)
        self._spec = None if self.losses.default else self.losses.c_struct()
        self._step = 0                                                  # host counter of enqueued optimiser steps
        self.last_pred = None
        self.group = group
        self.global_rows = None if global_rows is None else int(global_rows)
        self._parts = StepParts(spans_ranks=group is not None)
        self._w_arr, self._g_arr = _vp_array(self.w), _vp_array(self.grad)
        self._m_arr, self._v_arr = _vp_array(self.exp_avg), _vp_array(self.exp_avg_sq)
        self._upload()

    def _upload(self):
        eng = self.engine
        eng.check(eng.lib.ag_ctx_load_weights_device(eng.ctx, current_stream(self.device), self._w_arr))

    def _run(self, data, max_edges, want_grad, total=None, accumulate=False):
        """total None: ag_train_step on the batch; else ag_train_step_part with B_total = total.  With a loss list both are
        ag_train_step_losses (B_total = B, accumulate = 0 for the whole batch)."""
        model, dev, eng = self.model, self.device, self.engine
        kw = {k: v for k, v in data.items() if k.endswith("_physics_param")}
        with torch.no_grad():
            inp = model._inputs(dev, data["state"], data["attrs"], data.get("Rr"), data.get("Rs"), data["p_instance"], data["action"],
                                data.get("edges"), kw)
            B, N, n_p, edges = inp.B, inp.N, inp.n_p, inp.edges
            nf = self.n_future
            fut = data["state_future"].to(device=dev, dtype=torch.float32)[:, :nf].contiguous()
            assert fut.shape == (B, nf, n_p, 3), tuple(fut.shape)
            eef = act_f = None
            if nf > 1:
                eef = data["eef_future"].to(device=dev, dtype=torch.float32)[:, :nf - 1].contiguous()
                act_f = data["action_future"].to(device=dev, dtype=torch.float32)[:, :nf - 1].contiguous()
                assert eef.shape == (B, nf - 1, N, 3) and act_f.shape == (B, nf - 1, N, 3)
            if max_edges is None:
                max_edges = int(edges.n_edges.max().item())                 # the one wait of the call
            pred = torch.empty((nf, B, n_p, 3), device=dev, dtype=torch.float32)
        args = (eng.ctx, current_stream(dev), *inp.c_args(), self._w_arr, nf, ptr(fut), ptr(eef), ptr(act_f),
                int(self.store_rest_state), max(1, int(max_edges)), int(want_grad), self._g_arr, ptr(self._loss), ptr(pred),
                ptr(self._status))
        spec = () if self._spec is None else (C.byref(self._spec), ptr(self.last_loss_terms))
        if total is None:
            eng.check(eng.lib.ag_train_step_losses(*args, B, 0, *spec) if spec else eng.lib.ag_train_step(*args))
            self.last_pred = pred
            return self._loss[nf].clone()
        before = self._loss[:nf].clone() if accumulate else None
        part = eng.lib.ag_train_step_losses if spec else eng.lib.ag_train_step_part
        eng.check(part(*args, int(total), int(accumulate), *spec))
        self.last_pred = self.last_pred + [pred] if accumulate else [pred]
        if not accumulate:
            return self._loss[nf].clone()
        return (self._loss[:nf].double() - before.double()).sum().float()      # what this part added to the running loss vector

    def _adam(self):
        self._step += 1
        h, eng = self.hyper, self.engine
        eng.check(eng.lib.ag_adam_step(eng.ctx, current_stream(self.device), self._w_arr, self._g_arr, self._m_arr, self._v_arr,
                                       self._step, h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"],
                                       ptr(self._status)))

    def accumulate(self, data, max_edges=None, total=None):
        """Enqueue one PART of an optimiser step: `data` as for step(), `total` the row count of the whole step (over every part,
        and over every rank when the object has a group).  The first part of a step overwrites the gradients and the loss vector,
        later parts add to them.  `total` may be left out on the first part only (it is then this part's rows, or global_rows) and
        must be the same on every part; a ValueError is raised before anything is enqueued.  max_edges bounds THIS part's graphs.
        Returns this part's share of loss_sum as a 0-d device tensor (for a later part: what it added to the running fp32 loss
        vector); .last_pred is a list with one (n_future, B_part, n_p, 3) tensor per part."""
        self.losses.forbid_parts("accumulate")
        if total is None and not self._parts.open:
            total = self.global_rows
        total, acc = self._parts.add(data["state"].shape[0], total)
        return self._run(data, max_edges, True, total=total, accumulate=acc)

    def _all_reduce(self):
        import torch.distributed as dist
        g = None if self.group is True else self.group
        dist.all_reduce(self._grad_flat, op=dist.ReduceOp.SUM, group=g)
        dist.all_reduce(self._loss, op=dist.ReduceOp.SUM, group=g)
        if self.last_loss_terms is not None:
            dist.all_reduce(self.last_loss_terms, op=dist.ReduceOp.SUM, group=g)
        self._flag.copy_(self._status[:1])
        dist.all_reduce(self._flag, op=dist.ReduceOp.MAX, group=g)
        self._status[:1].copy_(self._flag)

    def apply(self):
        """Close the step that accumulate() opened: the rows given must add up to `total` (a host comparison; with a group, at
        most `total`), then the all-reduce over the group if there is one, ag_adam_step and the step counter, as in step().
        Returns the full loss_sum as a 0-d device tensor."""
        self._parts.close()
        if self.group is not None:
            self._all_reduce()
        self._adam()
        return self._loss[self.n_future].clone()

    def step_parts(self, parts, max_edges=None):
        """One optimiser step over the dicts in `parts`: accumulate() each with total = the sum of their rows (global_rows with a
        group), then apply().  max_edges: one bound for all, or a list with one bound per part.  That is the way to train on a
        batch of mixed graph sizes without padding every graph to the largest: sort the graphs by edge count, split them into a
        few buckets, and pass each bucket's own bound - the edge-side GEMMs of a bucket then run over its bound, not the batch's.
        Returns loss_sum (0-d device tensor)."""
        self.losses.forbid_parts("step_parts")
        parts = list(parts)
        bounds = list(max_edges) if isinstance(max_edges, (list, tuple)) else [max_edges] * len(parts)
        if len(bounds) != len(parts) or not parts:
            raise ValueError(f"TrainStep.step_parts: {len(parts)} parts, {len(bounds)} max_edges bounds")
        self._parts.forbid_open("step_parts")
        total = self.global_rows if self.group is not None else sum(int(d["state"].shape[0]) for d in parts)
        if total is None:
            raise ValueError("TrainStep.step_parts: a data-parallel object needs global_rows")
        for d, k in zip(parts, bounds):
            self.accumulate(d, max_edges=k, total=total)
        return self.apply()

    def step(self, data, max_edges=None):
        """One training iteration on `data` (the dict train.py passes to model(**data): state, attrs, p_instance, action,
        <material>_physics_param, state_future, eef_future, action_future and either edges (an EdgeList) or dense Rr / Rs).
        Returns loss_sum as a 0-d DEVICE tensor.  max_edges: the caller's bound on the largest edge count of the batch (a data
        loader knows it: it built the edges); with it the call only enqueues.  None reads edges.n_edges.max() back once, which is
        then the step's only wait.  A batch with a graph beyond max_edges (or the EdgeList's capacity) is skipped on the device -
        weights, m and v stay as they were - and check() reports it.  Raises inside a step that accumulate() opened.  With a
        group: this rank's shard of a step of global_rows rows (= step_parts([data]))."""
        self._parts.forbid_open("step")
        if self.group is not None:
            return self.step_parts([data], max_edges=max_edges)
        loss = self._run(data, max_edges, True)
        self._adam()
        return loss

    def evaluate(self, data, max_edges=None):
        """The valid phase: forwards and loss only, no backward, no update.  Returns loss_sum (0-d device tensor); the n_future
        predictions are in .last_pred (n_future, B, n_p, 3).  A batch with a graph beyond max_edges raises the same sticky flag as in
        step(): its loss is then that of the guarded (empty) graph, and every following step() is skipped until check() has
        reported it."""
        self._parts.forbid_open("evaluate")        # it would overwrite the running loss vector
        return self._run(data, max_edges, False)

    def check(self):
        """One 16-byte read-back (waits for the enqueued steps).  Raises Exception("Exceeds max dims"), as the reference's
        pad_torch does, when a step since the last check was skipped; the step counter is then back at the number of applied
        steps and the flag is cleared, so the object is exactly where it was before the first skipped step."""
        st = self._status.cpu()
        if int(st[0]) != 0:
            self._step = int(st[1])
            self._status[0] = 0
            raise Exception("Exceeds max dims")                  # src/dynamics/utils.py:63-65 raises a bare Exception

    def sync_to_module(self):
        """Device master weights -> the model's nn.Parameters (state_dict / torch.save as before).  Bumps the parameters'
        versions, so a later plain model(...) re-uploads them.  A skipped step never touches the weights, so this needs no check()."""
        with torch.no_grad():
            for p, w in zip(self.model.ordered_parameters(), self.w):
                p.copy_(w)

    def optimizer_state_dict(self):
        """torch.optim.Adam's state_dict layout (the reference's latest_optim.pth), loadable into torch.optim.Adam(model.parameters()).
        Calls check() first (one read-back; raises for a skipped step): the `step` it reports is then the number of applied steps."""
        self.check()
        return adam_state_to_torch(self._step, self.exp_avg, self.exp_avg_sq, self.hyper, self._order)

    def load_optimizer_state_dict(self, sd):
        step, m, v, hyper = adam_state_from_torch(sd, self._order)
        with torch.no_grad():
            for k in range(len(self.w)):
                if m is None:
                    self.exp_avg[k].zero_()
                    self.exp_avg_sq[k].zero_()
                else:
                    self.exp_avg[k].copy_(m[k])
                    self.exp_avg_sq[k].copy_(v[k])
            self._status[1] = step
        self.hyper, self._step = hyper, step
