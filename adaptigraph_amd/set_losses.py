"""Set losses of the reference's training side (src/dynamics/gnn/loss.py) on the HIP engine.

    loss_funcs = [(torch.nn.MSELoss(), 1), (ChamferLoss(), 0.5), (HausdorffLoss(), 0.25)]      # train.py:65
    loss = sum(weight * func(pred, label) for func, weight in loss_funcs)                      # train.py:100-102

ChamferLoss (loss.py:4-22) and HausdorffLoss (loss.py:63-82) are torch.nn.Modules called as loss(pred, label) with pred (B,N,3)
and label (B,M,3) on the GPU; each returns a 0-d device tensor and is a torch.autograd.Function over ag_set_loss /
ag_set_loss_backward: no (B,N,M,3) tensor is ever formed.  The gradient goes toward pred only - the label is data, and a label
that requires grad raises NotImplementedError.  Called as loss(pred, label) every row counts, as in the reference's training
losses; called with counts, loss(pred, label, n_pred, n_label), each graph's real rows count (REAL ROWS below).  TrainStep takes
the same terms by name (losses=[("mse", 1), ("chamfer", 0.5)]) and runs them inside the device-resident step.
  * ties: the arg-min is the lowest index of the smallest distance and the Hausdorff winner the lowest (b, index) of the largest
    minimum, which are torch.min(dim)'s and torch.max()'s values and indices.  One gradient differs from the reference's autograd:
    torch.max() over the batch splits its gradient evenly among EQUAL maxima, HausdorffLoss gives the whole weight to the one
    winning pair per side.  Only exact ties - duplicated points - show it; the tied rows together carry the same pull.
  * non-finite input: a NaN distance wins a min and a max, so the loss is NaN (inf for an infinite coordinate), the gradient row
    of a NaN point is NaN, and the rows of graphs without a non-finite coordinate keep the bits of a clean run.

EarthMoverLoss (loss.py:25-60) is the third: the mean distance over the one-to-one matching of K = min(N, M) pairs per graph with
the smallest sum of distances.  The reference solves that assignment on the host (scipy.optimize.linear_sum_assignment per graph,
one device-to-host wait each); here it is a kernel (ag_emd.hip: shortest augmenting paths with dual variables in fp64, one
workgroup per graph), so the loss runs on the autograd path and inside TrainStep without a host wait.  earth_mover_assignment
returns the matching itself in scipy's layout.
  * cap: min(N, M) <= 512 (EMD_MAX_MATCH) and N + M within the solver's LDS tile (~4k points); beyond it NotImplementedError,
    before anything is enqueued.  The search is serial in its steps: a graph of K = 512 laid out adversarially takes 180 ms
    (profiles/r21_emd.json); a batch of 128 training-sized graphs (K = 100, random) 1.5 ms, forward and backward.
  * tie rule of the search: among equal path costs a free column wins, then the lowest column index.  The optimum of generic
    clouds is unique and does not depend on it.
  * non-finite input: a graph with a NaN or inf coordinate is not solved.  The loss is NaN, that graph's gradient rows are NaN
    and its match table is -1.  The reference's behaviour there is an accident - scipy raises, a bare except prints, and the
    previous graph's indices are used - and is not reproduced.
TrainStep takes the term as an EarthMoverLoss() instance.  The strings ("emd", ...) and foreign classes that are merely named
EarthMoverLoss keep their NotImplementedError: such a class is the reference's host solve, for which the message is true;
accepting the strings is left to a later change.

REAL ROWS (AG_LOSS_ROWS).  The loader's batches are padded: DeviceDynDataset.batch() samples each graph by radius, rows behind
n_obj[b] are zero in state_future, and the model's prediction there is not.  The plain losses would match real particles to
padding at the origin, let a padding row win the Hausdorff max and spend Earth-mover pairs on padding.  With counts
    loss(pred, label, n_pred, n_label)          n_pred, n_label: (B,) integer device tensors, None = full on that side
graph b's real rows are the prefixes pred[b, :n_pred[b]] and label[b, :n_label[b]] (the layout DeviceDynDataset and
dynamics_masked produce); prefix_counts(data["obj_mask"]) turns a loader batch's mask into counts on the device.  Counts are
clamped into [0, N] / [0, M] on the device, never read back; rows behind them are never read, so NaN or inf there changes no bit.
  * ChamferLoss    (1/B) sum_b [ mean_{i<nx_b} min_{j<ny_b} d + mean_{j<ny_b} min_{i<nx_b} d ]: the mean over graphs of each graph's
    own Chamfer distance, i.e. the planning side's mean_chamfer(...).mean() (src/planning/losses.py:12-24) - deliberately not the
    pooled mean sum / sum n_b: graphs weigh equally, and the term splits into parts and ranks through B_total with no count
    exchanged.  Full counts: the plain loss up to the last place (the division happens per graph).
  * HausdorffLoss  max over the real rows of every graph, per side; full counts give the plain loss's bits.  Still refused in parts.
  * EarthMoverLoss (1/B) sum_b (1/K_b) sum of the optimal assignment over the real rows, K_b = min(nx_b, ny_b); the smaller real
    cloud is the row side, x when the counts are equal.  The caps stay on the padded sizes.
  * a graph with an empty side (nx_b == 0 or ny_b == 0) is batch padding - a rule of this package; torch's mean over nothing is
    NaN.  It adds 0 to Chamfer and Earth-mover, has no Hausdorff candidate (all graphs empty: 0), its gradient rows are 0, and it
    still counts in B.
  * gradient: rows i >= nx_b are written as exact 0; a real row's scale is g/(B nx_b) for the x-side Chamfer sum, g/(B ny_b) for
    the y-side sum, g/(B K_b) for Earth-mover.  A non-finite coordinate in a REAL row keeps the rules above (NaN loss; an
    Earth-mover graph fails alone).
LossSpec(losses, real_rows=True) / TrainStep(..., real_rows=True) put the flag on every set term of the list; the step takes the
counts from attrs: n_b = the first i < n_p with attrs[b, i, 0] <= 0.  An MSE term still runs over all rows, as in train.py.
"""
from __future__ import annotations

import torch

from . import _lib
from .context import default_engine, ptr, current_stream, _require_gpu


class _SetLossFunction(torch.autograd.Function):
    """ag_set_loss forward, ag_set_loss_backward backward.  The forward leaves its arg-min tables (Earth-mover: its match table
    and status words) in `work`; the backward reads them instead of searching (solving) again."""

    @staticmethod
    def forward(ctx, x, y, kind, counts=None):
        dev = x.device
        eng = default_engine(dev)
        B, N, _ = x.shape
        M = y.shape[1]
        out = torch.empty((), device=dev, dtype=torch.float32)
        work = _work_buffer(B, N, M, dev, counts)
        eng.check(eng.lib.ag_set_loss(eng.ctx, current_stream(dev), ptr(x), ptr(y), B, N, M, B, kind, ptr(out), ptr(work)))
        ctx.save_for_backward(x, y, work)
        ctx.kind = kind
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, y, work = ctx.saved_tensors
        dev = x.device
        eng = default_engine(dev)
        B, N, _ = x.shape
        M = y.shape[1]
        g_out = g_out.to(torch.float32).reshape(1).contiguous()
        g_x = torch.empty_like(x)
        eng.check(eng.lib.ag_set_loss_backward(eng.ctx, current_stream(dev), ptr(x), ptr(y), B, N, M, B, ctx.kind, ptr(g_out),
                                               ptr(g_x), ptr(work)))
        return g_x, None, None, None


def _work_buffer(B, N, M, dev, counts):
    """B*(N+M) + 4 int32 of tables; with counts the 2B input words nx, ny behind them (adaptigraph_amd.h, ag_set_loss)"""
    n_tab = B * (N + M) + 4
    if counts is None:
        return torch.empty(n_tab, device=dev, dtype=torch.int32)
    work = torch.empty(n_tab + 2 * B, device=dev, dtype=torch.int32)
    work[n_tab:].view(2, B).copy_(counts)
    return work


def _counts(n_pred, n_label, B, N, M, dev, name):
    """None when both are None; else the (2, B) int32 device tensor [nx, ny], a missing side full.  Shape and dtype are checked
    on the host; the VALUES are never read back - the kernels clamp them."""
    if n_pred is None and n_label is None:
        return None
    rows = []
    for n, full, what in ((n_pred, N, "n_pred"), (n_label, M, "n_label")):
        if n is None:
            rows.append(torch.full((B,), full, device=dev, dtype=torch.int32))
            continue
        if not isinstance(n, torch.Tensor) or n.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise TypeError(f"{name}: {what} must be an integer tensor of shape ({B},), got {type(n).__name__}"
                            f"{'' if not isinstance(n, torch.Tensor) else ' of ' + str(n.dtype)}")
        if tuple(n.shape) != (B,):
            raise AssertionError(f"{name}: {what} must have shape ({B},), got {tuple(n.shape)}")
        if n.device != dev:
            raise AssertionError(f"{name}: {what} lives on {n.device}, the clouds on {dev}")
        if n.dtype == torch.int64:                               # clamp before narrowing: the kernels then clamp into [0, N]
            n = n.clamp(-1, 2 ** 31 - 1)
        rows.append(n.to(torch.int32))
    return torch.stack(rows)


def _set_loss(pred, label, kind, name, n_pred=None, n_label=None):
    dev = _require_gpu(pred.device)
    if label.requires_grad:
        raise NotImplementedError(f"{name}: the label is data; a gradient toward it is not implemented")
    if pred.dim() != 3 or label.dim() != 3 or pred.shape[2] != 3 or label.shape[2] != 3 or pred.shape[0] != label.shape[0]:
        raise AssertionError(f"{name}: pred (B,N,3) and label (B,M,3) expected, got {tuple(pred.shape)} and {tuple(label.shape)}")
    counts = _counts(n_pred, n_label, pred.shape[0], pred.shape[1], label.shape[1], dev, name)
    x = pred.to(torch.float32).contiguous()
    y = label.detach().to(device=dev, dtype=torch.float32).contiguous()
    if counts is None:
        return _SetLossFunction.apply(x, y, kind)
    return _SetLossFunction.apply(x, y, kind | _lib.AG_LOSS_ROWS, counts)


def prefix_counts(mask):
    """(B, n) bool or uint8 mask -> (B,) int32 device tensor: the index of the first false entry of every row (n if there is
    none), i.e. the length of the row's true prefix.  prefix_counts(data["obj_mask"]) feeds a loader batch to the set losses.
    Runs on the mask's device without a wait."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2 or mask.dtype not in (torch.bool, torch.uint8):
        raise AssertionError("prefix_counts: a (B, n) bool or uint8 mask expected")
    return (mask != 0).to(torch.int32).cumprod(dim=1).sum(dim=1, dtype=torch.int32)


class ChamferLoss(torch.nn.Module):
    """loss.py:4-22: mean over all B*N nearest distances pred -> label plus mean over all B*M nearest distances label -> pred.
    With n_pred / n_label: the mean over graphs of each graph's Chamfer distance over its real rows (module docstring)."""

    def forward(self, pred, label, n_pred=None, n_label=None):
        return _set_loss(pred, label, _lib.AG_LOSS_CHAMFER, "ChamferLoss", n_pred, n_label)


class HausdorffLoss(torch.nn.Module):
    """loss.py:63-82: the largest nearest distance pred -> label over the whole batch plus the largest label -> pred.  With
    n_pred / n_label: over the real rows only (module docstring)."""

    def forward(self, pred, label, n_pred=None, n_label=None):
        return _set_loss(pred, label, _lib.AG_LOSS_HAUSDORFF, "HausdorffLoss", n_pred, n_label)


class EarthMoverLoss(torch.nn.Module):
    """loss.py:25-60: mean over the B * min(N, M) distances of the per-graph optimal one-to-one matching pred <-> label.  The
    assignment is solved exactly on the device (module docstring: cap, tie rule, non-finite rule); x rows left unmatched
    (N > M) get a zero gradient.  With n_pred / n_label: the mean over graphs of each graph's mean matched distance over its
    real rows (module docstring)."""

    def forward(self, pred, label, n_pred=None, n_label=None):
        return _set_loss(pred, label, _lib.AG_LOSS_EMD, "EarthMoverLoss", n_pred, n_label)


def earth_mover_assignment(pred, label, n_pred=None, n_label=None):
    """The matching EarthMoverLoss uses, in the layout of scipy.optimize.linear_sum_assignment per graph: (ind1, ind2), int64
    device tensors of shape (B, K), K = min(N, M), ind1 ascending, pred[b, ind1[b, k]] matched to label[b, ind2[b, k]].  A failed
    graph (non-finite input) has ind1 = ind2 = -1.  With n_pred / n_label the layout is the same and graph b's entries beyond
    K_b = min(nx_b, ny_b) are -1.  Read from the `work` buffer of ag_set_loss; no host wait."""
    dev = _require_gpu(pred.device)
    if pred.dim() != 3 or label.dim() != 3 or pred.shape[2] != 3 or label.shape[2] != 3 or pred.shape[0] != label.shape[0]:
        raise AssertionError(f"earth_mover_assignment: pred (B,N,3) and label (B,M,3) expected, got {tuple(pred.shape)} and "
                             f"{tuple(label.shape)}")
    x = pred.detach().to(torch.float32).contiguous()
    y = label.detach().to(device=dev, dtype=torch.float32).contiguous()
    eng = default_engine(dev)
    B, N, _ = x.shape
    M = y.shape[1]
    K = min(N, M)
    counts = _counts(n_pred, n_label, B, N, M, dev, "earth_mover_assignment")
    kind = _lib.AG_LOSS_EMD if counts is None else _lib.AG_LOSS_EMD | _lib.AG_LOSS_ROWS
    out = torch.empty((), device=dev, dtype=torch.float32)
    work = _work_buffer(B, N, M, dev, counts)
    eng.check(eng.lib.ag_set_loss(eng.ctx, current_stream(dev), ptr(x), ptr(y), B, N, M, B, kind, ptr(out), ptr(work)))
    match = work[:B * N].view(B, N).to(torch.int64)
    failed = (work[B * N:B * N + B] != 0).view(B, 1)
    # the K matched rows in ascending order (a stable sort keeps the index order inside both groups); a failed graph has none
    ind1 = torch.sort((match < 0).to(torch.int8), dim=1, stable=True)[1][:, :K]
    ind2 = torch.gather(match, 1, ind1)
    none = failed | (ind2 < 0)                                  # a failed graph; with counts, the entries beyond K_b
    return torch.where(none, -1, ind1), torch.where(none, -1, ind2)


class LossSpec:
    """The loss list of a training step, parsed and checked on the host: [(term, weight), ...] with a term "mse", "chamfer" or
    "hausdorff", or an instance of torch.nn.MSELoss, ChamferLoss, HausdorffLoss or this package's EarthMoverLoss (name
    "earth_mover").  The Earth-mover strings and a foreign class named EarthMoverLoss - the reference's host solve - stay
    refused.  Pure host object (no device, no library), the pattern of StepParts: every argument error is raised here, before
    anything is enqueued.  None = [("mse", 1)] through the entry points TrainStep always used (.default)."""

    MAX_TERMS = 4
    KINDS = {"mse": _lib.AG_LOSS_MSE, "chamfer": _lib.AG_LOSS_CHAMFER, "hausdorff": _lib.AG_LOSS_HAUSDORFF}

    def __init__(self, losses=None, real_rows=False):
        self.default = losses is None
        self.real_rows = bool(real_rows)
        terms = [("mse", 1.0)] if losses is None else list(losses)
        if not 1 <= len(terms) <= self.MAX_TERMS:
            raise ValueError(f"TrainStep: {len(terms)} loss terms, 1 to {self.MAX_TERMS} are served")
        self.names, self.kinds, self.weights = [], [], []
        for item in terms:
            try:
                term, weight = item
            except (TypeError, ValueError):
                raise ValueError(f"TrainStep: a loss term is a (term, weight) pair, got {item!r}") from None
            name = self._name(term)
            w = float(weight)
            if w != w or w in (float("inf"), float("-inf")):
                raise ValueError(f"TrainStep: the weight of loss term {name!r} is {w}")
            self.names.append(name)
            kind = _lib.AG_LOSS_EMD if name == "earth_mover" else self.KINDS[name]
            # real_rows: every set term runs over each graph's real rows; MSE over all rows, as in train.py
            self.kinds.append(kind | _lib.AG_LOSS_ROWS if self.real_rows and kind != _lib.AG_LOSS_MSE else kind)
            self.weights.append(w)

    @classmethod
    def _name(cls, term):
        if isinstance(term, str):
            key = term.lower()
            if key in cls.KINDS:
                return key
            if key in ("emd", "earthmover", "earth_mover", "earthmoverloss"):
                cls._refuse_earth_mover()
            raise ValueError(f"TrainStep: unknown loss term {term!r} (known: {sorted(cls.KINDS)})")
        if isinstance(term, torch.nn.MSELoss):
            if term.reduction != "mean":
                raise ValueError(f"TrainStep: MSELoss(reduction={term.reduction!r}); the step computes the mean")
            return "mse"
        if isinstance(term, ChamferLoss):
            return "chamfer"
        if isinstance(term, HausdorffLoss):
            return "hausdorff"
        if isinstance(term, EarthMoverLoss):                    # this package's own; ahead of the refusal by name
            return "earth_mover"
        if type(term).__name__ == "EarthMoverLoss":
            cls._refuse_earth_mover()
        raise ValueError(f"TrainStep: unknown loss term {term!r} (known: {sorted(cls.KINDS)} or their modules)")

    @staticmethod
    def _refuse_earth_mover():
        raise NotImplementedError("TrainStep: the Earth-mover loss is not implemented: its assignment solve is a host step "
                                  "(scipy.optimize.linear_sum_assignment per graph in the reference, loss.py:42), which the "
                                  "device-resident step cannot run")

    @property
    def n_terms(self):
        return len(self.kinds)

    @property
    def has_hausdorff(self):
        return any(k & ~_lib.AG_LOSS_ROWS == _lib.AG_LOSS_HAUSDORFF for k in self.kinds)

    def forbid_parts(self, what):
        """A batch max does not split: accumulate / step_parts / a process group with a Hausdorff term.  The means (MSE, Chamfer,
        Earth-mover) split."""
        if self.has_hausdorff:
            raise ValueError(f"TrainStep.{what} with a Hausdorff term: its max runs over the whole batch and does not split into "
                             f"parts or ranks; use step() on one rank, or drop the term")

    def c_struct(self):
        s = _lib.AgLossSpec()
        s.n_terms = self.n_terms
        for k, (kind, w) in enumerate(zip(self.kinds, self.weights)):
            s.kind[k], s.weight[k] = kind, w
        return s
