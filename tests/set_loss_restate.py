"""Restatement of the reference's training set losses (src/dynamics/gnn/loss.py: ChamferLoss :4-22, HausdorffLoss :63-82) in plain
torch, written for float64 and autograd, and of the train-loop body with a loss list (train.py:65, 100-102).  Independent of the
engine: it is the CPU yardstick of tests/test_set_losses.py and is held against the reference's own values and gradients in
tests/golden/set_losses.npz and train_losses_rope.npz.  Also the gap measures the fixtures are conditioned on."""
from __future__ import annotations

import numpy as np
import torch

import train_restate as TR

TERMS = ("mse", "chamfer", "hausdorff")


def pair_dist(x, y):
    """x (B,N,3), y (B,M,3) -> (B,N,M) Euclidean distances; zero gradient at zero distance, as torch.norm has it."""
    d = x[:, :, None, :] - y[:, None, :, :]
    return torch.linalg.vector_norm(d, dim=3)


def chamfer(x, y):
    dis = pair_dist(x, y)
    return dis.min(dim=2)[0].mean() + dis.min(dim=1)[0].mean()


def hausdorff(x, y):
    dis = pair_dist(x, y)
    return dis.min(dim=2)[0].max() + dis.min(dim=1)[0].max()


def term_value(name, pred, gt):
    if name == "mse":
        return torch.nn.functional.mse_loss(pred, gt)
    return {"chamfer": chamfer, "hausdorff": hausdorff}[name](pred, gt)


def chain_loss_terms(step, inp, n_future, losses):
    """TR.chain_loss with loss = sum(weight * term(pred, gt)) over `losses` = [(name, weight), ...] (train.py:100-102).
    Returns (loss_sum, terms (n_future, n_terms) detached, predictions per step detached)."""
    state, action = inp["state"], inp["action"]
    n_p = inp["n_p"]
    loss, table, preds = 0, [], []
    for fi in range(n_future):
        gt = inp["state_future"][:, fi]
        pred, _ = step(state, action)
        p = pred[:, :gt.shape[1], :3]
        vals = [term_value(name, p, gt) for name, _ in losses]
        loss = loss + sum(w * v for (_, w), v in zip(losses, vals))
        table.append([float(v.detach()) for v in vals])
        preds.append(p.detach())
        if fi < n_future - 1:
            nxt = inp["eef_future"][:, fi].clone().unsqueeze(1)
            nxt[:, -1, :n_p] = pred[:, :n_p]
            state = torch.cat([state[:, 1:], nxt], 1)
            action = inp["action_future"][:, fi]
    return loss, np.array(table, np.float64), preds


def winners(x, y):
    """What decides the gradient's routing: both arg-min tables and the two arg-max (flat indices), as numpy arrays."""
    dis = pair_dist(torch.as_tensor(x), torch.as_tensor(y))
    mx, ax = dis.min(dim=2)
    my, ay = dis.min(dim=1)
    return ax.numpy(), ay.numpy(), int(mx.reshape(-1).argmax()), int(my.reshape(-1).argmax())


def gaps(x, y):
    """float64 gaps of a cloud pair batch, [nn_xy, nn_yx, top_xy, top_yx]: the smallest distance between a point's nearest and
    second-nearest neighbour in each direction, and the distance between the two largest minima in each direction.  inf where
    there is no second candidate."""
    dis = pair_dist(torch.as_tensor(np.asarray(x, np.float64)), torch.as_tensor(np.asarray(y, np.float64))).numpy()
    out = []
    for axis in (2, 1):
        s = np.sort(dis, axis=axis)
        two = np.take(s, [0, 1], axis=axis) if dis.shape[axis] > 1 else None
        out.append(float(np.diff(two, axis=axis).min()) if two is not None else np.inf)
    for axis in (2, 1):
        m = np.sort(dis.min(axis=axis).reshape(-1))
        out.append(float(m[-1] - m[-2]) if m.size > 1 else np.inf)
    return np.array(out, np.float64)


def restated_chain(f, losses, dtype=torch.float64):
    """The chain of a training fixture in `dtype` with the loss list: (loss_sum, terms, predictions, 22 gradients, dstate0)."""
    inp = TR.fixture_inputs(f, dtype)
    B, N = inp["attrs"].shape[:2]
    recv, send = TR.fixture_edges(f, B, N)
    W = TR.weights(f, dtype)
    inp["state"].requires_grad_(True)
    step = lambda s, a: TR.forward(W, s, inp["attrs"], a, inp["phys"], inp["group"], recv, send, inp["n_p"],  # noqa: E731
                                   int(f["pstep"]))
    loss, terms, preds = chain_loss_terms(step, inp, int(f["n_future"]), losses)
    loss.backward()
    return loss.item(), terms, preds, {k: W[k].grad.numpy() for k in TR.KEYS}, inp["state"].grad.numpy()
