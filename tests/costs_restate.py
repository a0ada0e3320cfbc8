"""Torch restatement of the planner's cost functions and MPPI update (reference src/planning/losses.py:4-92, running_cost of
src/planning/plan.py:27-59, src/planning/plan_utils.py:31-39 and :42-101), written from the formulas, in any dtype on the CPU.

tests/test_costs_restate.py pins the float64 run to the reference's recorded outputs (tests/golden/costs.npz, mppi.npz) at the
tolerance the fp32 oracle meets there; tests/test_gpu_costs_edges.py then uses float64 as the yardstick for the HIP kernels and
the fp32 run as the measure of what fp32 arithmetic costs on the same inputs.  torch.min / max / maximum / clamp propagate NaN:
so does everything here, which is what makes the fp32 run the expectation for non-finite inputs too.

Every function takes fp32 (or any) tensors / arrays and computes in `dtype`.
"""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64


def T(a, dtype=F64):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).detach().to("cpu", dtype)


def _dist(p, q):
    """p (P,D), q (Q,D) -> (Q,P) Euclidean distances."""
    return torch.linalg.vector_norm(p[None, :, :] - q[:, None, :], dim=-1)


def chamfer_row(x, y, chunk=512):
    """x (N,3), y (M,3) -> scalar: mean over y of the distance to the nearest x + mean over x of the distance to the nearest y."""
    near_x, near_y = [], None                       # per y point its nearest x; per x point its nearest y
    for j0 in range(0, y.shape[0], chunk):
        d = _dist(x, y[j0:j0 + chunk])              # (m, N)
        near_x.append(d.min(1).values)
        m = d.min(0).values
        near_y = m if near_y is None else torch.minimum(near_y, m)
    return torch.cat(near_x).mean() + near_y.mean()


def chamfer(x, y, x_mask=None, y_mask=None, dtype=F64):
    """x (R,N,3), y (1|R,M,3) -> (R,).  Masks (R,N) / (1|R,M) select points by indexing, row by row (mean_chamfer)."""
    x = x.to(dtype) if isinstance(x, torch.Tensor) and x.requires_grad else T(x, dtype)
    y = T(y, dtype)
    R, N, M = x.shape[0], x.shape[1], y.shape[1]
    if x_mask is None and y_mask is None and N * M <= (1 << 21):          # rows in batches: the same formula, fewer Python steps
        out, step = [], max(1, (1 << 22) // (N * M))
        for r0 in range(0, R, step):
            d = torch.linalg.vector_norm(x[r0:r0 + step, None, :, :] - (y if y.shape[0] == 1 else y[r0:r0 + step])[:, :, None, :], dim=-1)
            out.append(d.min(2).values.mean(1) + d.min(1).values.mean(1))
        return torch.cat(out)
    out = []
    for r in range(R):
        ry = 0 if y.shape[0] == 1 else r
        xr = x[r] if x_mask is None else x[r][torch.as_tensor(np.asarray(x_mask[r]), dtype=torch.bool)]
        yr = y[ry] if y_mask is None else y[ry][torch.as_tensor(np.asarray(y_mask[ry]), dtype=torch.bool)]
        out.append(chamfer_row(xr, yr))
    return torch.stack(out)


def box_loss(state, target, dtype=F64):
    """state (R,N,3), target (2,2) [[xmin,xmax],[zmin,zmax]] -> (R,): mean distance of the particles to the box in the x-z plane."""
    s, t = T(state, dtype), T(target, dtype)
    x, z = s[:, :, 0], s[:, :, 2]
    zero = torch.zeros_like(x)
    xd = torch.maximum(t[0, 0] - x, zero) + torch.maximum(x - t[0, 1], zero)
    zd = torch.maximum(t[1, 0] - z, zero) + torch.maximum(z - t[1, 1], zero)
    return (xd ** 2 + zd ** 2).sqrt().mean(1)


def bounds(state, dtype=F64):
    """state (R,N,3) -> (R,4) [xmin, xmax, zmin, zmax]."""
    s = T(state, dtype)
    x, z = s[:, :, 0], s[:, :, 2]
    return torch.stack([x.min(1).values, x.max(1).values, z.min(1).values, z.max(1).values], 1)


def _clouds_2d(state_pred, state_init):
    """Look-ahead step h is judged against the cloud before it: the initial one, then the prediction of step h-1.  (B,H,N,2)"""
    B = state_pred.shape[0]
    init = state_init[:, [0, 2]][None, None].expand(B, 1, -1, -1)
    return torch.cat([init, state_pred[:, :-1][..., [0, 2]]], 1)


def _collision(d, size):
    return torch.exp(-torch.maximum(d - size, torch.zeros_like(d)) * 100.0)


def rope_penalty(state_pred, action, state_init, sim_real_ratio=10.0, dtype=F64):
    sp, a, si = T(state_pred, dtype), T(action, dtype), T(state_init, dtype)
    d = torch.linalg.vector_norm(a[:, :, None, :2] - _clouds_2d(sp, si), dim=-1).min(-1).values
    return _collision(d, 0.02 * sim_real_ratio)


def cloth_terms(state_pred, action, state_init, sim_real_ratio=10.0, dtype=F64):
    """(B,H,2): [exp(-100 max(dmin - size, 0)), min(dmax, 0.4 ratio)] against the INITIAL cloud - the two terms before the
    batch-global maximum."""
    a, si = T(action, dtype), T(state_init, dtype)
    d = torch.linalg.vector_norm(a[:, :, None, :2] - si[None, None][..., [0, 2]], dim=-1)
    far = d.max(-1).values
    return torch.stack([_collision(d.min(-1).values, 0.005 * sim_real_ratio),
                        torch.minimum(far, torch.ones_like(far) * 0.4 * sim_real_ratio)], -1)


def cloth_combine(terms):
    far = terms[..., 1]
    return 1.0 - terms[..., 0] - far / far.max().item() * 0.2


def cloth_penalty(state_pred, action, state_init, sim_real_ratio=10.0, dtype=F64):
    return cloth_combine(cloth_terms(state_pred, action, state_init, sim_real_ratio, dtype))


def granular_penalty(state_pred, action, state_init, sim_real_ratio=10.0, dtype=F64):
    """Nine points along the pusher blade: start point + c * radius * (sin theta, -cos theta), c = -1, -0.75 .. 1."""
    sp, a, si = T(state_pred, dtype), T(action, dtype), T(state_init, dtype)
    x, z, th = a[:, :, 0], a[:, :, 1], a[:, :, 2]
    rad = 0.05 * sim_real_ratio
    dx, dz = rad * torch.sin(th), -rad * torch.cos(th)
    pts = []
    for c in (1.0, 0.75, 0.5, 0.25):
        pts.append(torch.stack([x - c * dx, z - c * dz], -1))
    pts.append(torch.stack([x, z], -1))
    for c in (0.25, 0.5, 0.75, 1.0):
        pts.append(torch.stack([x + c * dx, z + c * dz], -1))
    pts = torch.stack(pts, 2)                                                         # (B,H,9,2)
    d = torch.linalg.vector_norm(pts[:, :, :, None] - _clouds_2d(sp, si)[:, :, None], dim=-1)
    return _collision(d.min(-1).values.min(-1).values, 0.02 * sim_real_ratio)


PENALTY = {"rope": rope_penalty, "cloth": cloth_penalty, "granular": granular_penalty}


def running_cost(state, action, state_cur, error_func, penalty_func, bbox, dtype=F64):
    """state (B,H,N,3) -> reward (B,).  error_func((B*H,N,3)) -> (B*H,), penalty_func(state, action, state_cur) -> (B,H): restatements
    run in the same dtype.  error_weight is a Python float, as in the reference (so formed in double precision in every dtype)."""
    s = T(state, dtype)
    B, H = s.shape[:2]
    error = error_func(s.reshape(B * H, s.shape[2], 3)).reshape(B, H)
    error_weight = 2.0 / (error.max().item() + 1e-6)
    pen = penalty_func(s, action, state_cur)
    bd = bounds(s.reshape(B * H, s.shape[2], 3), dtype).reshape(B, H, 4)
    bb = np.asarray(bbox, np.float64)
    zero = torch.zeros_like(bd[..., 0])
    viol = torch.stack([torch.maximum(bd[..., 0] - float(bb[0, 0]), zero), torch.maximum(float(bb[0, 1]) - bd[..., 1], zero),
                        torch.maximum(bd[..., 2] - float(bb[1, 0]), zero), torch.maximum(float(bb[1, 1]) - bd[..., 3], zero)], -1)
    box = torch.exp(-viol * 100.0).max(-1).values
    return -error_weight * error[:, -1] - 5.0 * pen.mean(1) - 5.0 * box.mean(1)


# ---- MPPI (plan_utils.py:31-39, 42-101)
def angle_normalize(x):
    return ((x + math.pi) % (2 * math.pi)) - math.pi


def clip_actions(action, lo, hi, dtype=F64):
    """theta wrapped into [-pi, pi) (torch.remainder: the result takes the divisor's sign), every component clamped."""
    a = T(action, dtype).clone()
    a[..., 2] = angle_normalize(a[..., 2])
    return torch.clamp(a, T(lo, dtype), T(hi, dtype))


def _encode(xs, ys, xe, ye, push_length):
    theta = torch.atan2(ys - ye, xs - xe)
    length = torch.linalg.vector_norm(torch.stack([xe - xs, ye - ys], -1), dim=-1) / push_length
    return torch.stack([xs, ys, theta, length], -1)


def _end_points(a, push_length):
    return a[..., 0] - a[..., 3] * push_length * torch.cos(a[..., 2]), a[..., 1] - a[..., 3] * push_length * torch.sin(a[..., 2])


def mppi_update(act_seqs, rewards, reward_weight, lo, hi, push_length=0.1, dtype=F64):
    """act_seqs (B,H,4), rewards (B,) -> (H,4): softmax(reward * weight)-weighted means of the pushes' start and end points,
    re-encoded as (x, z, theta, length) and limited."""
    a = T(act_seqs, dtype)
    # The logits are an fp32 tensor in the reference and on the device: at reward_weight = 500 and |reward| = 5 the rounding of
    # that one product (half an ulp of 2500: 1.2e-4 in the exponent) outweighs everything after it by two orders of magnitude, and
    # both sides commit it identically.  Formed in fp32 in every dtype, so that float64 measures the arithmetic that can differ.
    logits = (T(rewards, torch.float32) * reward_weight).to(dtype)
    w = torch.softmax(logits, 0)[:, None]
    xe, ye = _end_points(a, push_length)
    enc = _encode((w * a[..., 0]).sum(0), (w * a[..., 1]).sum(0), (w * xe).sum(0), (w * ye).sum(0), push_length)
    return clip_actions(enc, lo, hi, dtype)


def mppi_perturb(act_seq, noise, lo, hi, push_length=0.1, dtype=F64):
    """act_seq (H,4), noise (H,S,4) -> (S,H,4): start and end point of look-ahead step i moved by 0.1 * 10^i * noise[i], re-encoded
    and limited; sample 0 keeps the nominal action."""
    a, n = T(act_seq, dtype), T(noise, dtype)
    H, S = n.shape[:2]
    xe, ye = _end_points(a, push_length)
    out = a[None].repeat(S, 1, 1)
    for i in range(H):
        res = T(torch.tensor(0.1 * (10 ** i), dtype=torch.float32), dtype) * n[i]     # the scale is an fp32 constant on the device
        enc = _encode(a[i, 0] + res[:, 0], a[i, 1] + res[:, 1], xe[i] + res[:, 2], ye[i] + res[:, 3], push_length)
        out[1:, i] = clip_actions(enc, lo, hi, dtype)[1:]
    return out


def circular_diff(a, b):
    """|a - b| modulo 2 pi, in [0, pi]."""
    d = (a - b).abs() % (2 * math.pi)
    return torch.minimum(d, 2 * math.pi - d)


def nn_margin(x, y, x_mask=None, y_mask=None):
    """Smallest gap, in float64, between the nearest and the second-nearest neighbour distance over every valid point of either
    cloud (inf where the other cloud has a single valid point): the arg-min of the chamfer gradient is unambiguous iff this is
    clearly above fp32 resolution.  x (R,N,3), y (1|R,M,3)."""
    x, y = T(x), T(y)
    worst = math.inf
    for r in range(x.shape[0]):
        ry = 0 if y.shape[0] == 1 else r
        xr = x[r] if x_mask is None else x[r][torch.as_tensor(np.asarray(x_mask[r]), dtype=torch.bool)]
        yr = y[ry] if y_mask is None else y[ry][torch.as_tensor(np.asarray(y_mask[ry]), dtype=torch.bool)]
        d = _dist(xr, yr)
        for dim in (0, 1):
            if d.shape[dim] >= 2:
                two = torch.topk(d, 2, dim=dim, largest=False).values
                gap = (two.select(dim, 1) - two.select(dim, 0)).min().item()
                worst = min(worst, gap)
    return worst


# ---- seeded inputs of tests/test_gpu_costs_edges.py; tests/test_costs_restate.py checks their preconditions on the CPU ----------
F32 = np.float32
CHAMFER_SHAPES = [(1, 1), (1, 7), (2, 3), (3, 2), (4, 5), (5, 4), (255, 257), (256, 256), (1023, 1025), (1024, 1024), (1025, 1)]
CHAMFER_GRAD_SHAPES = [(1, 1), (1, 7), (5, 4), (257, 255), (1025, 3)]
CHAMFER_MAX_POINTS = (160 * 1024 - 2048) // 12 - 2          # both clouds in LDS, each padded to even length (ag_cost.hip)
MASK_KINDS = ("none", "random", "one")
TIE_MARGIN = 1e-4


def _mask(rng, rows, n, kind):
    if kind == "none":
        return None
    m = rng.uniform(size=(rows, n)) < 0.5 if kind == "random" else np.zeros((rows, n), bool)
    m[np.arange(rows), rng.integers(0, n, rows)] = True      # never an empty cloud (the reference raises there)
    return m


def chamfer_case(N, M, By, mask_kind, R=3, seed=0):
    """-> x (R,N,3), y (By,M,3) fp32 N(0,1) / N(0.2,1) coordinates, x_mask, y_mask (None or bool)."""
    rng = np.random.default_rng([11, N, M, By, MASK_KINDS.index(mask_kind), seed])
    x = rng.normal(0.0, 1.0, (R, N, 3)).astype(F32)
    y = rng.normal(0.2, 1.0, (By, M, 3)).astype(F32)
    return x, y, _mask(rng, R, N, mask_kind), _mask(rng, By, M, mask_kind)


def chamfer_grad_case(N, M, By, masked, R=3):
    """chamfer_case whose nearest and second-nearest neighbours differ by more than TIE_MARGIN everywhere (float64): the first of
    the seeds 0, 1, 2 .. that has the property with a factor two to spare."""
    for seed in range(200):
        x, y, xm, ym = chamfer_case(N, M, By, "random" if masked else "none", R, seed)
        if nn_margin(x, y, xm, ym) > 2 * TIE_MARGIN:
            return x, y, xm, ym
    raise AssertionError("no seed separates the neighbours")


def with_garbage(a, mask):
    """Masked-out points overwritten with 1e30 and NaN in turn."""
    a = a.copy()
    idx = np.argwhere(~mask)
    for k, (r, i) in enumerate(idx):
        a[r, i] = (1e30, np.nan, -1e30)[k % 3] if k % 2 == 0 else np.nan
    return a


BOX = np.array([[-2.6, -1.2], [0.4, 1.9]], F32)               # the target box of tests/golden/costs.npz
BBOX = np.array([[-4.5, 0.0], [-2.5, 4.5]])                  # rope.yaml's workspace, sim units


def box_case(N, R=4):
    """Points around the box: inside, outside, and - the first two of every row (N = 1: the first) - exactly on its edges and corners."""
    rng = np.random.default_rng([12, N])
    s = np.stack([rng.uniform(-4.0, 0.2, (R, N)), rng.normal(0, 1, (R, N)), rng.uniform(-1.0, 3.3, (R, N))], -1).astype(F32)
    (x0, x1), (z0, z1) = BOX
    edge = [(x0, 1.0), (x1, 1.0), (-2.0, z0), (-2.0, z1), (x0, z0), (x1, z1), (x0, 3.0), (-3.5, z1)]
    for k, (ex, ez) in enumerate(edge):
        s[k % R, (k // R) % N, [0, 2]] = (ex, ez)
    return s


def penalty_case(N, B, H, width=4):
    """state_pred (B,H,N,3) whose look-ahead steps sit 1.5 apart (the pusher sizes are 0.05 and 0.2), state_init (N,3), action
    (B,H,width) with start points near the clouds; candidate 0 / step 0 starts on a particle."""
    rng = np.random.default_rng([13, N, B, H])
    init = (rng.normal(0, 0.4, (N, 3)) + [-2.0, 0.0, 1.0]).astype(F32)
    shift = np.zeros((1, H, 1, 3)); shift[0, :, 0, 0] = 1.5 * (1 + np.arange(H)); shift[0, :, 0, 2] = -0.7 * (1 + np.arange(H))
    pred = (init[None, None] + shift + rng.normal(0, 0.05, (B, H, N, 3))).astype(F32)
    act = np.zeros((B, H, width), F32)
    before = np.concatenate([np.broadcast_to(init, (B, 1, N, 3)), pred[:, :-1]], 1)        # the cloud step h is judged against
    pick = before[np.arange(B)[:, None], np.arange(H)[None], rng.integers(0, N, (B, H))]
    act[..., 0] = pick[..., 0] + rng.uniform(-0.6, 0.6, (B, H))
    act[..., 1] = pick[..., 2] + rng.uniform(-0.6, 0.6, (B, H))
    act[0, 0, :2] = init[0, [0, 2]] + 0.01
    act[..., 2] = rng.uniform(-3.14, 3.14, (B, H))
    if width == 4:
        act[..., 3] = rng.uniform(2, 10, (B, H))
    return pred, act, init


def reward_case(B, H, N=64):
    """running_cost inputs: clouds inside rope.yaml's workspace, some poking through a side; a 33-point target."""
    rng = np.random.default_rng([14, B, H])
    init = (rng.normal(0, 0.3, (N, 3)) + [-2.2, 0.0, 1.0]).astype(F32)
    state = (init[None, None] + rng.normal(0, 0.5, (B, H, 1, 3)) + rng.normal(0, 0.05, (B, H, N, 3))).astype(F32)
    act = np.zeros((B, H, 4), F32)
    act[..., 0] = -2.2 + rng.uniform(-1.5, 1.5, (B, H))
    act[..., 1] = 1.0 + rng.uniform(-1.5, 1.5, (B, H))
    act[..., 2] = rng.uniform(-3.14, 3.14, (B, H))
    act[..., 3] = rng.uniform(2, 10, (B, H))
    target = (init[rng.integers(0, N, 33)] + F32([0.5, 0.0, 0.3]) + rng.normal(0, 0.05, (33, 3))).astype(F32)
    return state, act, init, target


MPPI_LO = np.array([-4.5, -2.5, -3.14, 2.0], F32)
MPPI_HI = np.array([0.0, 4.5, 3.14, 10.0], F32)
MPPI_REWARD_WEIGHT = 500.0
MPPI_REWARD_KINDS = ("spread", "equal", "dominant")


def mppi_case(B, H, kind):
    """Candidates scattered around one nominal push per step (step 1's nominal angle is next to pi, so candidates fall on both
    sides of the wrap), rewards with spread * reward_weight = 200 / all equal / one candidate far ahead."""
    rng = np.random.default_rng([15, B, H, MPPI_REWARD_KINDS.index(kind)])
    nominal = np.array([[-2.0, 1.0, 0.8, 6.0], [-3.0, 2.5, 3.1, 4.0], [-1.0, -1.0, -2.0, 8.0]], F32)[:H]
    a = (nominal[None] + rng.normal(0, 1, (B, H, 4)) * [0.4, 0.4, 0.3, 1.0]).astype(F32)
    a[..., 3] = np.clip(a[..., 3], 2.0, 10.0)
    if kind == "spread":
        r = -5.0 + rng.uniform(-0.4, 0.0, B)
    elif kind == "equal":
        r = np.full(B, -5.0)
    else:
        r = -5.0 + rng.uniform(-0.01, 0.0, B)
        r[B // 2] = -4.0
    return a, r.astype(F32)


def clip_case():
    """theta at -pi, pi, their fp32 neighbours, +-3 pi, +-1e4 (and a few ordinary angles); the other components in and out of range."""
    pi = F32(np.pi)
    th = np.array([-pi, pi, np.nextafter(-pi, F32(0)), np.nextafter(-pi, F32(-4)), np.nextafter(pi, F32(0)), np.nextafter(pi, F32(4)),
                   3 * pi, -3 * pi, 1e4, -1e4, 0.0, -0.0, 1.0, -2.5, 6.0, -6.0], F32)
    rng = np.random.default_rng(16)
    a = (rng.normal(0, 1, (th.size, 4)) * [4, 4, 1, 6] + [-2, 1, 0, 6]).astype(F32)
    a[:, 2] = th
    return a
