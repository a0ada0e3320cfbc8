"""Restatement of the engine's CMA-ES (adaptigraph_amd/csrc/ag_cma.hip) in numpy float64: standard (mu/mu_w, lambda)-CMA-ES with
positive weights (Hansen, "The CMA Evolution Strategy: A Tutorial", 2016), the fold / wrap boundary rule, the ranking with its tie
and NaN rules, the status bits.  Independent of the engine; the CPU yardstick of tests/test_cma_restate.py and the oracle of
tests/test_gpu_cma.py.  Two switches vary what the algorithm leaves open, so that their effect on a state can be MEASURED:
  eig   'eigh' (numpy.linalg.eigh) or 'jacobi' (round-robin Jacobi rotations, written here)
  sums  'forward' or 'reverse': the direction of the sums over ranks (y_w and the rank-mu matrix)

CMA_STATE_TOL - the bound of the device-against-restatement comparison of a state field, relative to the field's largest entry:
measured (tests/test_cma_restate.py::test_tolerance_measurement) as the largest deviation between the (eigh, forward) and the
(jacobi, reverse) variant, teacher-forced - same draws, same values per generation - over all shapes of the GPU test, fields
m, sigma, C, p_sigma, p_c, A: 2.5e-14 (at n = 64, popsize = 16, 3 generations; the other shapes 0 .. 7.1e-15).  Times 100 for
the two sources the variants do not show: the device's grouped (tree-ordered) sums and its sqrt / exp / pow / division against
numpy's."""
from __future__ import annotations

import math

import numpy as np

CMA_STATE_MEASURED = 2.5e-14
CMA_STATE_TOL = 100 * CMA_STATE_MEASURED
STATE_FIELDS = ("m", "sigma", "C", "p_sigma", "p_c", "A")
# (n, popsize, generations, corner) of the teacher-forced GPU test: no rotation exists | small | odd popsize, C becomes non-trivial |
# more than one wavefront, not a multiple of 64, started at a corner of the box | the cap on n | crosses the blocks of ask and rank
GPU_CASES = ((1, 4, 4, False), (4, 8, 4, False), (12, 11, 12, False), (12, 70, 6, True), (64, 16, 3, False), (4, 2049, 3, False))


def constants(n, popsize):
    """The strategy constants of dimension n and population popsize."""
    mu = popsize // 2
    w = math.log((popsize + 1) / 2.0) - np.log(np.arange(1, mu + 1, dtype=np.float64))
    w = w / w.sum()
    mu_eff = 1.0 / float(np.sum(w * w))
    c_sigma = (mu_eff + 2.0) / (n + mu_eff + 5.0)
    c_1 = 2.0 / ((n + 1.3) ** 2 + mu_eff)
    return {"mu": mu, "weights": w, "mu_eff": mu_eff, "c_sigma": c_sigma,
            "d_sigma": 1.0 + 2.0 * max(0.0, math.sqrt((mu_eff - 1.0) / (n + 1.0)) - 1.0) + c_sigma,
            "c_c": (4.0 + mu_eff / n) / (n + 4.0 + 2.0 * mu_eff / n), "c_1": c_1,
            "c_mu": min(1.0 - c_1, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((n + 2.0) ** 2 + mu_eff)),
            "chi_n": math.sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n))}


def bound(g, lo, hi, periodic, period):
    """Genotype -> phenotype per coordinate, fp64: wrap a periodic coordinate into [-period/2, period/2), then fold a coordinate
    with finite lo < hi onto [lo, hi] (the identity inside, bit for bit); an infinite limit passes through."""
    g = np.array(g, dtype=np.float64)
    lo, hi, per = np.broadcast_to(lo, g.shape), np.broadcast_to(hi, g.shape), np.broadcast_to(periodic, g.shape).astype(bool)
    r = np.fmod(g + 0.5 * period, period)
    neg = r < 0
    r = np.where(neg, r + period, r)
    r = np.where(neg & (r >= period), 0.0, r)
    g = np.where(per, r - 0.5 * period, g)
    box = np.isfinite(lo) & np.isfinite(hi) & (lo < hi)
    w = np.where(box, hi - lo, 1.0)
    t = np.fmod(g - np.where(box, lo, 0.0), 2.0 * w)
    t = np.where(t < 0, t + 2.0 * w, t)
    with np.errstate(invalid="ignore"):
        f = np.where(box, lo, 0.0) + np.where(t <= w, t, 2.0 * w - t)
        f = np.where(np.isnan(f), f, np.minimum(np.maximum(f, lo), hi))
    inside = (g >= lo) & (g <= hi)
    return np.where(box & ~inside, f, g)


def rank_order(values, maximize):
    """order[rank] = index: (value to minimise, index) ascending, the fp32 input negated when maximising; NaN after everything, NaNs
    and equal values by index (a stable sort does all of it)."""
    v = np.asarray(values, dtype=np.float32)
    return np.argsort(-v if maximize else v, kind="stable").astype(np.int32)


def _round_robin(ne, step):
    """The pairs of step `step` of the circle method over ne (even) indices."""
    out = [(ne - 1, step)]
    for k in range(1, ne // 2):
        out.append(((step + k) % (ne - 1), (step - k + ne - 1) % (ne - 1)))
    return [(min(a, b), max(a, b)) for a, b in out]


def jacobi_eigh(C, sweeps=60):
    """Eigenvalues (unsorted) and eigenvectors (columns) of a symmetric matrix by Jacobi rotations in round-robin order: a step's
    rotations lie in disjoint planes and are applied together, D <- J^T (D J).  Sweeps end when the off-diagonal norm - summed from
    the off-diagonal entries - is at most 1e-15 of the diagonal's."""
    D = np.array(C, dtype=np.float64)
    n = D.shape[0]
    V = np.eye(n)
    ne = n + (n & 1)
    for _ in range(sweeps):
        off2 = float(sum(np.sum(np.delete(D[i], i) ** 2) for i in range(n)))
        dg2 = float(np.sum(np.diag(D) ** 2))
        if not off2 > 1e-30 * dg2:
            break
        for step in range(ne - 1):
            rot = []
            for p, q in _round_robin(ne, step):
                if q >= n or D[p, q] == 0.0:
                    continue
                theta = (D[q, q] - D[p, p]) / (2.0 * D[p, q])
                t = (-1.0 if theta < 0 else 1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                rot.append((p, q, c, t * c))
            for p, q, c, s in rot:                               # columns
                dp, dq = D[:, p].copy(), D[:, q].copy()
                D[:, p], D[:, q] = c * dp - s * dq, s * dp + c * dq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
            for p, q, c, s in rot:                               # rows
                dp, dq = D[p].copy(), D[q].copy()
                D[p], D[q] = c * dp - s * dq, s * dp + c * dq
                D[p, q] = D[q, p] = 0.0
    return np.diag(D).copy(), V


class Restate:
    """The search: same constructor defaults, ask(draws) and tell(values) as adaptigraph_amd.CmaSearch, state as attributes."""

    def __init__(self, x0, sigma0, lower, upper, popsize=None, scale=None, periodic=(), period=2.0 * math.pi, maximize=False,
                 eig="eigh", sums="forward"):
        self.m = np.array(x0, dtype=np.float64).reshape(-1)
        n = self.n = self.m.size
        self.lo, self.hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).copy() for v in (lower, upper))
        if np.any(self.lo == self.hi):
            raise ValueError("lower == upper")
        self.periodic = np.zeros(n, bool)
        self.periodic[list(periodic)] = True
        self.period = float(period)
        if scale is None:
            scale = np.where(np.isfinite(self.lo) & np.isfinite(self.hi), self.hi - self.lo, 1.0)
            scale = np.where(self.periodic, np.minimum(scale, self.period), scale)
        self.scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (n,)).copy()
        self.popsize = int(popsize) if popsize is not None else 4 + int(math.floor(3.0 * math.log(n)))
        self.k = constants(n, self.popsize)
        self.mu = self.k["mu"]
        self.sigma = float(sigma0)
        self.C, self.A, self.A_inv = np.eye(n), np.eye(n), np.eye(n)
        self.p_sigma, self.p_c = np.zeros(n), np.zeros(n)
        self.g, self.status, self.maximize = 0, 0, bool(maximize)
        self.best_value, self.best_x, self.best_generation = (-np.inf if maximize else np.inf), np.zeros(n), -1
        self.eig, self.sums = eig, sums
        self.order, self.improved = None, False
        self.y = self.x = None

    def phenotype(self, genotype):
        return bound(genotype, self.lo, self.hi, self.periodic, self.period)

    def ask(self, draws):
        z = np.asarray(draws, dtype=np.float64)
        assert z.shape == (self.popsize, self.n)
        y = np.zeros_like(z)
        for j in range(self.n):                                  # ascending j, product and sum rounded separately
            y += self.A[j][None, :] * z[:, j:j + 1]
        self.y = y
        self.x = self.phenotype(self.m[None, :] + (self.sigma * self.scale)[None, :] * y).astype(np.float32)
        return self.x

    def _rank_sum(self, terms):
        """sum over the leading (rank) axis in the configured direction, one rank at a time"""
        s = np.zeros(terms.shape[1:])
        for r in (range(terms.shape[0]) if self.sums == "forward" else range(terms.shape[0] - 1, -1, -1)):
            s = s + terms[r]
        return s

    def tell(self, values):
        v = np.asarray(values, dtype=np.float32)
        assert v.shape == (self.popsize,)
        k, n, mu = self.k, self.n, self.mu
        self.order = rank_order(v, self.maximize)
        self.improved = False
        if np.isnan(v[self.order[mu - 1]]):                      # fewer than mu values are not NaN
            self.status |= 1
            return
        w = k["weights"]
        ys = self.y[self.order[:mu]]
        y_w = self._rank_sum(w[:, None] * ys)
        m = self.m + (self.sigma * self.scale) * y_w
        t = np.zeros(n)
        for j in range(n):
            t = t + self.A_inv[:, j] * y_w[j]
        c_s, c_c, c_1, c_mu = k["c_sigma"], k["c_c"], k["c_1"], k["c_mu"]
        p_sigma = (1.0 - c_s) * self.p_sigma + math.sqrt(c_s * (2.0 - c_s) * k["mu_eff"]) * t
        ps2 = 0.0
        for i in range(n):
            ps2 += p_sigma[i] * p_sigma[i]
        psn = math.sqrt(ps2)
        h = 1.0 if psn / math.sqrt(1.0 - (1.0 - c_s) ** (2.0 * (self.g + 1.0))) < (1.4 + 2.0 / (n + 1.0)) * k["chi_n"] else 0.0
        p_c = (1.0 - c_c) * self.p_c + (h * math.sqrt(c_c * (2.0 - c_c) * k["mu_eff"])) * y_w
        S = self._rank_sum((ys[:, :, None] * ys[:, None, :]) * w[:, None, None])
        C = (1.0 - c_1 - c_mu) * self.C + c_1 * (np.outer(p_c, p_c) + ((1.0 - h) * c_c * (2.0 - c_c)) * self.C) + c_mu * S
        with np.errstate(over="ignore", invalid="ignore"):
            sigma = self.sigma * math.exp((c_s / k["d_sigma"]) * (psn / k["chi_n"] - 1.0)) if np.isfinite(psn) else np.nan
            C = 0.5 * (C + C.T)
            ok = bool(np.all(np.isfinite(C)))
            if ok:
                d, B = np.linalg.eigh(C) if self.eig == "eigh" else jacobi_eigh(C)
                ok = bool(np.all(d > 0) and np.all(np.isfinite(d)))
            if ok:
                A = np.zeros((n, n))
                A_inv = np.zeros((n, n))
                r = np.sqrt(d)
                for j in range(n):
                    vv = np.outer(B[:, j], B[:, j])
                    A = A + vv * r[j]
                    A_inv = A_inv + vv * (1.0 / r[j])
                ok = bool(np.isfinite(sigma) and sigma > 0 and all(np.all(np.isfinite(a)) for a in (m, p_sigma, p_c, A, A_inv)))
        if not ok:
            self.status |= 2
            return
        self.m, self.sigma, self.C, self.p_sigma, self.p_c, self.A, self.A_inv = m, sigma, C, p_sigma, p_c, A, A_inv
        b = int(self.order[0])
        key, best = (-float(v[b]), -self.best_value) if self.maximize else (float(v[b]), self.best_value)
        if key < best:
            self.best_value, self.best_x, self.best_generation, self.improved = float(v[b]), self.x[b].astype(np.float64), self.g, True
        self.g += 1

    def fields(self):
        return {"m": self.m, "sigma": np.array([self.sigma]), "C": self.C, "p_sigma": self.p_sigma, "p_c": self.p_c, "A": self.A,
                "A_inv": self.A_inv}


def deviation(a, b):
    """Relative max-norm deviation of two arrays: max |a - b| / max |b| (0 when both are all zero)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    top = float(np.max(np.abs(b))) if b.size else 0.0
    diff = float(np.max(np.abs(a - b))) if b.size else 0.0
    return diff / top if top > 0 else diff


def ellipsoid(n, seed=0):
    """f(x) = sum c_i (x_i - t_i)^2 with c over three decades and t inside the box [-1, 2]^n: (f, c, t, lo, hi)."""
    rng = np.random.default_rng(seed)
    c = 10.0 ** np.linspace(0.0, 3.0, n) if n > 1 else np.ones(1)
    t = rng.uniform(-0.5, 1.5, n)
    lo, hi = np.full(n, -1.0), np.full(n, 2.0)

    def f(x):
        x = np.asarray(x, dtype=np.float64)
        return np.sum(c * (x - t) ** 2, axis=-1)
    return f, c, t, lo, hi


def case(n, popsize, generations, seed=0, corner=False):
    """A seeded search on the ellipsoid -> (constructor keywords, draws (generations, popsize, n), f).  corner: the mean starts at
    the upper corner of the box with sigma0 = 1 and coordinate 2 is periodic with limits +-3.14, inside +-pi - most of the first
    population leaves the box."""
    f, _, _, lo, hi = ellipsoid(n, seed)
    rng = np.random.default_rng(100 + seed)
    x0, periodic, sigma0 = rng.uniform(-0.5, 1.5, n), (), 0.3
    if corner:
        lo[2], hi[2] = -3.14, 3.14
        x0, periodic, sigma0 = hi.copy(), (2,), 1.0
    draws = rng.standard_normal((generations, popsize, n))
    return dict(x0=x0, sigma0=sigma0, lower=lo, upper=hi, popsize=popsize, periodic=periodic), draws, f


def moved_fraction(search):
    """Share of the last population's coordinates that the boundary rule folded or wrapped."""
    g = search.m[None, :] + (search.sigma * search.scale)[None, :] * search.y
    return float(np.mean(search.phenotype(g) != g))
