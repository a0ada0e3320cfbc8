"""CMA-ES search on the HIP engine: `CmaSearch`, an ask / tell optimiser whose generations never wait for the host.

The arithmetic lives in csrc/ag_cma.hip (ag_cma_init / ag_cma_ask / ag_cma_tell of libadaptigraph_hip_cma.so,
include/adaptigraph_amd_cma.h): standard
(mu/mu_w, lambda)-CMA-ES with positive weights, fp64, the whole optimiser state in one device buffer.  This module draws the
standard-normal numbers (one torch.randn per generation), owns the buffers and hands device pointers to the C-ABI.  There is no
CPU path.

    search = CmaSearch(x0, 0.25, lower, upper, popsize=1024, device="cuda", maximize=True)
    for _ in range(generations):
        x = search.ask()                       # (popsize, n) fp32 on the device, inside the limits
        search.tell(reward_of(x))              # (popsize,) fp32 on the device; nothing is read back
    best_value, best_x = search.result()[:2]   # the one read-back

Limits are met by folding (a triangle wave over [lower, upper], continuous, the identity inside), periodic coordinates are
wrapped into [-period/2, period/2) first; `scale` is the unit sigma is relative to, per coordinate.  With `dynamics_error_sweep` as
the function under `tell` this is the device-side partner of the reference's `optimize_cma` loop
(physics_param_optimizer.py:125-175).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .context import ptr, current_stream, _require_gpu

STATUS_BITS = {0: "fewer than mu of the values told were not NaN: the generation was skipped",
               1: "a non-finite number or an eigenvalue <= 0 appeared in the update: it was dropped"}
_HEADER = ("n", "popsize", "mu", "maximize", "g", "status", "sigma", "mu_eff", "c_sigma", "d_sigma", "c_c", "c_1", "c_mu", "chi_n",
           "period", "best_value", "best_generation")


def state_fields(n, mu):
    """name -> (offset, shape) of the arrays of a state buffer, in doubles (include/adaptigraph_amd_cma.h)."""
    out, at = {}, _lib.CMA_HDR
    for name, shape in (("m", (n,)), ("C", (n, n)), ("p_sigma", (n,)), ("p_c", (n,)), ("A", (n, n)), ("A_inv", (n, n)),
                        ("scale", (n,)), ("lo", (n,)), ("hi", (n,)), ("periodic", (n,)), ("best_x", (n,)), ("weights", (mu,))):
        out[name] = (at, shape)
        at += int(np.prod(shape))
    return out


class CmaSearch:
    """CmaSearch(x0, sigma0, lower, upper, popsize=None, device=..., scale=None, periodic=(), period=2 pi, maximize=False).

    x0 (n,) start mean; sigma0 the start step in units of `scale`; lower / upper (n,) limits, either may be infinite;
    popsize None: 4 + floor(3 ln n); scale None: upper - lower where both are finite, else 1 - a periodic coordinate takes
    min(upper - lower, period); periodic: indices of the coordinates that wrap.  1 <= n <= 64 and 4 <= popsize <= 32768, else
    NotImplementedError before anything is enqueued."""

    def __init__(self, x0, sigma0, lower, upper, popsize=None, device="cuda", scale=None, periodic=(), period=2.0 * math.pi,
                 maximize=False):
        def host(v):
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            return np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))

        # a device tensor as x0 is copied into the state on the device: the caller's stream is not waited for
        self._x0_dev = x0.detach() if isinstance(x0, torch.Tensor) and x0.is_cuda else None
        x0 = np.zeros(x0.numel()) if self._x0_dev is not None else host(x0)
        n = x0.size
        lo, hi = np.broadcast_to(host(lower), (n,)).copy(), np.broadcast_to(host(upper), (n,)).copy()
        if np.any(lo == hi):
            raise ValueError(f"CmaSearch: lower == upper at coordinate(s) {np.nonzero(lo == hi)[0].tolist()}: fix such a coordinate "
                             "outside the search")
        flags = np.zeros(n, dtype=np.int32)
        flags[np.asarray(list(periodic), dtype=np.int64)] = 1
        if scale is None:
            both = np.isfinite(lo) & np.isfinite(hi)
            scale = np.where(both, hi - lo, 1.0)
            scale = np.where(flags != 0, np.minimum(scale, float(period)), scale)
        else:
            scale = np.broadcast_to(host(scale), (n,)).copy()
        popsize = int(popsize) if popsize is not None else 4 + int(math.floor(3.0 * math.log(n)))
        if not (1 <= n <= _lib.CMA_MAX_N and _lib.CMA_MIN_POP <= popsize <= _lib.CMA_MAX_POP):
            raise NotImplementedError(f"CmaSearch: n = {n}, popsize = {popsize} outside 1 <= n <= {_lib.CMA_MAX_N}, "
                                      f"{_lib.CMA_MIN_POP} <= popsize <= {_lib.CMA_MAX_POP}")
        self.device = torch.device(device)
        self.n, self.popsize, self.mu, self.maximize = n, popsize, popsize // 2, bool(maximize)
        self.waits = 0
        self.order = self.improved = None
        self._y = self._x = None
        self._init = (x0, float(sigma0), np.ascontiguousarray(scale, dtype=np.float64), lo, hi, flags, float(period))
        self._state = None
        if self.device.type == "cuda" and torch.cuda.is_available():
            self._upload()

    def _upload(self):
        dev = _require_gpu(self.device)
        self._lib = lib = _lib.load_cma()
        self._dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        words = lib.ag_cma_state_doubles(self.n, self.popsize)
        if words < 0:
            raise NotImplementedError(f"CmaSearch: the library serves no state of n = {self.n}, popsize = {self.popsize}")
        x0, sigma0, scale, lo, hi, flags, period = self._init
        self._state = torch.zeros(words, dtype=torch.float64, device=dev)
        hp = lambda a: C.c_void_p(a.ctypes.data)
        self._check(lib.ag_cma_init(self._dev_index, current_stream(dev), self.n, self.popsize, hp(x0), sigma0, hp(scale), hp(lo), hp(hi),
                                      hp(flags), period, int(self.maximize), ptr(self._state)))
        if self._x0_dev is not None:
            at = state_fields(self.n, self.mu)["m"][0]
            self._state[at:at + self.n] = self._x0_dev.reshape(-1).to(device=dev, dtype=torch.float64)
        self.order = torch.zeros(self.popsize, dtype=torch.int32, device=dev)
        self.improved = torch.zeros(1, dtype=torch.bool, device=dev)

    def _check(self, rc):
        """the engine's error mapping (context.Engine.check) on this library's codes"""
        if rc == 0:
            return
        msg = self._lib.ag_cma_last_error().decode()
        if rc == _lib.AG_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        if rc == _lib.AG_ERR_INVALID:
            raise AssertionError(msg)
        raise RuntimeError(f"adaptigraph_amd: {msg} (code {rc})")

    def _need(self):
        if self._state is None:
            _require_gpu(self.device)                           # raises the package's "no CPU fallback"
            self._upload()
        return self._lib

    def ask(self, draws=None):
        """One population -> (popsize, n) fp32 phenotypes on the device.  `draws`: the (popsize, n) standard-normal numbers to use
        instead of one torch.randn (tests, replays)."""
        lib = self._need()
        dev = self._state.device
        if draws is None:
            z = torch.randn((self.popsize, self.n), dtype=torch.float64, device=dev)
        else:
            z = torch.as_tensor(draws).detach().to(device=dev, dtype=torch.float64).contiguous()
            assert z.shape == (self.popsize, self.n)
        self._y = torch.empty((self.popsize, self.n), dtype=torch.float64, device=dev)
        self._x = torch.empty((self.popsize, self.n), dtype=torch.float32, device=dev)
        self._check(lib.ag_cma_ask(self._dev_index, current_stream(dev), ptr(self._state), ptr(z), ptr(self._y), ptr(self._x)))
        return self._x

    def tell(self, values):
        """The update from the (popsize,) fp32 device tensor of the last ask's values.  Leaves `order` (int32, best first) and
        `improved` (bool, one element) on the device; nothing waits."""
        lib = self._need()
        dev = self._state.device
        assert self._y is not None, "tell() needs the population of an ask()"
        assert isinstance(values, torch.Tensor) and values.shape == (self.popsize,)
        v = values.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.order = torch.empty(self.popsize, dtype=torch.int32, device=dev)      # fresh: the caller may keep the last ones
        self.improved = torch.empty(1, dtype=torch.bool, device=dev)
        self._check(lib.ag_cma_tell(self._dev_index, current_stream(dev), ptr(self._state), ptr(self._y), ptr(self._x), ptr(v),
                                      ptr(self.order), ptr(self.improved)))

    # ------------------------------------------------------------------------------------------------ read-backs
    def _host_state(self):
        self._need()
        self.waits += 1
        return self._state.cpu().numpy()

    def _fold(self, g, s):
        """bound() of the kernels on a host vector (the mean's phenotype)."""
        lo, hi, per, P = s["lo"], s["hi"], s["periodic"] != 0, s["period"]
        g = np.array(g, dtype=np.float64)
        r = np.fmod(g + 0.5 * P, P)
        r = np.where(r < 0, r + P, r)
        r = np.where(r >= P, 0.0, r)
        g = np.where(per, r - 0.5 * P, g)
        box = np.isfinite(lo) & np.isfinite(hi)
        w = np.where(box, hi - lo, 1.0)
        t = np.fmod(g - np.where(box, lo, 0.0), 2 * w)
        t = np.where(t < 0, t + 2 * w, t)
        f = np.clip(lo + np.where(t <= w, t, 2 * w - t), lo, hi)
        return np.where(box & ~((g >= lo) & (g <= hi)), f, g)

    def state(self):
        """A host copy of the state's named fields (one read-back)."""
        raw = self._host_state()
        out = {k: float(raw[i]) for i, k in enumerate(_HEADER)}
        for k in ("n", "popsize", "mu", "maximize", "g", "status", "best_generation"):
            out[k] = int(out[k])
        for k, (at, shape) in state_fields(self.n, self.mu).items():
            out[k] = raw[at:at + int(np.prod(shape))].reshape(shape).copy()
        return out

    def result(self):
        """The one read-back of a search -> (best value, best phenotype (n,) fp32, the mean's phenotype (n,) fp32, sigma,
        generations told, status).  A set status bit raises RuntimeError naming it, once: the bit is cleared."""
        s = self.state()
        if s["status"]:
            self._state[5:6].zero_()
            said = "; ".join(f"bit {b}: {why}" for b, why in STATUS_BITS.items() if s["status"] >> b & 1)
            raise RuntimeError(f"CmaSearch: status {s['status']} ({said})")
        return (s["best_value"], s["best_x"].astype(np.float32), self._fold(s["m"], s).astype(np.float32), s["sigma"], s["g"],
                s["status"])
