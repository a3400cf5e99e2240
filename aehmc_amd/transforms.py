"""Constrained parameters: transforms between a model's parameters and the unconstrained position the samplers move.

The reference gets this from aeppl (``TransformValuesRewrite`` with a ``LogTransform`` on the regression notebook's noise
scale); here a ``Model`` ties an ordered set of named transforms to a log-density written on the CONSTRAINED scale:

    model = transforms.Model({"w": transforms.Real(5), "sigma": transforms.Positive()}, logprob)
    state = nuts.new_state(model.unconstrain({"w": w0, "sigma": s0}), model)      # model(q) is a logprob_fn
    draws = model.constrain(samples)                                              # [..., D_in] -> [..., D_out], one kernel
    summary.run(kernel, state, eps, imm, n, constrain=model)                      # summaries of sigma, not of log sigma

With x the unconstrained coordinates of a parameter, theta the constrained ones and ldj the log of the absolute Jacobian
determinant (operation order as in csrc/constrain.cuh and include/aehmc_hip.h):

    Real(n=())                 theta = x                                   ldj = 0
    LowerBound(lo, n=())       theta = lo + exp(x)                         ldj = x             (Positive = LowerBound(0))
    UpperBound(hi, n=())       theta = hi - exp(x)                         ldj = x
    Interval(lo, hi, n=())     theta = lo + (hi - lo) s                    ldj = log(hi - lo) - softplus(x) - softplus(-x)
                               s = 1 / (1 + exp(-x)) where x >= 0, else e / (1 + e), e = exp(x)
    Ordered(n), 2 <= n <= 64   theta_0 = x_0, theta_j = theta_{j-1} + exp(x_j)         ldj = sum_{j >= 1} x_j
    Simplex(K), 2 <= K <= 64   theta_j = exp(xt_j - L), xt = (x_0 ... x_{K-2}, 0),     ldj = sum_j xt_j - K L
                               L = logsumexp(xt) about its maximum, summed ascending   (K - 1 coordinates in, K out)

``n`` is ``()`` (a scalar parameter) or a length (a vector): traced values are scalars and vectors.  ``lo`` / ``hi`` are
floats or arrays of the parameter's shape.  The limit of 64 is the tracer's: running sums and a softmax over traced
scalars are written out term by term.  A Simplex with +inf among its coordinates gives NaN (inf - inf).

``model(q)`` is built from operations ``aehmc_amd.tracing`` already records (slices, ``np.exp``, ``scipy.special.expit``,
``tracing.softplus``, ``tracing.logsumexp``, lists of scalars), so it is traced like any other ``logprob_fn`` -- and it
evaluates on a plain numpy vector too.  A model of ONE vector parameter under a coordinate-wise transform whose
``logprob`` returns one ``sum`` over that parameter keeps the per-coordinate form (``targets.Custom``: every kernel
family): the Jacobian term joins the body of that sum.  Anything else is a joint density (``targets.CustomJoint``)."""
from __future__ import annotations

import math
import operator
from typing import Mapping

import numpy as np

from . import tracing
from .utils import RaveledParamsMap

MAX_LEN = 64  # aehmc_hip.h: AEHMC_CONSTRAIN_MAX_LEN -- the longest Ordered / Simplex (tracing: sums over lists of scalars)
# aehmc_hip.h: AEHMC_CONSTRAIN_REAL ... _SIMPLEX
K_REAL, K_LOWER, K_UPPER, K_INTERVAL, K_ORDERED, K_SIMPLEX = range(6)
# aehmc_hip.h: aehmc_constrain_entry, 40 bytes
ENTRY = np.dtype([("kind", "<i4"), ("pos", "<i4"), ("len", "<i4"), ("reserved", "<i4"), ("first", "<i8"), ("lo", "<f8"),
                  ("hi", "<f8")])


def _shape(n, what):
    if isinstance(n, (tuple, list)):
        shape = tuple(n)
    else:
        shape = (n,)
    if len(shape) > 1:
        raise ValueError(f"{what}: a parameter is a scalar, n=(), or a vector, n=length (traced values are scalars and "
                         f"vectors), got shape {shape}")
    try:
        shape = tuple(operator.index(s) for s in shape)
    except TypeError:
        raise ValueError(f"{what}: the length must be an integer, got {n!r}") from None
    if shape and shape[0] < 1:
        raise ValueError(f"{what}: the length must be positive, got {shape[0]}")
    return shape


def _bound(v, shape, what):
    """A bound -- a float or an array of the parameter's shape -- as a finite fp64 array of that shape."""
    a = np.asarray(v, dtype=np.float64)
    if a.ndim > 1:
        raise ValueError(f"{what}: a bound is a float or an array of the parameter's shape {shape}, got shape {a.shape}")
    if a.ndim == 1 and a.shape != shape:
        raise ValueError(f"{what}: a bound is a float or an array of the parameter's shape {shape}, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: the bounds must be finite")
    return np.broadcast_to(a, shape).copy()


class Transform:
    """One parameter's map.  ``shape``: the constrained parameter's; ``n_in`` / ``n_out``: coordinates in and out."""

    kind = None

    def __init__(self, n=()):
        self.shape = _shape(n, type(self).__name__)
        self.n_in = self.n_out = self.shape[0] if self.shape else 1
        self.lo = np.zeros(self.shape)
        self.hi = np.zeros(self.shape)

    coordinate_wise = True

    @staticmethod
    def _value(a):
        """a bound as a float where every coordinate has the same one (a literal in the traced source), else the array"""
        flat = a.reshape(-1)
        return float(flat[0]) if (flat == flat[0]).all() else a

    # forward(x) -> (theta, ldj or None) on traced values or numpy; inverse(theta, name) on float64 torch [C, n_out]
    def forward(self, x):
        raise NotImplementedError

    def entries(self, first):
        e = np.zeros(self.n_out, dtype=ENTRY)
        e["kind"], e["len"] = self.kind, 1
        e["first"] = first + np.arange(self.n_out)
        e["lo"], e["hi"] = self.lo.reshape(-1), self.hi.reshape(-1)
        return e

    def __repr__(self):
        return f"{type(self).__name__}({self.shape[0] if self.shape else ()})"


def _total(x):
    return x.sum() if getattr(x, "ndim", 0) else x


class Real(Transform):
    kind = K_REAL

    def forward(self, x):
        return x, None

    def ldj_vector(self, x):
        return None

    def inverse(self, t, name):
        return t


class LowerBound(Transform):
    kind = K_LOWER

    def __init__(self, lo=0.0, n=()):
        super().__init__(n)
        self.lo = _bound(lo, self.shape, type(self).__name__)

    def forward(self, x):
        return self._value(self.lo) + np.exp(x), _total(x)

    def ldj_vector(self, x):
        return x

    def inverse(self, t, name):
        import torch
        lo = torch.as_tensor(self.lo.reshape(-1))
        if not bool((t > lo).all()):
            raise ValueError(f"unconstrain: {name} has a value that is not above its lower bound")
        return torch.log(t - lo)


class Positive(LowerBound):
    def __init__(self, n=()):
        super().__init__(0.0, n)


class UpperBound(Transform):
    kind = K_UPPER

    def __init__(self, hi=0.0, n=()):
        super().__init__(n)
        self.hi = _bound(hi, self.shape, type(self).__name__)

    def forward(self, x):
        return self._value(self.hi) - np.exp(x), _total(x)

    def ldj_vector(self, x):
        return x

    def inverse(self, t, name):
        import torch
        hi = torch.as_tensor(self.hi.reshape(-1))
        if not bool((t < hi).all()):
            raise ValueError(f"unconstrain: {name} has a value that is not below its upper bound")
        return torch.log(hi - t)


class Interval(Transform):
    kind = K_INTERVAL

    def __init__(self, lo, hi, n=()):
        super().__init__(n)
        self.lo = _bound(lo, self.shape, "Interval")
        self.hi = _bound(hi, self.shape, "Interval")
        if not (self.lo < self.hi).all():
            raise ValueError("Interval: lo >= hi; the bounds must satisfy lo < hi in every coordinate")
        self.width = self.hi - self.lo
        if not np.isfinite(self.width).all():
            raise ValueError("Interval: hi - lo overflows")

    def forward(self, x):
        from scipy.special import expit
        theta = self._value(self.lo) + self._value(self.width) * expit(x)
        return theta, _total(self.ldj_vector(x))

    def ldj_vector(self, x):
        return self._value(np.log(self.width)) - tracing.softplus(x) - tracing.softplus(-x)

    def inverse(self, t, name):
        import torch
        lo, hi = torch.as_tensor(self.lo.reshape(-1)), torch.as_tensor(self.hi.reshape(-1))
        if not bool(((t > lo) & (t < hi)).all()):
            raise ValueError(f"unconstrain: {name} has a value that is not inside its interval")
        u = (t - lo) / (hi - lo)
        return torch.log(u) - torch.log1p(-u)


def _segment_length(n, what):
    shape = _shape(n, what)
    if not shape:
        raise ValueError(f"{what}: needs a length")
    if not 2 <= shape[0] <= MAX_LEN:
        raise ValueError(f"{what}: the length must be in [2, {MAX_LEN}] (sums over traced scalars are written out term by "
                         f"term, up to {MAX_LEN}), got {shape[0]}")
    return shape


class Ordered(Transform):
    kind = K_ORDERED
    coordinate_wise = False

    def __init__(self, n):
        super().__init__(_segment_length(n, "Ordered"))

    def forward(self, x):
        n = self.n_out
        theta = [x[0]]
        for j in range(1, n):
            theta.append(theta[-1] + np.exp(x[j]))
        ldj = x[1]
        for j in range(2, n):
            ldj = ldj + x[j]
        return np.stack(theta), ldj

    def entries(self, first):
        e = super().entries(first)
        e["pos"], e["len"], e["first"] = np.arange(self.n_out), self.n_out, first
        return e

    def inverse(self, t, name):
        import torch
        gaps = t[:, 1:] - t[:, :-1]
        if not bool((gaps > 0).all()) or bool(torch.isnan(t).any()):
            raise ValueError(f"unconstrain: {name} is not strictly increasing")
        return torch.cat([t[:, :1], torch.log(gaps)], dim=1)


class Simplex(Transform):
    kind = K_SIMPLEX
    coordinate_wise = False
    SUM_TOL = 1e-8  # |sum(theta) - 1| a value handed to unconstrain may have

    def __init__(self, K):
        super().__init__(_segment_length(K, "Simplex"))
        self.n_in = self.n_out - 1

    def forward(self, x):
        K = self.n_out
        xt = [x[j] for j in range(K - 1)] + [0.0]
        L = tracing.logsumexp(xt)
        theta = np.stack([np.exp(v - L) for v in xt])
        tot = xt[0]
        for v in xt[1:]:
            tot = tot + v
        return theta, tot - float(K) * L

    def entries(self, first):
        e = super().entries(first)
        e["pos"], e["len"], e["first"] = np.arange(self.n_out), self.n_out, first
        return e

    def inverse(self, t, name):
        import torch
        if not bool((t > 0).all()) or not bool(((t.sum(dim=1) - 1.0).abs() <= self.SUM_TOL).all()):
            raise ValueError(f"unconstrain: {name} is not a point of the open simplex (positive entries that sum to 1 "
                             f"within {self.SUM_TOL})")
        lt = torch.log(t)
        return lt[:, :-1] - lt[:, -1:]


class Model:
    """``spec``: an ordered mapping name -> Transform.  ``logprob(**params)``: the log-density on the constrained scale,
    every parameter handed over by name as a traced scalar or vector.  The instance is a ``logprob_fn`` of the
    unconstrained position, ``model(q) = logprob(**theta(q)) + sum of ldj`` (``include_jacobian=False``: without the
    Jacobian term -- the density a mode finder wants), and one stable callable: ``new_kernel(srng, model)`` and
    ``new_state(q0, model)`` trace it once.

    ``dim`` / ``constrained_dim``: coordinates in and out (one more out per Simplex).  ``params_map``: the
    ``RaveledParamsMap`` of the constrained layout; ``unravel(y)`` gives ``{name: view}``.  ``unconstrain(params)``:
    constrained values to a position, on the host in float64 torch.  ``constrain(samples)``: positions to constrained
    draws on the device (csrc/constrain.cuh).  ``table``: the kernel's per-output entries (a numpy record array)."""

    def __init__(self, spec, logprob, include_jacobian: bool = True):
        if not isinstance(spec, Mapping) or not spec:
            raise ValueError("spec must be a non-empty mapping from parameter names to transforms")
        for k, t in spec.items():
            if not isinstance(k, str) or not isinstance(t, Transform):
                raise ValueError(f"spec maps names to transforms, got {k!r}: {type(t).__name__}")
        if not callable(logprob):
            raise ValueError("logprob must be callable: logprob(**params) on the constrained scale")
        self.spec = dict(spec)
        self.logprob = logprob
        self.include_jacobian = bool(include_jacobian)
        self._in, self._out = {}, {}
        a = b = 0
        tab = []
        for k, t in self.spec.items():
            self._in[k], self._out[k] = slice(a, a + t.n_in), slice(b, b + t.n_out)
            tab.append(t.entries(a))
            a, b = a + t.n_in, b + t.n_out
        self.dim, self.constrained_dim = a, b
        self.table = np.concatenate(tab)
        self.params_map = RaveledParamsMap({k: np.zeros(t.shape) for k, t in self.spec.items()})
        self._device_tables = {}

    # ---------------------------------------------------------------------------------------------- the density
    def __call__(self, q):
        if (q.ndim if hasattr(q, "ndim") else np.ndim(q)) == 0:  # a scalar position: one scalar parameter
            if self.dim != 1:
                raise ValueError(f"a scalar position for a model of {self.dim} coordinates")
            pick = lambda s, t: q  # noqa: E731
        else:
            if len(q) != self.dim:
                raise ValueError(f"the model has {self.dim} unconstrained coordinates, the position has {len(q)}")
            pick = lambda s, t: q[s] if t.shape or t.n_in != 1 else q[s.start]  # noqa: E731
        xs = {k: pick(self._in[k], t) for k, t in self.spec.items()}
        params, ldjs = {}, []
        for k, t in self.spec.items():
            params[k], ldj = t.forward(xs[k])
            if ldj is not None:
                ldjs.append(ldj)
        lp = self.logprob(**params)
        if not self.include_jacobian or not ldjs:
            return lp
        fused = self._fused(lp, xs)
        if fused is not None:
            return fused
        for ldj in ldjs:
            lp = lp + ldj
        return lp

    def _fused(self, lp, xs):
        """One vector parameter, a coordinate-wise transform, a density that is one sum over it: the Jacobian term inside
        that sum's body (the per-coordinate form survives: targets.Custom), else None."""
        if len(self.spec) != 1:
            return None
        (k, t), = self.spec.items()
        x = xs[k]
        if not (t.coordinate_wise and t.shape and isinstance(x, tracing.V) and isinstance(lp, tracing.S)):
            return None
        if lp.op != "sum" or lp.args[1] != self.dim:
            return None
        v, n, body = lp.args
        term = t.ldj_vector(x).at(tracing.Idx.var(v))
        return tracing.S(lp.ctx, "sum", (v, n, body + term), True)

    # ---------------------------------------------------------------------------------------------- layouts
    def unravel(self, y):
        """``{name: view}`` of constrained draws y [..., D_out]."""
        if y.shape[-1] != self.constrained_dim:
            raise ValueError(f"expected [..., {self.constrained_dim}] constrained values, got {tuple(y.shape)}")
        lead = tuple(y.shape[:-1])
        return {k: y[..., self._out[k]].reshape(lead + t.shape) for k, t in self.spec.items()}

    def unconstrain(self, params):
        """``{name: constrained value [C, ...] or [...]}`` -> the position [C, D_in] / [D_in] (float64 torch, on the
        host): what ``new_state`` takes.  A value outside its support is a ``ValueError`` that names the parameter."""
        import torch
        if not isinstance(params, Mapping) or set(params) != set(self.spec):
            raise ValueError(f"unconstrain takes a value for each of {list(self.spec)}")
        vals, batch = {}, None
        for k, t in self.spec.items():
            v = params[k]
            v = v.detach().to(device="cpu", dtype=torch.float64) if isinstance(v, torch.Tensor) else \
                torch.as_tensor(np.asarray(v, dtype=np.float64))
            if tuple(v.shape) == t.shape:
                b = None
            elif v.ndim == len(t.shape) + 1 and tuple(v.shape[1:]) == t.shape:
                b = v.shape[0]
            else:
                raise ValueError(f"unconstrain: {k} must have shape {t.shape} or [C, *{t.shape}], got {tuple(v.shape)}")
            if b is not None:
                if batch is not None and b != batch:
                    raise ValueError(f"unconstrain: {k} has {b} chains, another parameter {batch}")
                batch = b
            vals[k] = (v, b)
        C = batch if batch is not None else 1
        cols = []
        for k, t in self.spec.items():
            v, b = vals[k]
            v = v.reshape(1, t.n_out).expand(C, t.n_out) if b is None else v.reshape(C, t.n_out)
            if bool(torch.isnan(v).any()):
                raise ValueError(f"unconstrain: {k} holds a NaN")
            cols.append(t.inverse(v, k))
        x = torch.cat(cols, dim=1).contiguous()
        return x if batch is not None else x[0]

    # ---------------------------------------------------------------------------------------------- the device map
    def _table_on(self, eng):
        import torch
        if eng.device not in self._device_tables:
            self._device_tables[eng.device] = torch.from_numpy(self.table.view(np.uint8).copy()).to(eng.device)
        return self._device_tables[eng.device]

    def _constrain_rows(self, eng, x, out=None):
        """x [R, D_in] -> [R, D_out] on the engine's device (``out``: a buffer of that shape)."""
        return eng.constrain(x, self._table_on(eng), self.constrained_dim, out)

    def constrain(self, samples, out=None):
        """Positions [..., D_in] (float64, contiguous, on the device) -> constrained draws [..., D_out], one kernel, out
        of place (``out``: a contiguous float64 tensor of the result's shape that shares no memory with the input)."""
        import torch

        from .engine import get_engine
        if not isinstance(samples, torch.Tensor) or samples.dtype != torch.float64 or not samples.is_contiguous():
            raise ValueError("constrain takes a contiguous float64 torch tensor [..., D_in]")
        if samples.ndim < 1 or samples.shape[-1] != self.dim:
            raise ValueError(f"constrain takes [..., {self.dim}] positions, got {tuple(samples.shape)}")
        lead = tuple(samples.shape[:-1])
        want = lead + (self.constrained_dim,)
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != want or
                                out.dtype != torch.float64 or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float64 tensor {want}")
        eng = get_engine(samples.device if samples.is_cuda else None)
        y = self._constrain_rows(eng, samples.reshape(-1, self.dim),
                                 None if out is None else out.reshape(-1, self.constrained_dim))
        return y.reshape(want)

    # ---------------------------------------------------------------------------------------------- vector functions
    def pointwise(self, fn):
        """``fn(**params)`` -- written on the constrained scale, with the names ``logprob`` takes -- as a
        ``summary.Pointwise`` of the UNCONSTRAINED position (``dim`` is ``model.dim``): the model's pointwise
        log-likelihood, for ``summary.loo`` / ``waic`` and ``summary.run(..., waic=)``.  It is traced as a function of the
        constrained vector; when called, the rows go through ``constrain``'s kernel a block at a time, so no transform is
        evaluated per observation and no full constrained copy is made."""
        from .summary import Pointwise

        def on_constrained(y):
            return fn(**{k: y[self._out[k]] if t.shape else y[self._out[k].start] for k, t in self.spec.items()})

        return Pointwise(on_constrained, self.dim, _model=self)

    def __repr__(self):
        return f"Model({', '.join(f'{k}: {t!r}' for k, t in self.spec.items())})"
