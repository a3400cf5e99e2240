"""What hmc.py / nuts.py share: the kernel factory, and the shape plumbing -- the reference works on one chain
(position of shape () or (D,)); the engine adds a leading chain axis."""
from __future__ import annotations

import numpy as np
import torch

from .engine import _dev_f64, get_engine, rng_to_device
from .integrators import IntegratorState
from .trajectory import Diagnostics


class Layout:
    """How user-facing arrays map to the engine's [C, D] rows."""

    def __init__(self, shape, batched: bool, num_chains: int):
        shape = tuple(shape)
        self.user_shape = shape
        if batched:
            if len(shape) == 0 or shape[0] != num_chains:
                raise ValueError(f"position must have leading dimension {num_chains} (one row per "
                                 f"chain of the RandomStream), got shape {shape}")
            self.C = num_chains
            self.D = int(np.prod(shape[1:])) if len(shape) > 1 else 1
            if len(shape) > 2:
                raise ValueError("position must be [C] or [C, D]")
        else:
            if len(shape) > 1:
                raise ValueError("position must be a scalar or a vector (use RandomStream(seeds=...) "
                                 "for many chains)")
            self.C = 1
            self.D = shape[0] if len(shape) == 1 else 1
        self.scalar_chain_shape = shape[:1] if batched else ()

    @property
    def scalar(self):  # a chain's position is a scalar (the reference's size-() random variable)
        return len(self.user_shape) == len(self.scalar_chain_shape)

    def rows(self, x, device):
        return _dev_f64(x, device).reshape(self.C, self.D).clone()

    def vec(self, t):  # [C, D] -> user shape
        return t.reshape(self.user_shape)

    def per_chain(self, t):  # [C] -> () or [C]
        return t.reshape(self.scalar_chain_shape)


def state_rows(state: IntegratorState, layout: Layout, device):
    q = layout.rows(state.position, device)
    U = _dev_f64(state.potential_energy, device).reshape(layout.C).clone()
    g = layout.rows(state.potential_energy_grad, device)
    return q, U, g


def new_state(q, logprob_fn, num_chains=None) -> IntegratorState:
    """Create a new HMC/NUTS state from a position (reference: aehmc/hmc.py:16-40):
    ``potential_energy = -logprob_fn(q)`` and its gradient, ``momentum=None``.

    ``q``: scalar / [D] for one chain, [C] / [C, D] for many (pass ``num_chains=C`` to mark
    a leading chain axis; a 2-D position is always read as [C, D])."""
    eng = get_engine()
    shape = tuple(q.shape) if hasattr(q, "shape") else np.shape(q)
    batched = (num_chains is not None) or len(shape) == 2
    C = shape[0] if batched else 1
    layout = Layout(shape, batched, C)
    rows = layout.rows(q, eng.device)
    from .targets import as_target
    logprob_fn = as_target(logprob_fn, layout.D, layout.scalar)  # (a Python function of the position: traced once)
    eng.set_target(logprob_fn, layout.D)
    if eng.metric_ndim is None or eng.metric_D != layout.D:
        # new_state needs no metric; bind a unit one so that the ctx is complete
        eng.set_metric(torch.ones(layout.D, dtype=torch.float64, device=eng.device), layout.D)
    eng.ensure_workspace(layout.C, 1)
    if not getattr(logprob_fn, "gradient_checked", True):  # a hand-written gradient: verified where it is first evaluated
        eng.check_gradient(rows)
        logprob_fn.gradient_checked = True
    U, g = eng.new_state(rows)
    return IntegratorState(position=layout.vec(rows), momentum=None,
                           potential_energy=layout.per_chain(U),
                           potential_energy_grad=layout.vec(g))


def diagnostics(layout: Layout, q, U, g, out, tree: bool) -> Diagnostics:
    """trajectory.py:379-384 record from the engine's [C, ...] outputs (``tree``: NUTS fields;
    HMC returns None for them as hmc.py:199-204 does)."""
    flags = out["flags"].bool()  # [2, C]: is_turning (HMC: the accept flag), is_diverging
    return Diagnostics(
        state=IntegratorState(position=layout.vec(q), momentum=layout.vec(out["momentum"]),
                              potential_energy=layout.per_chain(U),
                              potential_energy_grad=layout.vec(g)),
        acceptance_probability=layout.per_chain(out["acceptance_probability"]),
        num_doublings=layout.per_chain(out["num_doublings"]) if tree else None,
        is_turning=layout.per_chain(flags[0]) if tree else None,
        is_diverging=layout.per_chain(flags[1]),
        n_leapfrog=layout.per_chain(out["n_leapfrog"]))


def trajectory_lengths(num_integration_steps, num_samples: int):
    """``num_integration_steps`` of a ``sample`` call: None for a single integer (one L for every transition), or the
    ``num_samples`` per-transition lengths as a list of ints -- from a sequence, a numpy array or an integer tensor.
    A wrong count, a negative or a non-integer entry raise ``ValueError``."""
    x = num_integration_steps
    if isinstance(x, torch.Tensor):
        if x.ndim == 0:
            return None
        if x.dtype.is_floating_point or x.dtype == torch.bool or x.is_complex():
            raise ValueError("per-transition num_integration_steps must be an integer tensor")
        x = x.detach().cpu().numpy()
    if isinstance(x, (int, np.integer)) or np.ndim(x) == 0:
        return None
    arr = np.asarray(x)
    if arr.ndim != 1 or arr.shape[0] != int(num_samples):
        raise ValueError(f"per-transition num_integration_steps must hold num_samples = {int(num_samples)} lengths, got "
                         f"shape {tuple(arr.shape)}")
    if arr.dtype.kind not in "iu":
        if arr.dtype.kind != "f" or not np.all(arr == np.floor(arr)):
            raise ValueError("per-transition num_integration_steps must be integers")
    if np.any(arr < 0):
        raise ValueError("num_integration_steps must be >= 0 for every transition")
    return [int(v) for v in arr]


def histories(layout: Layout, out, n: int, keep_samples: bool):
    """(samples [N, ...], acceptance history, divergence history) of a sample() call."""
    samples = out["samples"].reshape((n,) + layout.user_shape) if keep_samples else None
    hist_shape = (n,) + layout.scalar_chain_shape
    return (samples, out["acceptance_history"].reshape(hist_shape),
            out["divergence_history"].bool().reshape(hist_shape))


def bind_target(k, eng, state: IntegratorState, layout: Layout, scalar):
    """Before an engine call of the kernel with the settings ``k`` (``step._hmc`` / ``step._nuts``): its generator states
    placed on the engine's device, the state as rows ``q, U, g`` and its target bound (``scalar``: what
    ``Engine.set_target`` hands to ``targets.as_target`` should a Python function still have to be traced)."""
    holder = k["holder"]
    if "rng" not in holder or holder["rng"].device != eng.device:  # (uploaded at construction when a GPU is there)
        holder["rng"] = holder["rng"].to(eng.device) if "rng" in holder else rng_to_device(k["rng_host"], eng.device)
    q, U, g = state_rows(state, layout, eng.device)
    eng.set_target(k["logprob_fn"], layout.D, scalar=scalar)
    return q, U, g


def make_kernel(srng, logprob_fn, *, nuts: bool, n_sites: int, settings: dict):
    """What ``hmc.new_kernel`` and ``nuts.new_kernel`` build alike, as ``(holder, bind, finish)``: ``holder["rng"]`` is
    the live device tensor of the ``n_sites`` generator states per chain drawn from ``srng``; ``bind(state,
    inverse_mass_matrix) -> eng, layout, q, U, g`` readies the engine for one call; ``finish(step, sample)`` returns
    ``step`` with ``sample``, the chain layout and the settings (``_nuts`` / ``_hmc``: for tests, resuming and the
    one-call warm-up of window_adaptation.run) attached."""
    rng_host = srng.sites(n_sites)
    holder = {}
    if torch.cuda.is_available():  # the generator states go to the device with the kernel, not with its first call
        holder["rng"] = rng_to_device(rng_host, get_engine().device)
    k = dict(srng=srng, rng_host=rng_host, holder=holder, logprob_fn=logprob_fn, **settings)

    def _bind(state: IntegratorState, inverse_mass_matrix):
        eng = get_engine()
        layout = Layout(tuple(state.position.shape), srng.batched, srng.num_chains)
        q, U, g = bind_target(k, eng, state, layout, layout.scalar)
        eng.set_metric(inverse_mass_matrix, layout.D)
        return eng, layout, q, U, g

    def finish(step, sample):
        step.sample = sample
        step.num_chains, step.batched = srng.num_chains, srng.batched
        setattr(step, "_nuts" if nuts else "_hmc", k)
        return step

    return holder, _bind, finish
