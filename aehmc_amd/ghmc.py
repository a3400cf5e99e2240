"""Generalised HMC with a persistent momentum and a non-reversible slice variable (Horowitz 1991; Neal 2020; the form of
Hoffman & Sountsov, "Tuning-Free Generalized Hamiltonian Monte Carlo", AISTATS 2022) -- thin wrapper over the HIP engine
(``aehmc_ghmc_sample``, csrc/ghmc_fused.cuh).

Every transition is exactly ONE leapfrog: the momentum is partially refreshed (``alpha``), kept between transitions and
flipped on rejection; the accept test compares against a slice variable that drifts by ``delta`` per transition instead
of drawing a random number.  The momentum is kept WHITENED, ``v ~ N(0, I)``: the preconditioner is a ``scale`` -- a
scalar or a ``[D]`` vector shared by all chains, in the role of ``sqrt(inverse_mass_matrix)`` -- so a momentum stays
valid when ``meads.run`` rewrites the scale between two transitions.  ``scale**2`` is an ``inverse_mass_matrix`` for the
HMC and NUTS kernels.

    kernel = ghmc.new_kernel(srng, logprob_fn)
    state = ghmc.new_state(q0, logprob_fn)
    state, (step_size, scale, alpha, delta), _ = meads.run(kernel, state, 1000)
    samples, info, acc, div = kernel.sample(state, step_size, scale, alpha, delta, 1000)
"""
from __future__ import annotations

from typing import Any, Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np

from ._common import bind_target, histories, make_kernel, new_state as _new_integrator_state
from .engine import EngineError, PerChain, _dev_f64
from .trajectory import Diagnostics


class GhmcState(NamedTuple):
    """The chain state of generalised HMC: ``momentum`` is whitened; ``momentum`` / ``slice`` None: the next transition
    draws them (the momentum as a full refreshment, the slice uniform on (-1, 1) from generator site #2)."""
    position: Any
    momentum: Optional[Any]
    potential_energy: Any
    potential_energy_grad: Any
    slice: Optional[Any] = None


def new_state(position, logprob_fn, num_chains=None) -> GhmcState:
    """``potential_energy = -logprob_fn(position)`` and its gradient; momentum and slice are left None."""
    s = _new_integrator_state(position, logprob_fn, num_chains)
    return GhmcState(s.position, None, s.potential_energy, s.potential_energy_grad, None)


def check_scale(scale):
    """``ValueError`` unless ``scale`` is ONE scalar or 1-D value shared by all chains."""
    if isinstance(scale, PerChain):
        raise ValueError("ghmc: the scale is shared by all chains (a scalar or [D]); a PerChain scale is not supported")
    ndim = scale.ndim if hasattr(scale, "ndim") else np.ndim(scale)
    if ndim > 1:
        raise ValueError(f"ghmc: the scale is a scalar or a [D] vector (a diagonal preconditioner), got {ndim} dimensions; "
                         "dense preconditioners are not supported")


def check_parameters(step_size, alpha, delta):
    """``ValueError`` unless step_size > 0, 0 < alpha <= 1, delta >= 0; returns them as floats."""
    eps, alpha, delta = float(step_size), float(alpha), float(delta)
    if not eps > 0:
        raise ValueError(f"ghmc: step_size must be positive, got {eps}")
    if not 0 < alpha <= 1:
        raise ValueError(f"ghmc: alpha must lie in (0, 1], got {alpha}")
    if not delta >= 0:
        raise ValueError(f"ghmc: delta must be >= 0, got {delta}")
    return eps, alpha, delta


def _scale_rows(scale, D, device):
    check_scale(scale)
    s = _dev_f64(scale, device).reshape(-1)
    if s.numel() not in (1, D):
        raise ValueError(f"ghmc: the scale must have 1 or {D} entries, got {s.numel()}")
    return s


def engine_call(fn, *args, **kwargs):
    """An engine call whose argument errors (a limit the engine names: code -2) surface as ``ValueError``."""
    try:
        return fn(*args, **kwargs)
    except EngineError as e:
        if "(-2)" in str(e):
            raise ValueError(str(e)) from e
        raise


def state_of(layout, q, U, g, out) -> GhmcState:
    return GhmcState(layout.vec(q), layout.vec(out["momentum"]), layout.per_chain(U), layout.vec(g),
                     layout.per_chain(out["slice"]))


def _diagnostics(layout, q, U, g, out) -> Diagnostics:
    flags = out["flags"].bool()  # [2, C]: the accept flag, is_diverging
    return Diagnostics(state=state_of(layout, q, U, g, out),
                       acceptance_probability=layout.per_chain(out["acceptance_probability"]), num_doublings=None,
                       is_turning=layout.per_chain(flags[0]), is_diverging=layout.per_chain(flags[1]),
                       n_leapfrog=layout.per_chain(out["n_leapfrog"]))


def new_kernel(srng, logprob_fn, divergence_threshold: int = 1000) -> Callable:
    """Build a generalised-HMC kernel.  ``logprob_fn``: a ``targets.Target`` or a Python function of the position.  Two
    generator sites are taken from ``srng``: #1 refreshes the momentum, #2 draws the initial slice variable (once).

    ``kernel(state, step_size, scale, alpha, delta) -> (Diagnostics, updates)``: one transition; ``Diagnostics.state`` is
    the new ``GhmcState`` and ``Diagnostics.is_turning`` carries the ACCEPT FLAG (the test draws no random number, so it
    is a function of the state; the C ABI reuses the same field).  ``updates[srng]`` are the generator states, as for HMC."""
    thr = float(divergence_threshold)
    holder, _, finish = make_kernel(srng, logprob_fn, nuts=False, n_sites=2, settings=dict(divergence_threshold=thr))

    def _call(state: GhmcState, step_size, scale, alpha, delta, n, keep_samples):
        from ._common import Layout
        from .engine import get_engine
        params = check_parameters(step_size, alpha, delta)
        check_scale(scale)
        eng = get_engine()
        layout = Layout(tuple(state.position.shape), srng.batched, srng.num_chains)
        q, U, g = bind_target(step._ghmc, eng, state, layout, layout.scalar)
        s = _scale_rows(scale, layout.D, eng.device)
        out = engine_call(eng.ghmc_sample, holder["rng"], params, s, thr, n, q, U, g, state.momentum,
                          getattr(state, "slice", None), keep_samples)
        return layout, q, U, g, out

    def step(state: GhmcState, step_size, scale, alpha, delta) -> Tuple[Diagnostics, Dict]:
        """One transition for every chain."""
        layout, q, U, g, out = _call(state, step_size, scale, alpha, delta, 1, False)
        return _diagnostics(layout, q, U, g, out), {srng: holder["rng"]}

    def sample(state: GhmcState, step_size, scale, alpha, delta, num_samples: int, keep_samples: bool = True):
        """``num_samples`` consecutive transitions per chain in ONE launch.  Returns what ``hmc``'s ``.sample`` returns:
        ``(samples [N, ...], Diagnostics of the last transition, acceptance history [N, ...], divergence history [N, ...])``;
        ``Diagnostics.n_leapfrog`` is ``num_samples``."""
        n = int(num_samples)
        if n < 1:
            raise ValueError("ghmc: num_samples must be at least 1")
        layout, q, U, g, out = _call(state, step_size, scale, alpha, delta, n, keep_samples)
        samples, acc_hist, div_hist = histories(layout, out, n, keep_samples)
        return samples, _diagnostics(layout, q, U, g, out), acc_hist, div_hist

    finish(step, sample)
    step._ghmc = step._hmc  # (not an HMC kernel: chees.run and window_adaptation.run must not take it for one)
    del step._hmc
    return step
