"""MEADS warm-up for generalised HMC: step size, diagonal preconditioner, momentum damping and slice drift from all
chains together (Hoffman & Sountsov, "Tuning-Free Generalized Hamiltonian Monte Carlo", AISTATS 2022; this is the
all-chains variant, without the paper's folds).

All four parameters are closed-form cross-chain statistics of the current positions and potential gradients
(csrc/meads.cuh: an estimate of the largest eigenvalue of the standardised positions and of the scaled gradients, from
the engine's symmetric rank-C product) -- no dual averaging, no learning rate, no target acceptance rate, no windows.
The transitions are ``ghmc`` kernels: one leapfrog each, every chain the same work.

    kernel = ghmc.new_kernel(srng, logprob_fn)
    state, (step_size, scale, alpha, delta), _ = meads.run(kernel, ghmc.new_state(q0, logprob_fn), 1000)
    samples, info, acc, div = meads.sample(kernel, state, step_size, scale, alpha, delta, num_samples)

``scale`` is a ``[D]`` device tensor in the role of ``sqrt(inverse_mass_matrix)``: ``scale**2`` is an
``inverse_mass_matrix`` for the HMC and NUTS kernels."""
from __future__ import annotations

from typing import NamedTuple, Tuple

import torch

from ._common import bind_target
from .engine import _dev_f64, get_engine
from .ghmc import GhmcState, engine_call, state_of
from .window_adaptation import _layout


class MeadsState(NamedTuple):
    """The adaptation state (device arrays; ``aehmc_meads_state``)."""
    params: torch.Tensor    # [3]: step size, alpha, delta
    scale: torch.Tensor     # [D]
    count: torch.Tensor     # [1] int64: updates done
    skipped: torch.Tensor   # [1] int64: updates the guard refused
    position_shape: Tuple = ()
    batched: bool = False


def _ghmc_settings(kernel):
    k = getattr(kernel, "_ghmc", None)
    if k is None:
        raise ValueError("meads works around a generalised-HMC kernel (ghmc.new_kernel); HMC and NUTS kernels have their "
                         "own warm-ups (window_adaptation.run, chees.run)")
    return k


def _options(step_size_multiplier, damping_slowdown, initial_step_size):
    mult, slow, eps0 = float(step_size_multiplier), float(damping_slowdown), float(initial_step_size)
    if not mult > 0 or not eps0 > 0:
        raise ValueError("meads: step_size_multiplier and initial_step_size must be positive")
    return mult, slow, eps0


def _chains(layout):
    if layout.C < 2:
        raise ValueError(f"meads takes its statistics ACROSS chains: at least 2 are needed, got {layout.C}")
    return layout.C, layout.D


def _parameters(st):
    """``(step_size, scale, alpha, delta)``: three Python floats (one read-back) and the [D] device tensor."""
    eps, alpha, delta = st["params"].tolist()
    return eps, st["scale"], alpha, delta


def _as_state(st, layout) -> MeadsState:
    return MeadsState(st["params"], st["scale"], st["count"], st["skipped"], layout.user_shape,
                      bool(layout.scalar_chain_shape))


def adaptation(*, step_size_multiplier=0.5, damping_slowdown=1.0, initial_step_size=0.01):
    """The MEADS warm-up as ``(init, update)`` for callers that drive the loop themselves (``run`` below is this loop
    inside the engine, bit-equal to it)::

        init, update = meads.adaptation()
        meads_state, (step_size, scale, alpha, delta) = init(state)
        meads_state, (step_size, scale, alpha, delta) = update(meads_state, state.position, state.potential_energy_grad)
        for i in range(num_steps):
            info, _ = kernel(state, step_size, scale, alpha, delta)
            state = info.state
            meads_state, (step_size, scale, alpha, delta) = update(meads_state, state.position, state.potential_energy_grad)

    ``init`` returns the parameters before any update: ``initial_step_size``, scale 1, alpha 1, delta 0.5.  ``update`` is
    one ``aehmc_meads_update`` on COPIES of the state arrays -- states are values."""
    mult, slow, eps0 = _options(step_size_multiplier, damping_slowdown, initial_step_size)

    def init(initial_chain_state: GhmcState, num_chains=None):
        layout, _ = _layout(initial_chain_state.position, num_chains)
        _, D = _chains(layout)
        eng = get_engine()
        st = eng.meads_alloc(D, eps0)
        return _as_state(st, layout), _parameters(st)

    def update(meads_state: MeadsState, position, potential_energy_grad):
        eng = get_engine()
        if tuple(position.shape) != tuple(meads_state.position_shape):
            raise ValueError(f"position has shape {tuple(position.shape)}, the warm-up was initialised with "
                             f"{tuple(meads_state.position_shape)}")
        layout, _ = _layout(position, position.shape[0] if meads_state.batched else None)
        C, D = _chains(layout)
        st = {k: getattr(meads_state, k).clone() for k in ("params", "scale", "count", "skipped")}

        def rows(x):
            return _dev_f64(x, eng.device).reshape(C, D).contiguous()
        engine_call(eng.meads_update, C, D, rows(position), rows(potential_energy_grad), mult, slow, st)
        return _as_state(st, layout), _parameters(st)

    return init, update


def run(kernel, initial_state: GhmcState, num_steps=1000, *, step_size_multiplier=0.5, damping_slowdown=1.0,
        initial_step_size=0.01):
    """Warm a ``ghmc.new_kernel`` kernel up for ``num_steps`` transitions.  Returns ``(last_chain_state, (step_size, scale,
    alpha, delta), updates)``: Python floats and ``scale`` as a ``[D]`` device tensor, for ``kernel.sample``.

    ONE engine call (``aehmc_meads_warmup``): an update on the starting state, then per step one transition that reads
    the state's own parameters on the device and one update; nothing is read back between the steps.  Bit-equal to the
    hand-driven ``meads.adaptation`` loop.  A kernel that is not a generalised-HMC one and fewer than 2 chains raise
    ``ValueError``."""
    return _run(kernel, initial_state, num_steps, step_size_multiplier, damping_slowdown, initial_step_size)[:3]


def _run(kernel, initial_state, num_steps, step_size_multiplier, damping_slowdown, initial_step_size):
    """``run``, returning also the final ``MeadsState``."""
    k = _ghmc_settings(kernel)
    mult, slow, eps0 = _options(step_size_multiplier, damping_slowdown, initial_step_size)
    n = int(num_steps)
    if n < 0:
        raise ValueError("meads: num_steps must be >= 0")
    pos = initial_state.position
    layout, _ = _layout(pos, getattr(kernel, "num_chains", None) or None, getattr(kernel, "batched", pos.ndim == 2))
    C, D = _chains(layout)
    eng = get_engine()
    q, U, g = bind_target(k, eng, initial_state, layout, layout.scalar)
    st = eng.meads_alloc(D, eps0)
    rng, thr = k["holder"]["rng"], k["divergence_threshold"]
    momentum, slice_ = initial_state.momentum, getattr(initial_state, "slice", None)
    out = engine_call(eng.meads_warmup, rng, n, mult, slow, thr, q, U, g, st, momentum, slice_)
    if n == 0:  # (no transition ran: the state carries what it came with)
        state = GhmcState(layout.vec(q), momentum, layout.per_chain(U), layout.vec(g), slice_)
    else:
        state = state_of(layout, q, U, g, out)
    return state, _parameters(st), {k["srng"]: rng}, _as_state(st, layout)


def sample(kernel, state: GhmcState, step_size, scale, alpha, delta, num_samples: int, keep_samples: bool = True):
    """``kernel.sample(state, step_size, scale, alpha, delta, num_samples)``: one launch."""
    _ghmc_settings(kernel)
    return kernel.sample(state, step_size, scale, alpha, delta, num_samples, keep_samples)
