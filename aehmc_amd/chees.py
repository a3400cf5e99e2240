"""ChEES warm-up for static HMC: ONE trajectory length and ONE step size adapted from all chains together (Hoffman,
Radul, Sountsov, "An adaptive MCMC scheme for setting trajectory lengths in Hamiltonian Monte Carlo", AISTATS 2021).

``hmc.new_kernel`` takes ``num_integration_steps`` from the caller.  With many chains it can be adapted: ChEES maximises
the squared change of ``|q - E q|^2`` per unit of trajectory length, a cross-chain criterion that every warm-up step
estimates from all chains, and samples with jittered lengths ``L_i = ceil(halton(i) T / step_size)``.  The update is one
launch sequence of ``aehmc_chees_update`` (csrc/chees.cuh); the transitions are the package's HMC kernels, which read the
length of a transition from device memory, so ``run`` is one engine call and ``sample`` another: they
export the returned state and the accept flag rather than the proposal, and the accept flag weights the returned state
(``E[1{accept} f(proposal)] = E[alpha f(proposal)]``; on accept the returned momentum is the flipped end momentum).

The metric is held fixed.  The intended workflow adapts it first, pooled, at a provisional length::

    state, (eps0, imm), _ = window_adaptation.run(kernel, state, n, pooled=True, num_integration_steps=L0)
    state, (eps, imm, T), _ = chees.run(kernel, state, n, imm)
    samples, info, acc, div = chees.sample(kernel, state, eps, imm, T, num_samples)
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ._common import bind_target, diagnostics, histories
from .engine import PerChain, _dev_f64, get_engine
from .integrators import IntegratorState
from .step_size import DualAveragingState
from .window_adaptation import _layout


def halton(n: int) -> float:
    """The base-2 radical inverse of ``n >= 1``: 1/2, 1/4, 3/4, 1/8, 5/8, ... (exact in binary floating point)."""
    n = int(n)
    if n < 1:
        raise ValueError("halton(n) needs n >= 1")
    h, f = 0.0, 0.5
    while n:
        if n & 1:
            h += f
        n >>= 1
        f *= 0.5
    return h


def num_integration_steps(step_size: float, trajectory_length: float, index: int, jitter: bool = True) -> int:
    """``max(1, ceil(halton(index) T / step_size))``, the L of jittered transition ``index``; ``jitter=False``:
    ``max(1, ceil(T / step_size))``."""
    h = halton(index) if jitter else 1.0
    return max(1, math.ceil((h * float(trajectory_length)) / float(step_size)))


def trajectory_lengths(step_size: float, trajectory_length: float, num_samples: int, *, jitter: bool = True,
                       first: int = 1):
    """The lengths ``chees.sample`` runs: ``num_integration_steps(step_size, T, first + i, jitter)`` for ``i`` in
    ``range(num_samples)`` -- also what ``summary.run(..., num_integration_steps=...)`` takes for a jittered run that
    is summarised without being stored."""
    return [num_integration_steps(step_size, trajectory_length, int(first) + i, jitter) for i in range(int(num_samples))]


class CheesState(NamedTuple):
    """The adaptation state (device arrays; ``aehmc_chees_state``): every array [1] but ``step_size`` [C]."""
    step: torch.Tensor
    log_trajectory_length: torch.Tensor
    log_trajectory_length_avg: torch.Tensor
    adam_m: torch.Tensor
    adam_v: torch.Tensor
    halton_weight: torch.Tensor   # of the transition the next update will see
    num_steps: torch.Tensor       # L of that transition
    da_state: DualAveragingState
    step_size: torch.Tensor
    position_shape: Tuple = ()    # user-facing shape of the chain position and whether it has a leading chain axis
    batched: bool = False


_FIELDS = ("step", "log_T", "log_T_avg", "adam_m", "adam_v", "h", "num_steps")
_DA = ("da_step", "da_x", "da_x_avg", "da_g_avg", "da_mu")


def _as_state(st, layout) -> CheesState:
    return CheesState(*(st[n] for n in _FIELDS), DualAveragingState(*(st[n] for n in _DA)), st["step_size"],
                      layout.user_shape, bool(layout.scalar_chain_shape))


def _copied_arrays(state: CheesState) -> Dict:
    """The state's arrays by their ``aehmc_chees_state`` names, cloned: states are values."""
    st = dict(zip(_FIELDS, state[:len(_FIELDS)]))
    st.update(zip(_DA, state.da_state))
    st["step_size"] = state.step_size
    return {k: v.clone() for k, v in st.items()}


def _hmc_settings(kernel):
    k = getattr(kernel, "_hmc", None)
    if k is None:
        raise ValueError("chees works around a static HMC kernel (hmc.new_kernel); NUTS chooses its own trajectory lengths")
    return k


def _options(initial_step_size, initial_trajectory_length, target_acceptance_rate, learning_rate,
             max_num_integration_steps):
    eps0 = float(initial_step_size)
    T0 = eps0 if initial_trajectory_length is None else float(initial_trajectory_length)
    if not eps0 > 0 or not T0 > 0:
        raise ValueError("initial_step_size and initial_trajectory_length must be positive")
    if int(max_num_integration_steps) < 1:
        raise ValueError("max_num_integration_steps must be at least 1")
    return eps0, T0, float(target_acceptance_rate), float(learning_rate), int(max_num_integration_steps)


class _Metric:
    """A SHARED metric, held fixed, as ``aehmc_chees_update`` takes it: a scalar, a diagonal [D], or dense [D, D] (the
    caller's ``momentum . imm`` from the engine's GEMM with scalar 1)."""

    def __init__(self, inverse_mass_matrix):
        imm = inverse_mass_matrix
        if isinstance(imm, PerChain):
            raise ValueError("chees adapts ONE trajectory length and step size from all chains: the metric must be a "
                             "shared scalar, [D] or [D, D] value, not a PerChain one")
        ndim = imm.ndim if hasattr(imm, "ndim") else np.ndim(imm)
        if ndim > 2:
            raise ValueError(f"Expected a mass matrix of dimension 1 (diagonal) or 2, got {ndim}")
        self.value, self.ndim, self._dev = imm, ndim, None

    def velocity_args(self, eng, D, momentum):
        """``(momentum array, inverse_mass_diag, inverse_mass_scalar)`` of one update."""
        if self._dev is None:
            t = _dev_f64(self.value, eng.device)
            # (a scalar: read once per adaptation)
            self._dev = float(t) if self.ndim == 0 else t.reshape((D, D) if self.ndim == 2 else (D,)).contiguous()
        if isinstance(self._dev, float):
            return momentum, None, self._dev
        if self.ndim == 2:
            return eng.gemm_nt(momentum, self._dev), None, 1.0  # (imm is symmetric: momentum . imm^T)
        return momentum, self._dev, 0.0


def adaptation(num_steps: int, *, inverse_mass_matrix=1.0, initial_step_size=1.0, initial_trajectory_length=None,
               target_acceptance_rate=0.651, learning_rate=0.025, max_num_integration_steps=1000):
    """The ChEES warm-up as ``(init, update)`` for callers that drive the loop themselves, in the shapes of
    ``window_adaptation.window_adaptation`` (``run`` below is this loop on the engine's own arrays)::

        init, update = chees.adaptation(num_steps, inverse_mass_matrix=imm)
        chees_state, (step_size, L) = init(state)
        for i in range(num_steps):
            before = state.position
            info, _ = kernel(state, step_size, imm, L)
            state = info.state._replace(momentum=None)
            accepted = (state.position != before).reshape(C, -1).any(1)
            chees_state, (step_size, L) = update(i, chees_state, before, info, accepted)

    ``update`` is one launch sequence of ``aehmc_chees_update`` on COPIES of the state arrays -- states are values -- and
    returns the step size as ``PerChain([C])`` with all entries equal (it stays on the device) and the
    ``num_integration_steps`` of the next transition as a Python int: reading that one int64 back is the only host
    synchronisation of a step.  ``accepted``: the accept flag per chain; an accepted HMC proposal moves the chain, so
    "the position changed" is that flag.  After the last step the step size is the dual-averaging average and
    ``exp(chees_state.log_trajectory_length)`` the averaged trajectory length.

    ``initial_step_size`` starts dual averaging as ``window_adaptation`` does (the first step size is exp(0) = 1);
    the default initial trajectory length is the initial step size, so the first transition runs one leapfrog."""
    n_steps = int(num_steps)
    eps0, T0, target, lr, max_steps = _options(initial_step_size, initial_trajectory_length, target_acceptance_rate,
                                               learning_rate, max_num_integration_steps)
    metric = _Metric(inverse_mass_matrix)

    def init(initial_chain_state: IntegratorState, num_chains: Optional[int] = None):
        eng = get_engine()
        layout, _ = _layout(initial_chain_state.position, num_chains)
        st, cst = eng.chees_alloc(layout.C)
        eng.chees_init(layout.C, eps0, T0, cst)
        return _as_state(st, layout), (PerChain(st["step_size"]), min(int(st["num_steps"]), max_steps))

    def update(step: int, chees_state: CheesState, position_before, info, accepted):
        eng = get_engine()
        position = info.state.position
        if tuple(position.shape) != tuple(chees_state.position_shape):
            raise ValueError(f"position has shape {tuple(position.shape)}, the warm-up was initialised with "
                             f"{tuple(chees_state.position_shape)}")
        C = chees_state.step_size.numel()
        layout, _ = _layout(position, C if chees_state.batched else None)
        D = layout.D
        st = _copied_arrays(chees_state)

        def rows(x):
            return _dev_f64(x, eng.device).reshape(C, D).contiguous()
        mom, diag, scalar = metric.velocity_args(eng, D, rows(info.state.momentum))
        flag = torch.as_tensor(accepted, device=eng.device).reshape(C).to(torch.int32).contiguous()
        eng.chees_update(C, D, int(step) == n_steps - 1, target, lr, max_steps, rows(position_before), rows(position), mom,
                         diag, scalar, flag, _dev_f64(info.acceptance_probability, eng.device).reshape(C).contiguous(),
                         eng.chees_cstate(st))
        return _as_state(st, layout), (PerChain(st["step_size"]), int(st["num_steps"]))

    return init, update


def run(kernel, initial_state: IntegratorState, num_steps=1000, inverse_mass_matrix=1.0, *, initial_step_size=1.0,
        initial_trajectory_length=None, target_acceptance_rate=0.651, learning_rate=0.025,
        max_num_integration_steps=1000):
    """Warm an ``hmc.new_kernel`` kernel up for ``num_steps`` transitions, adapting the trajectory length and the step
    size from all chains.  Returns ``(last_chain_state, (step_size, inverse_mass_matrix, trajectory_length), updates)``
    with ``step_size`` and ``trajectory_length`` as Python floats, for ``chees.sample``.

    ``inverse_mass_matrix`` is a SHARED scalar, ``[D]`` or ``[D, D]`` value and is held fixed -- adapt it first with
    ``window_adaptation.run(kernel, state, n, pooled=True, num_integration_steps=L0)``; a ``PerChain`` metric and any
    kernel but a static HMC one raise ``ValueError``.

    ONE engine call (``aehmc_chees_warmup``): per step the position is copied, the transition runs on whatever route
    ``aehmc_hmc_step`` picks for the target with the step sizes bound to the adaptation state's ``[C]`` array, and the
    update rewrites that array and ``num_steps`` in place.  On the routes whose kernels read the trajectory length from
    device memory the transition takes ``num_steps`` from the state itself and the host waits for
    nothing between the steps; on the others the engine reads the one int64 back per step.  Bit-equal to the
    hand-driven ``chees.adaptation`` loop either way."""
    return _run(kernel, initial_state, num_steps, inverse_mass_matrix, initial_step_size, initial_trajectory_length,
                target_acceptance_rate, learning_rate, max_num_integration_steps)[:3]


def _run(kernel, initial_state, num_steps, inverse_mass_matrix, initial_step_size, initial_trajectory_length,
         target_acceptance_rate, learning_rate, max_num_integration_steps):
    """``run``, returning also the final ``CheesState`` and the engine's record of the last transition (a dict with
    ``n_leapfrog`` [C], ``acceptance_probability`` [C], ...; None for ``num_steps`` = 0)."""
    k = _hmc_settings(kernel)
    metric = _Metric(inverse_mass_matrix)
    eps0, T0, target, lr, max_steps = _options(initial_step_size, initial_trajectory_length, target_acceptance_rate,
                                               learning_rate, max_num_integration_steps)
    n = int(num_steps)
    eng = get_engine()
    pos = initial_state.position
    layout, _ = _layout(pos, getattr(kernel, "num_chains", None) or None, getattr(kernel, "batched", pos.ndim == 2))
    C, D = layout.C, layout.D
    st, cst = eng.chees_alloc(C)
    eng.chees_init(C, eps0, T0, cst)
    q, U, g = bind_target(k, eng, initial_state, layout, layout.scalar)
    eng.set_metric(inverse_mass_matrix, D)
    rng, thr = k["holder"]["rng"], k["divergence_threshold"]
    # (a scalar metric: the update takes its value from the host, as chees.adaptation's does)
    scalar = float(_dev_f64(inverse_mass_matrix, eng.device)) if metric.ndim == 0 else 0.0
    out = eng.chees_warmup(rng, n, target, lr, max_steps, scalar, thr, q, U, g, st, cst) if n > 0 else None
    state = IntegratorState(position=layout.vec(q), momentum=None, potential_energy=layout.per_chain(U),
                            potential_energy_grad=layout.vec(g))
    step_size, T = float(st["step_size"][0]), math.exp(float(st["log_T"]))
    return state, (step_size, inverse_mass_matrix, T), {k["srng"]: rng}, _as_state(st, layout), out


def sample(kernel, state: IntegratorState, step_size, inverse_mass_matrix, trajectory_length, num_samples: int, *,
           keep_samples: bool = True, jitter: bool = True, first: int = 1):
    """``num_samples`` transitions of a static HMC kernel with jittered lengths: transition ``i`` (from 0) runs
    ``L_i = max(1, ceil(halton(first + i) T / step_size))`` leapfrogs; ``jitter=False`` runs ``ceil(T / step_size)``
    every time.  Returns what ``kernel.sample`` returns: ``(samples [N, ...], Diagnostics of the last transition,
    acceptance history [N, ...], divergence history [N, ...])``.

    ONE engine call (``aehmc_hmc_sample_lengths``) with the lengths, which the host knows (``step_size`` and
    ``trajectory_length`` are host floats): one launch on the routes whose kernels read them from device memory, a loop
    of single transitions inside the engine on the others.  ``first``: continue a Halton sequence across calls
    (``first = 1 + draws so far``)."""
    k = _hmc_settings(kernel)
    _Metric(inverse_mass_matrix)  # (a PerChain metric has no ONE trajectory length to go with)
    if isinstance(step_size, PerChain):
        raise ValueError("chees.sample takes the ONE step size of chees.run, not PerChain step sizes")
    eps, T, n = float(step_size), float(trajectory_length), int(num_samples)
    if not eps > 0 or not T > 0 or n < 1 or int(first) < 1:
        raise ValueError("chees.sample needs step_size > 0, trajectory_length > 0, num_samples >= 1 and first >= 1")
    lengths = trajectory_lengths(eps, T, n, jitter=jitter, first=first)
    eng = get_engine()
    pos = state.position
    layout, _ = _layout(pos, getattr(kernel, "num_chains", None) or None, getattr(kernel, "batched", pos.ndim == 2))
    C, D = layout.C, layout.D
    q, U, g = bind_target(k, eng, state, layout, layout.scalar)
    eng.set_metric(inverse_mass_matrix, D)
    rng, thr = k["holder"]["rng"], k["divergence_threshold"]
    out = eng.hmc_sample_lengths(rng, eng.set_step_sizes(eps), lengths, thr, q, U, g, keep_samples)
    out["n_leapfrog"].fill_(lengths[-1])  # (documented: of the last transition; the engine reports the call's total)
    samples, acc_hist, div_hist = histories(layout, out, n, keep_samples)
    return samples, diagnostics(layout, q, U, g, out, False), acc_hist, div_hist
