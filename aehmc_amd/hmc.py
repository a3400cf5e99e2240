"""HMC kernel -- thin wrapper over the HIP engine (reference: aehmc/hmc.py)."""
from __future__ import annotations

from typing import Callable, Dict, Tuple

from ._common import diagnostics, histories, make_kernel, new_state as _new_state, trajectory_lengths
from .integrators import IntegratorState
from .random import RandomStream
from .trajectory import Diagnostics

new_state = _new_state


def new_kernel(srng: RandomStream, logprob_fn, divergence_threshold: int = 1000) -> Callable:
    """Build a HMC kernel (reference: aehmc/hmc.py:43-126).

    Same arguments as the reference; ``logprob_fn`` is a ``targets.Target`` or, as in the reference, a Python function of the position (traced once: ``targets.from_callable``).  The two RNG
    call sites of the reference graph (momentum hmc.py:122, accept hmc.py:194) are taken
    from ``srng`` here, in that order."""
    thr = float(divergence_threshold)
    holder, bind, finish = make_kernel(srng, logprob_fn, nuts=False, n_sites=2, settings=dict(divergence_threshold=thr))

    def step(state: IntegratorState, step_size, inverse_mass_matrix,
             num_integration_steps: int) -> Tuple[Diagnostics, Dict]:
        """One HMC transition for every chain (reference: aehmc/hmc.py:77-124)."""
        eng, layout, q, U, g = bind(state, inverse_mass_matrix)
        out = eng.hmc_step(holder["rng"], eng.set_step_sizes(step_size), int(num_integration_steps), thr, q, U, g)
        return diagnostics(layout, q, U, g, out, False), {srng: holder["rng"]}

    def sample(state: IntegratorState, step_size, inverse_mass_matrix, num_integration_steps,
               num_samples: int, keep_samples: bool = True, into=None):
        """``num_samples`` consecutive transitions per chain in one engine call -- the
        user-level ``aesara.scan(kernel, n_steps=N)`` loop of the reference
        (tests/test_hmc.py:138-148).  Returns ``(samples [N, ...], Diagnostics of the last
        transition, acceptance history [N, ...], divergence history [N, ...])``.  ``into``: a device buffer the draws
        are written to instead of a fresh one (``samples`` is then a view of it).

        ``num_integration_steps``: an int, or one length per transition -- a sequence, numpy array or integer tensor of
        ``num_samples`` entries >= 0 (randomised-length HMC): still one engine call, bit-equal to the loop of single
        transitions ``kernel(state, step_size, imm, L_i)``; ``Diagnostics.n_leapfrog`` is then the sum of the lengths."""
        lengths = trajectory_lengths(num_integration_steps, num_samples)
        eng, layout, q, U, g = bind(state, inverse_mass_matrix)
        if lengths is None:
            out = eng.hmc_sample(holder["rng"], eng.set_step_sizes(step_size), int(num_integration_steps), thr,
                                 int(num_samples), q, U, g, keep_samples, into)
        else:
            out = eng.hmc_sample_lengths(holder["rng"], eng.set_step_sizes(step_size), lengths, thr, q, U, g,
                                         keep_samples, into)
        info = diagnostics(layout, q, U, g, out, False)
        samples, acc_hist, div_hist = histories(layout, out, int(num_samples), keep_samples)
        return samples, info, acc_hist, div_hist

    return finish(step, sample)
