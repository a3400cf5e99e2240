"""NUTS kernel -- thin wrapper over the HIP engine (reference: aehmc/nuts.py)."""
from __future__ import annotations

from typing import Callable, Dict, Tuple

from ._common import diagnostics, histories, make_kernel, new_state as _new_state
from .integrators import IntegratorState
from .random import RandomStream
from .trajectory import Diagnostics

new_state = _new_state  # reference: aehmc/nuts.py:14


def new_kernel(srng: RandomStream, logprob_fn, max_num_expansions: int = 10,
               divergence_threshold: int = 1000) -> Callable:
    """Build an iterative NUTS kernel (reference: aehmc/nuts.py:17-155).

    RNG call sites, in the reference's graph-construction order: momentum (nuts.py:113),
    direction (trajectory.py:516), uniform progressive sampling (proposals.py:99), biased
    progressive sampling (proposals.py:131)."""
    max_exp, thr = int(max_num_expansions), float(divergence_threshold)
    holder, bind, finish = make_kernel(srng, logprob_fn, nuts=True, n_sites=4,
                                       settings=dict(max_num_expansions=max_exp, divergence_threshold=thr))

    def step(state: IntegratorState, step_size, inverse_mass_matrix) -> Tuple[Diagnostics, Dict]:
        """One NUTS transition for every chain (reference: aehmc/nuts.py:56-153)."""
        eng, layout, q, U, g = bind(state, inverse_mass_matrix)
        out = eng.nuts_step(holder["rng"], eng.set_step_sizes(step_size), max_exp, thr, q, U, g)
        return diagnostics(layout, q, U, g, out, True), {srng: holder["rng"]}

    def sample(state: IntegratorState, step_size, inverse_mass_matrix, num_samples: int,
               keep_samples: bool = True, into=None):
        """``num_samples`` consecutive transitions per chain in one engine call (the
        reference's user-level ``aesara.scan(kernel, n_steps=N)``, tests/test_hmc.py:296-324).
        Returns ``(samples [N, ...], Diagnostics of the last transition with the leapfrog
        TOTAL in n_leapfrog, acceptance history, divergence history)``.  ``into``: a device buffer the
        draws are written to instead of a fresh one (``samples`` is then a view of it)."""
        eng, layout, q, U, g = bind(state, inverse_mass_matrix)
        out = eng.nuts_sample(holder["rng"], eng.set_step_sizes(step_size), max_exp, thr, int(num_samples), q, U, g,
                              keep_samples, into)
        info = diagnostics(layout, q, U, g, out, True)
        samples, acc_hist, div_hist = histories(layout, out, int(num_samples), keep_samples)
        return samples, info, acc_hist, div_hist

    return finish(step, sample)
