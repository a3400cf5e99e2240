"""Stan-style window adaptation of the step size and the inverse mass matrix (diagonal, or
dense per chain with ``is_mass_matrix_full``), one adaptation per chain (reference: aehmc/window_adaptation.py, step_size.py,
mass_matrix.py, algorithms.py).  The schedule is host logic; the per-chain dual-averaging /
Welford updates run in one HIP kernel per warm-up step (`aehmc_adapt_update`).

``pooled=True`` adapts ONE step size and ONE inverse mass matrix from all chains together (`aehmc_pooled_adapt_update`:
the mean acceptance probability into dual averaging, a batch Welford update per warm-up step) and returns plain shared
values, which the kernels take on their shared-metric routes."""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from ._common import Layout, bind_target, diagnostics
from .engine import PerChain, _dev_f64, get_engine
from .integrators import IntegratorState
from .step_size import DualAveragingState


def build_schedule(num_steps: int, initial_buffer_size: int = 75, final_buffer_size: int = 50,
                   first_window_size: int = 25) -> List[Tuple[int, bool]]:
    """(window_label, is_middle_window_end) per warm-up step (reference:
    aehmc/window_adaptation.py:230-327): a fast initial buffer, slow windows doubling in
    size with no memory, a fast final buffer; labels 0 = fast, 1 = slow."""
    if num_steps < 20:  # too short for mass-matrix adaptation
        return [(0, False)] * num_steps
    if initial_buffer_size + first_window_size + final_buffer_size > num_steps:
        initial_buffer_size = int(0.15 * num_steps)
        final_buffer_size = int(0.1 * num_steps)
        first_window_size = num_steps - initial_buffer_size - final_buffer_size
    slow_end = num_steps - final_buffer_size
    labels = [(0, False)] * initial_buffer_size
    start, size = initial_buffer_size, first_window_size
    while start < slow_end:
        if 3 * size <= slow_end - start:
            this, size = size, 2 * size
        else:
            this = slow_end - start
        labels += [(1, False)] * (this - 1) + [(1, True)]
        start += this
    return labels + [(0, False)] * (num_steps - slow_end)


def _layout(position, num_chains=None, batched=None):
    """``(Layout, the chain position is a scalar)`` of a position; without ``batched`` a leading chain axis is read off
    ``num_chains`` being given or the position being 2-D."""
    shape = tuple(position.shape)
    if batched is None:
        batched = num_chains is not None or len(shape) == 2
    layout = Layout(shape, batched, num_chains if num_chains is not None else (shape[0] if batched else 1))
    return layout, layout.scalar


class _Adaptation(NamedTuple):
    """The engine calls of an adaptation: one state per chain, or the pooled one."""
    alloc: Callable
    init: Callable
    update: Callable
    cstate: Callable


def _adaptation(eng, pooled) -> _Adaptation:
    if pooled:
        return _Adaptation(eng.pooled_adapt_alloc, eng.pooled_adapt_init, eng.pooled_adapt_update, eng.pooled_cstate)
    return _Adaptation(eng.adapt_alloc, eng.adapt_init, eng.adapt_update, eng.adapt_cstate)


def _start(eng, pooled, layout, full, initial_step_size):
    """A fresh adaptation state ``(arrays, C struct)``: identity metric, dual averaging started at ``initial_step_size``."""
    ad = _adaptation(eng, pooled)
    st, cst = ad.alloc(layout.C, layout.D, full)
    ad.init(layout.C, layout.D, float(initial_step_size), cst)
    return st, cst


def _params(pooled, layout, scalar_position, st):
    """The state's arrays as the kernel's ``(step_size, inverse_mass_matrix)``: ``PerChain`` values, or pooled the step
    size as ``PerChain([C])`` with all entries equal and the shared metric as a plain tensor."""
    if pooled:
        return PerChain(st["step_size"]), (st["imm"].reshape(()) if scalar_position else st["imm"])
    return (PerChain(layout.per_chain(st["step_size"])),
            PerChain(st["imm"].reshape(layout.C) if scalar_position else st["imm"], st["sqrt_mass"]))


def run(kernel, initial_state: IntegratorState, num_steps=1000, *, is_mass_matrix_full=False,
        initial_step_size=1.0, target_acceptance_rate=0.80, fused=True, num_integration_steps=None,
        pooled=False) -> Tuple[IntegratorState, Tuple, Dict]:
    """Warm a kernel up for ``num_steps`` transitions (reference:
    aehmc/window_adaptation.py:17-116).  Returns ``(last_chain_state, (step_size,
    inverse_mass_matrix), updates)`` where the parameters are ``PerChain`` values -- one
    step size and one (diagonal or dense) inverse mass matrix per chain, exactly as running the
    reference once per chain would produce -- to be passed back to ``kernel``.

    With a NUTS or HMC kernel of this package the whole loop runs inside one C-ABI call
    (``aehmc_nuts_warmup`` / ``aehmc_hmc_warmup``: transition, adaptation update, transition, ... enqueued back to back);
    ``fused=False`` -- and any other kernel -- takes the step-by-step loop below, which issues the
    same kernels in the same order (identical results).

    An HMC kernel (``hmc.new_kernel``) takes a fourth argument; pass its fixed trajectory length as
    ``num_integration_steps`` and the loop calls ``kernel(state, step_size, imm, num_integration_steps)``
    (the reference's loop calls ``kernel(chain_state, *parameters)``, window_adaptation.py:66, so there an
    HMC kernel has to be wrapped in a lambda that closes over the length -- which works here too).

    ``pooled=True``: one adaptation from all chains together instead of one per chain.  The parameters are then a
    Python ``float`` (one read-back after the loop) and a plain device tensor ``[D]`` / ``[D, D]`` (0-d for a scalar
    position) -- shared values, so ``kernel(state, step_size, imm)`` and ``kernel.sample`` run the shared-metric kernels.
    There is no limit on D of its own."""
    if getattr(kernel, "_hmc", None) is not None and num_integration_steps is None:
        raise ValueError("window_adaptation.run with an HMC kernel needs num_integration_steps")
    extra = () if num_integration_steps is None else (int(num_integration_steps),)
    eng = get_engine()
    target = float(target_acceptance_rate)
    pos = initial_state.position
    layout, scalar_position = _layout(pos, getattr(kernel, "num_chains", None) or None,
                                      getattr(kernel, "batched", pos.ndim == 2))
    C, D = layout.C, layout.D
    full = bool(is_mass_matrix_full) and not scalar_position  # mass_matrix.py:54-57: a scalar stays a scalar
    if full and not pooled and D > 2048:  # one wavefront factors each chain's matrix (tests: up to D = 1024)
        raise ValueError("is_mass_matrix_full keeps one dense D x D matrix per chain (as the reference does) and "
                         "is supported up to D = 2048")
    st, cst = _start(eng, pooled, layout, full, initial_step_size)
    schedule = build_schedule(int(num_steps))
    # The transitions read the state's own arrays, which the update kernels rewrite in place -- pooled: the step size from
    # all C entries of ``step_size``, so that no value returns to the host between steps, the metric as a SHARED one
    # (one object: Engine.set_metric keys it by identity).  One ``PerChain`` pair serves every step of the per-chain loop
    # too: with ``sqrt_mass`` handed over the engine keeps nothing by the object's identity, it binds the arrays each call.
    eps = PerChain(st["step_size"])
    _, imm = _params(pooled, layout, scalar_position, st)
    nk = getattr(kernel, "_nuts", None)
    k = nk if nk is not None else getattr(kernel, "_hmc", None)
    if fused and k is not None and len(schedule) > 0:
        # (no ``scalar`` for set_target here: a Python function not yet traced is read as the kernels' own calls leave it)
        q, U, g = bind_target(k, eng, initial_state, layout, None)
        out = eng._warmup(nk is not None, pooled, k["holder"]["rng"], schedule, target,
                          nk["max_num_expansions"] if nk is not None else extra[0], k["divergence_threshold"],
                          q, U, g, st, cst, imm)
        info = diagnostics(layout, q, U, g, out, nk is not None)
        state, updates = info.state._replace(momentum=None), {k["srng"]: k["holder"]["rng"]}
    else:
        state, updates = initial_state, {}
        update = _adaptation(eng, pooled).update
        try:
            # pooled: the metric is bound here, and again after a window end (``force``: a kernel's in-place rewrite does
            # not move ``_version``)
            if pooled:
                eng.set_metric(imm, D, force=True, sqrt_mass=st["sqrt_mass"])
            for i, (stage, window_end) in enumerate(schedule):
                info, updates = kernel(state, eps, imm, *extra)
                state = info.state._replace(momentum=None)
                update(C, D, stage, window_end, i == len(schedule) - 1, target,
                       _dev_f64(info.acceptance_probability, eng.device).reshape(C).contiguous(),
                       _dev_f64(state.position, eng.device).reshape(C, D).contiguous(), cst)
                if pooled and window_end:
                    eng.set_metric(imm, D, force=True, sqrt_mass=st["sqrt_mass"])
        finally:
            if pooled:
                eng.forget_metric()
    if pooled:
        step_size = float(st["step_size"][0])  # the one read-back
        imm = st["imm"].clone()
        return state, (step_size, imm.reshape(()) if scalar_position else imm), updates
    return state, _params(False, layout, scalar_position,
                          {name: st[name].clone() for name in ("step_size", "imm", "sqrt_mass")}), updates


class WarmupState(NamedTuple):
    """window_adaptation.py:119-227's ``warmup_state = (da_state, mm_state)`` (DualAveragingState,
    algorithms.py:9-14; Welford state ``(mean, m2, sample_size)``, algorithms.py:141-165) plus the current
    parameters' device arrays the update kernel rewrites (step size, inverse mass matrix, its square root)."""
    da_state: DualAveragingState
    mm_state: Tuple
    step_size: torch.Tensor
    imm: torch.Tensor
    sqrt_mass: torch.Tensor
    work: Optional[torch.Tensor] = None
    position_shape: Tuple = ()   # user-facing shape of the chain position and whether it has a leading chain axis
    batched: bool = False


_FIELDS = ("da_step", "da_x", "da_x_avg", "da_g_avg", "da_mu", "wc_mean", "wc_m2", "wc_n", "step_size", "imm", "sqrt_mass")


def _warmup_state(pooled, layout, scalar_position, st):
    """``(WarmupState, parameters)`` over the arrays ``st`` of an adaptation state."""
    ws = WarmupState(DualAveragingState(*(st[name] for name in _FIELDS[:5])), tuple(st[name] for name in _FIELDS[5:8]),
                     st["step_size"], st["imm"], st["sqrt_mass"], st.get("work"), layout.user_shape,
                     bool(layout.scalar_chain_shape))
    return ws, _params(pooled, layout, scalar_position, st)


def window_adaptation(num_steps: int, is_mass_matrix_full: bool = False, initial_step_size=1.0,
                      target_acceptance_rate=0.80, pooled=False):
    """The warm-up as ``(init, update)`` for callers that drive the loop themselves (reference:
    aehmc/window_adaptation.py:119-227 -- ``run`` above is that loop in one engine call):

        init, update = window_adaptation(num_steps)
        warmup_state, parameters = init(state)              # parameters = (step_size, inverse_mass_matrix)
        for i in range(num_steps):
            info, _ = kernel(state, *parameters)
            state = info.state._replace(momentum=None)
            warmup_state, parameters = update(i, warmup_state, parameters, info)

    ``update`` is one launch of the warm-up kernel (``aehmc_adapt_update``: dual averaging in every stage, Welford in
    the slow windows, new metric + restart at a window end, the averaged step size after the last step) on COPIES of
    the state arrays -- states are values, as in the reference; the parameters are ``PerChain`` values (one
    adaptation per chain).

    ``pooled=True``: the pair of the pooled adaptation (one launch sequence of ``aehmc_pooled_adapt_update`` per
    ``update``).  The warm-up state then holds ONE dual-averaging and Welford state; the parameters are the step size
    as ``PerChain([C])`` with all entries equal (it stays on the device; ``float(p.value[0])`` reads it) and the shared
    inverse mass matrix as a plain tensor."""
    schedule = build_schedule(int(num_steps))
    target = float(target_acceptance_rate)

    def init(initial_chain_state: IntegratorState, num_chains: Optional[int] = None):
        """window_adaptation.py:130-143: identity metric, dual averaging started at ``initial_step_size`` (so the
        first step size is exp(0) = 1, algorithms.py:56-76)."""
        layout, scalar_position = _layout(initial_chain_state.position, num_chains)
        st, _ = _start(get_engine(), pooled, layout, bool(is_mass_matrix_full) and not scalar_position, initial_step_size)
        return _warmup_state(pooled, layout, scalar_position, st)

    def update(step: int, warmup_state: WarmupState, parameters, chain_state):
        """window_adaptation.py:192-214 for warm-up step ``step`` (0-based) after the transition ``chain_state``."""
        del parameters  # (the arrays in warmup_state ARE the current parameters)
        eng = get_engine()
        position = chain_state.state.position
        C = warmup_state.step_size.numel()
        if tuple(position.shape) != tuple(warmup_state.position_shape):
            raise ValueError(f"position has shape {tuple(position.shape)}, the warm-up was initialised with "
                             f"{tuple(warmup_state.position_shape)}")
        layout, scalar_position = _layout(position, C if warmup_state.batched else None)
        full = warmup_state.imm.ndim == (2 if pooled else 3)
        da, mm = warmup_state.da_state, warmup_state.mm_state
        old = zip(_FIELDS, (*da, *mm, warmup_state.step_size, warmup_state.imm, warmup_state.sqrt_mass))
        st = {name: t.clone() for name, t in old}  # states are values
        if warmup_state.work is not None:  # (scratch of the window-end factorisation, not state)
            st["work"] = warmup_state.work
        stage, window_end = schedule[int(step)]
        ad = _adaptation(eng, pooled)
        ad.update(C, layout.D, stage, window_end, int(step) == len(schedule) - 1, target,
                  _dev_f64(chain_state.acceptance_probability, eng.device).reshape(C).contiguous(),
                  _dev_f64(position, eng.device).reshape(C, layout.D).contiguous(), ad.cstate(st, full))
        return _warmup_state(pooled, layout, scalar_position, st)

    return init, update
