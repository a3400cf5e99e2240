"""Stan-style window adaptation of the step size and the inverse mass matrix (diagonal, or
dense per chain with ``is_mass_matrix_full``), one adaptation per chain (reference: aehmc/window_adaptation.py, step_size.py,
mass_matrix.py, algorithms.py).  The schedule is host logic; the per-chain dual-averaging /
Welford updates run in one HIP kernel per warm-up step (`aehmc_adapt_update`).

``pooled=True`` adapts ONE step size and ONE inverse mass matrix from all chains together (`aehmc_pooled_adapt_update`:
the mean acceptance probability into dual averaging, a batch Welford update per warm-up step) and returns plain shared
values, which the kernels take on their shared-metric routes."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from ._common import Layout
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
    if pooled:
        return _run_pooled(eng, kernel, initial_state, int(num_steps), bool(is_mass_matrix_full),
                           float(initial_step_size), float(target_acceptance_rate), bool(fused), extra)
    pos = initial_state.position
    srng_chains = getattr(kernel, "num_chains", None)
    batched = getattr(kernel, "batched", pos.ndim == 2)
    layout = Layout(tuple(pos.shape), batched, srng_chains or (pos.shape[0] if batched else 1))
    C, D = layout.C, layout.D
    scalar_position = (len(layout.user_shape) - (1 if batched else 0)) == 0
    full = bool(is_mass_matrix_full) and not scalar_position  # mass_matrix.py:54-57: a scalar stays a scalar
    if full and D > 2048:  # one wavefront factors each chain's matrix (tests: up to D = 1024)
        raise ValueError("is_mass_matrix_full keeps one dense D x D matrix per chain (as the reference does) and "
                         "is supported up to D = 2048")
    st, cst = eng.adapt_alloc(C, D, full)
    eng.adapt_init(C, D, float(initial_step_size), cst)
    schedule = build_schedule(int(num_steps))

    def imm_param():
        return PerChain(st["imm"].reshape(C) if scalar_position else st["imm"], st["sqrt_mass"])

    nk = getattr(kernel, "_nuts", None)
    if fused and nk is not None and len(schedule) > 0:
        from ._common import diagnostics, state_rows
        from .engine import rng_to_device
        if "rng" not in nk["holder"] or nk["holder"]["rng"].device != eng.device:  # (uploaded at construction, maybe elsewhere)
            nk["holder"]["rng"] = (nk["holder"]["rng"].to(eng.device) if "rng" in nk["holder"]
                                   else rng_to_device(nk["rng_host"], eng.device))
        q, U, g = state_rows(initial_state, layout, eng.device)
        eng.set_target(nk["logprob_fn"], D)
        out = eng.nuts_warmup(nk["holder"]["rng"], schedule, float(target_acceptance_rate),
                              nk["max_num_expansions"], nk["divergence_threshold"], q, U, g, st, cst, imm_param())
        info = diagnostics(layout, q, U, g, out, True)
        state, updates = info.state._replace(momentum=None), {nk["srng"]: nk["holder"]["rng"]}
        schedule = []
    elif fused and getattr(kernel, "_hmc", None) is not None and len(schedule) > 0:
        from ._common import diagnostics, state_rows
        from .engine import rng_to_device
        hk = kernel._hmc
        if "rng" not in hk["holder"] or hk["holder"]["rng"].device != eng.device:
            hk["holder"]["rng"] = (hk["holder"]["rng"].to(eng.device) if "rng" in hk["holder"]
                                   else rng_to_device(hk["rng_host"], eng.device))
        q, U, g = state_rows(initial_state, layout, eng.device)
        eng.set_target(hk["logprob_fn"], D)
        out = eng.hmc_warmup(hk["holder"]["rng"], schedule, float(target_acceptance_rate), extra[0],
                             hk["divergence_threshold"], q, U, g, st, cst, imm_param())
        info = diagnostics(layout, q, U, g, out, False)
        state, updates = info.state._replace(momentum=None), {hk["srng"]: hk["holder"]["rng"]}
        schedule = []
    else:
        state, updates = initial_state, {}
    for i, (stage, window_end) in enumerate(schedule):
        info, updates = kernel(state, PerChain(st["step_size"]), imm_param(), *extra)
        state = info.state._replace(momentum=None)
        eng.adapt_update(C, D, stage, window_end, i == len(schedule) - 1, float(target_acceptance_rate),
                         info.acceptance_probability.reshape(C).contiguous(),
                         state.position.reshape(C, D).contiguous(), cst)
    step_size = st["step_size"].clone()
    imm, sqrt_mass = st["imm"].clone(), st["sqrt_mass"].clone()
    return state, (PerChain(layout.per_chain(step_size)),
                   PerChain(imm.reshape(C) if scalar_position else imm, sqrt_mass)), updates


def _run_pooled(eng, kernel, initial_state, num_steps, is_mass_matrix_full, initial_step_size, target, fused, extra):
    """``run(..., pooled=True)``: the loop of ``run`` around ONE adaptation state (Engine.pooled_adapt_alloc).  The
    transitions read the state's own arrays -- the step size from all C entries of ``step_size``, bound as per-chain
    step sizes so that no value returns to the host between steps, the metric as a SHARED one -- and after a window end
    the metric is bound again (``force=True``: a kernel's in-place rewrite does not move ``_version``)."""
    pos = initial_state.position
    srng_chains = getattr(kernel, "num_chains", None)
    batched = getattr(kernel, "batched", pos.ndim == 2)
    layout = Layout(tuple(pos.shape), batched, srng_chains or (pos.shape[0] if batched else 1))
    C, D = layout.C, layout.D
    scalar_position = (len(layout.user_shape) - (1 if batched else 0)) == 0
    full = is_mass_matrix_full and not scalar_position  # mass_matrix.py:54-57: a scalar stays a scalar
    st, cst = eng.pooled_adapt_alloc(C, D, full)
    eng.pooled_adapt_init(C, D, initial_step_size, cst)
    schedule = build_schedule(num_steps)
    imm = st["imm"].reshape(()) if scalar_position else st["imm"]  # (one object: Engine.set_metric keys it by identity)
    nk, hk = getattr(kernel, "_nuts", None), getattr(kernel, "_hmc", None)
    k = nk if nk is not None else hk
    if fused and k is not None and len(schedule) > 0:
        from ._common import diagnostics, state_rows
        from .engine import rng_to_device
        if "rng" not in k["holder"] or k["holder"]["rng"].device != eng.device:
            k["holder"]["rng"] = (k["holder"]["rng"].to(eng.device) if "rng" in k["holder"]
                                  else rng_to_device(k["rng_host"], eng.device))
        q, U, g = state_rows(initial_state, layout, eng.device)
        eng.set_target(k["logprob_fn"], D)
        out = eng.warmup_pooled(nk is not None, k["holder"]["rng"], schedule, target,
                                nk["max_num_expansions"] if nk is not None else extra[0], k["divergence_threshold"],
                                q, U, g, st, cst, imm)
        info = diagnostics(layout, q, U, g, out, nk is not None)
        state, updates = info.state._replace(momentum=None), {k["srng"]: k["holder"]["rng"]}
    else:
        state, updates = initial_state, {}
        try:
            eng.set_metric(imm, D, force=True, sqrt_mass=st["sqrt_mass"])
            for i, (stage, window_end) in enumerate(schedule):
                info, updates = kernel(state, PerChain(st["step_size"]), imm, *extra)
                state = info.state._replace(momentum=None)
                eng.pooled_adapt_update(C, D, stage, window_end, i == len(schedule) - 1, target,
                                        _dev_f64(info.acceptance_probability, eng.device).reshape(C).contiguous(),
                                        _dev_f64(state.position, eng.device).reshape(C, D).contiguous(), cst)
                if window_end:
                    eng.set_metric(imm, D, force=True, sqrt_mass=st["sqrt_mass"])
        finally:
            eng.forget_metric()
    step_size = float(st["step_size"][0])  # the one read-back
    out_imm = st["imm"].clone()
    return state, (step_size, out_imm.reshape(()) if scalar_position else out_imm), updates


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
    if pooled:
        return _pooled_pair(schedule, bool(is_mass_matrix_full), float(initial_step_size),
                            float(target_acceptance_rate))

    def _layout(position, num_chains):
        shape = tuple(position.shape)
        batched = num_chains is not None or len(shape) == 2
        C = (num_chains if num_chains is not None else shape[0]) if batched else 1
        layout = Layout(shape, batched, C)
        scalar_position = (len(shape) - (1 if batched else 0)) == 0
        return layout, scalar_position

    def _params(layout, scalar_position, ws: WarmupState):
        C = layout.C
        return (PerChain(layout.per_chain(ws.step_size)),
                PerChain(ws.imm.reshape(C) if scalar_position else ws.imm, ws.sqrt_mass))

    def _cstate(eng, ws: WarmupState, full):
        from . import _lib
        da, (mean, m2, n) = ws.da_state, ws.mm_state
        ptr = dict(da_step=da.step, da_x=da.iterates, da_x_avg=da.iterates_avg, da_g_avg=da.gradient_avg,
                   da_mu=da.shrinkage_pts, wc_mean=mean, wc_m2=m2, wc_n=n, step_size=ws.step_size, imm=ws.imm,
                   sqrt_mass=ws.sqrt_mass)
        if ws.work is not None:
            ptr["work"] = ws.work
        return _lib.CAdaptState(full=int(bool(full)), **{k: v.data_ptr() for k, v in ptr.items()})

    def init(initial_chain_state: IntegratorState, num_chains: Optional[int] = None):
        """window_adaptation.py:130-143: identity metric, dual averaging started at ``initial_step_size`` (so the
        first step size is exp(0) = 1, algorithms.py:56-76)."""
        eng = get_engine()
        layout, scalar_position = _layout(initial_chain_state.position, num_chains)
        C, D = layout.C, layout.D
        full = bool(is_mass_matrix_full) and not scalar_position
        st, cst = eng.adapt_alloc(C, D, full)
        eng.adapt_init(C, D, float(initial_step_size), cst)
        ws = WarmupState(DualAveragingState(st["da_step"], st["da_x"], st["da_x_avg"], st["da_g_avg"], st["da_mu"]),
                         (st["wc_mean"], st["wc_m2"], st["wc_n"]), st["step_size"], st["imm"], st["sqrt_mass"],
                         st.get("work"), layout.user_shape, layout.C > 1 or num_chains is not None or
                         len(layout.user_shape) == 2)
        return ws, _params(layout, scalar_position, ws)

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
        D = layout.D
        full = warmup_state.imm.ndim == 3
        da, (mean, m2, n) = warmup_state.da_state, warmup_state.mm_state
        ws = WarmupState(DualAveragingState(*(t.clone() for t in da)), (mean.clone(), m2.clone(), n.clone()),
                         warmup_state.step_size.clone(), warmup_state.imm.clone(), warmup_state.sqrt_mass.clone(),
                         warmup_state.work, warmup_state.position_shape, warmup_state.batched)
        stage, window_end = schedule[int(step)]
        eng.adapt_update(C, D, stage, window_end, int(step) == len(schedule) - 1, float(target_acceptance_rate),
                         _dev_f64(chain_state.acceptance_probability, eng.device).reshape(C).contiguous(),
                         _dev_f64(position, eng.device).reshape(C, D).contiguous(), _cstate(eng, ws, full))
        return ws, _params(layout, scalar_position, ws)

    return init, update


_POOLED_FIELDS = ("da_step", "da_x", "da_x_avg", "da_g_avg", "da_mu", "wc_mean", "wc_m2", "wc_n", "step_size", "imm",
                  "sqrt_mass")


def _pooled_pair(schedule, is_mass_matrix_full, initial_step_size, target):
    """``window_adaptation(..., pooled=True)``: see there."""

    def _shape(position, num_chains):
        shape = tuple(position.shape)
        batched = num_chains is not None or len(shape) == 2
        C = (num_chains if num_chains is not None else shape[0]) if batched else 1
        return Layout(shape, batched, C), (len(shape) - (1 if batched else 0)) == 0

    def _ws(st, layout, batched):
        return WarmupState(DualAveragingState(st["da_step"], st["da_x"], st["da_x_avg"], st["da_g_avg"], st["da_mu"]),
                           (st["wc_mean"], st["wc_m2"], st["wc_n"]), st["step_size"], st["imm"], st["sqrt_mass"], None,
                           layout.user_shape, batched)

    def _params(scalar_position, ws):
        return PerChain(ws.step_size), (ws.imm.reshape(()) if scalar_position else ws.imm)

    def init(initial_chain_state: IntegratorState, num_chains: Optional[int] = None):
        eng = get_engine()
        layout, scalar_position = _shape(initial_chain_state.position, num_chains)
        full = is_mass_matrix_full and not scalar_position
        st, cst = eng.pooled_adapt_alloc(layout.C, layout.D, full)
        eng.pooled_adapt_init(layout.C, layout.D, initial_step_size, cst)
        ws = _ws(st, layout, layout.C > 1 or num_chains is not None or len(layout.user_shape) == 2)
        return ws, _params(scalar_position, ws)

    def update(step: int, warmup_state: WarmupState, parameters, chain_state):
        del parameters  # (the arrays in warmup_state ARE the current parameters)
        eng = get_engine()
        position = chain_state.state.position
        C = warmup_state.step_size.numel()
        if tuple(position.shape) != tuple(warmup_state.position_shape):
            raise ValueError(f"position has shape {tuple(position.shape)}, the warm-up was initialised with "
                             f"{tuple(warmup_state.position_shape)}")
        layout, scalar_position = _shape(position, C if warmup_state.batched else None)
        D = layout.D
        full = warmup_state.imm.ndim == 2
        da, (mean, m2, n) = warmup_state.da_state, warmup_state.mm_state
        old = dict(zip(_POOLED_FIELDS, (*da, mean, m2, n, warmup_state.step_size, warmup_state.imm,
                                        warmup_state.sqrt_mass)))
        st = {k: v.clone() for k, v in old.items()}  # states are values
        stage, window_end = schedule[int(step)]
        eng.pooled_adapt_update(C, D, stage, window_end, int(step) == len(schedule) - 1, target,
                                _dev_f64(chain_state.acceptance_probability, eng.device).reshape(C).contiguous(),
                                _dev_f64(position, eng.device).reshape(C, D).contiguous(), eng.pooled_cstate(st, full))
        ws = _ws(st, layout, warmup_state.batched)
        return ws, _params(scalar_position, ws)

    return init, update
