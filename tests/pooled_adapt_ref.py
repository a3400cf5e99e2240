"""numpy restatement of POOLED window adaptation (include/aehmc_hip.h, aehmc_pooled_adapt_update): one dual-averaging
state, one Welford state and one step size / inverse mass matrix adapted from all chains together.  Written from the
definition; imports nothing from aehmc_amd.

One warm-up step with positions X [C, D] and acceptance probabilities a [C] after the transition:
  abar = mean(a) goes through the reference's dual-averaging update (algorithms.py:78-115);
  slow stage, batch Welford (Chan et al.) with b = mean(X, axis 0):
    n' = n + C, d = b - mean, mean' = mean + d (C / n'), m2' = m2 + sum_c (X_c - b)(X_c - b)^T + (n C / n') d d^T
    (a diagonal metric keeps the diagonal of the last line);
  window end: cov = m2 / (n - 1), imm = (n / (n + 5)) cov + 1e-3 (5 / (n + 5)) (on the diagonal only when dense),
    sqrt_mass = sqrt(1 / imm) or chol(imm)^-T, Welford state zeroed, dual averaging restarted around the step size;
  after the last step the step size is exp(x_avg)."""
from typing import List, NamedTuple, Tuple

import numpy as np

GAMMA, T0, KAPPA = 0.05, 10, 0.75  # step_size.py:9-14


class PooledState(NamedTuple):
    step: int
    x: float
    x_avg: float
    g_avg: float
    mu: float
    mean: np.ndarray
    m2: np.ndarray
    n: int
    step_size: float
    imm: np.ndarray
    sqrt_mass: np.ndarray


def build_schedule(num_steps, initial_buffer_size=75, final_buffer_size=50, first_window_size=25) -> List[Tuple[int, bool]]:
    """(stage, is_window_end) per step: a fast buffer, slow windows that double, a fast buffer."""
    if num_steps < 20:
        return [(0, False)] * num_steps
    if initial_buffer_size + first_window_size + final_buffer_size > num_steps:
        initial_buffer_size = int(0.15 * num_steps)
        final_buffer_size = int(0.1 * num_steps)
        first_window_size = num_steps - initial_buffer_size - final_buffer_size
    end = num_steps - final_buffer_size
    out = [(0, False)] * initial_buffer_size
    start, size = initial_buffer_size, first_window_size
    while start < end:
        this = size if 3 * size <= end - start else end - start
        size = 2 * size
        out += [(1, False)] * (this - 1) + [(1, True)]
        start += this
    return out + [(0, False)] * (num_steps - end)


def sqrt_mass_of(imm, full):
    if not full:
        return np.sqrt(1.0 / imm)
    return np.triu(np.linalg.inv(np.linalg.cholesky(imm)).T)  # (L^-T is upper triangular; inv leaves rounding below)


def shrink(cov, n, full):
    """Stan's regularisation of a window's covariance estimate from n draws."""
    scaled = (n / (n + 5)) * cov
    eps = 1e-3 * (5 / (n + 5))
    return scaled + eps * np.eye(cov.shape[0]) if full else scaled + eps


def init(D, full, initial_step_size=1.0) -> PooledState:
    one = np.eye(D) if full else np.ones(D)
    return PooledState(1, 0.0, 0.0, 0.0, float(initial_step_size), np.zeros(D), np.zeros((D, D) if full else D), 0,
                       float(np.exp(0.0)), one, one.copy())


def update(s: PooledState, stage, window_end, last, X, a, target=0.8) -> PooledState:
    X = np.asarray(X, dtype=np.float64)
    C, D = X.shape
    full = s.m2.ndim == 2
    # dual averaging with the mean acceptance probability
    abar = float(np.sum(a) / C)
    eta = 1.0 / (s.step + T0)
    g_avg = (1.0 - eta) * s.g_avg + eta * (target - abar)
    x = s.mu - (np.sqrt(s.step) / GAMMA) * g_avg
    x_eta = float(s.step) ** (-KAPPA)
    x_avg = x_eta * s.x + (1.0 - x_eta) * s.x_avg
    step, mu = s.step + 1, s.mu
    step_size = float(np.exp(x))
    mean, m2, n, imm, sqrt_mass = s.mean, s.m2, s.n, s.imm, s.sqrt_mass
    if stage != 0:
        b = X.sum(axis=0) / C
        n1 = n + C
        d = b - mean
        mean = mean + d * (C / n1)
        Xc = X - b
        w = n * C / n1
        m2 = m2 + (Xc.T @ Xc + w * np.outer(d, d) if full else (Xc * Xc).sum(axis=0) + w * d * d)
        n = n1
    if window_end:
        imm = shrink(m2 / (n - 1), n, full)
        sqrt_mass = sqrt_mass_of(imm, full)
        mean, m2, n = np.zeros_like(mean), np.zeros_like(m2), 0
        step, x, x_avg, g_avg, mu = 1, 0.0, 0.0, 0.0, step_size  # restart around the current step size
    if last:
        step_size = float(np.exp(x_avg))
    return PooledState(step, float(x), float(x_avg), float(g_avg), float(mu), mean, m2, n, step_size, imm, sqrt_mass)


def run(transition, X0, num_steps, full, initial_step_size=1.0, target=0.8):
    """The pooled warm-up loop around ``transition(X, step_size, imm) -> (X', a)`` over all chains."""
    schedule = build_schedule(num_steps)
    s = init(X0.shape[1], full, initial_step_size)
    X = X0
    for i, (stage, wend) in enumerate(schedule):
        X, a = transition(X, s.step_size, s.imm)
        s = update(s, stage, wend, i == num_steps - 1, X, a, target)
    return X, s
