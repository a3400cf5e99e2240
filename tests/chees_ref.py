"""numpy restatement of the ChEES warm-up (include/aehmc_hip.h, aehmc_chees_init / aehmc_chees_update): one trajectory
length T and one step size adapted from all chains, written from the definition; imports nothing from aehmc_amd.  Also
a small numpy HMC for diagonal Gaussians, so that whole warm-ups run on the CPU.

One update with n = step, T = exp(log_T), h as stored, positions q0 / q1 [C, D] before / after the transition, the
returned momentum [C, D], accept flags and acceptance probabilities a [C]:
  m0, m1 = column means over ALL chains (math.fsum);  v_c = -imm o momentum_c (scalar / [D]) or -momentum_c . imm
  s_c = (|q1_c - m1|^2 - |q0_c - m0|^2) <q1_c - m1, v_c>  (long double);  A = sum accepted,  S = fsum(s_c, accepted only)
  G = h T S / max(A, 1), 0 when A = 0 or G is not finite;  Adam ascent on log_T;  abar = fsum(a) / C into dual averaging
  log_T clamped to [log eps, log(max_num_steps eps)];  log_T_avg = w log_T + (1 - w) log_T_avg, w = n^-kappa
  last: eps = exp(x_avg), log_T = log_T_avg;  step = n + 1, h = halton(n + 1), num_steps = max(1, ceil(h T / eps)) capped."""
import math
from typing import NamedTuple

import numpy as np

GAMMA, T0, KAPPA = 0.05, 10, 0.75  # step_size.py:9-14
U52 = 2.0 ** -52


class CheesState(NamedTuple):
    step: int
    log_T: float
    log_T_avg: float
    adam_m: float
    adam_v: float
    h: float
    num_steps: int
    da_step: int
    da_x: float
    da_x_avg: float
    da_g_avg: float
    da_mu: float
    step_size: float


def halton(n):
    """Base-2 radical inverse of n >= 1."""
    h, f = 0.0, 0.5
    while n:
        if n & 1:
            h += f
        n >>= 1
        f *= 0.5
    return h


def ratio(h, T, eps):
    """h T / eps, whose ceiling is the number of leapfrogs."""
    return (h * T) / eps


def num_steps_of(h, T, eps, most):
    r = math.ceil(ratio(h, T, eps)) if math.isfinite(ratio(h, T, eps)) else 1
    return int(min(max(r, 1), most))


def init(initial_step_size=1.0, initial_trajectory_length=None) -> CheesState:
    T = float(initial_step_size if initial_trajectory_length is None else initial_trajectory_length)
    log_T, eps = math.log(T), float(np.exp(0.0))
    return CheesState(1, log_T, log_T, 0.0, 0.0, 0.5, num_steps_of(0.5, math.exp(log_T), eps, 1 << 62), 1, 0.0, 0.0, 0.0,
                      float(initial_step_size), eps)


def velocity(momentum, imm):
    """-M^-1 momentum in long double; imm: scalar, [D] or [D, D]."""
    p = np.asarray(momentum, dtype=np.longdouble)
    imm = np.asarray(imm, dtype=np.longdouble)
    return -(p @ imm) if imm.ndim == 2 else -(imm * p)


class Sums(NamedTuple):
    S: float
    A: float
    abar: float
    m0: np.ndarray
    m1: np.ndarray
    S_bound: float      # n 2^-52 sum|terms| of each sum (see ``sums``)
    abar_bound: float
    m0_bound: np.ndarray
    m1_bound: np.ndarray


def sums(q0, q1, momentum, imm, accepted, a) -> Sums:
    """The sums of one update and their bounds: n 2^-52 sum|terms| for a sum of n terms, which holds for a
    double-precision sum of those terms in any order (2^-52 is twice the unit round-off; for the means a further
    2^-52 |m| covers the division and the rounding of the fsum value itself).

    n = C throughout.  The terms of S are the s_c of the accepted chains.  They are computed quantities -- D-term dot
    products about the rounded means -- so for S the bound is the acceptance bound the kernel is held to, not a theorem
    about every correct evaluation; on the shapes of tests/test_gpu_chees.py the device's S lies within 0.55 of it
    (C = 5, D = 7; 0.27 at C = 3, D = 1; below 0.01 from C = 64 on)."""
    q0, q1 = np.asarray(q0, dtype=np.float64), np.asarray(q1, dtype=np.float64)
    C, D = q0.shape
    acc = np.asarray(accepted).astype(bool)
    m0 = np.array([math.fsum(q0[:, j]) / C for j in range(D)])
    m1 = np.array([math.fsum(q1[:, j]) / C for j in range(D)])
    m0_b = C * U52 * np.abs(q0).sum(0) / C + U52 * np.abs(m0)
    m1_b = C * U52 * np.abs(q1).sum(0) / C + U52 * np.abs(m1)
    abar = math.fsum(a) / C
    abar_b = C * U52 * float(np.abs(a).sum()) / C + U52 * abs(abar)
    ld = np.longdouble
    s = np.zeros(C)
    rows = np.flatnonzero(acc)
    if rows.size:
        d0 = q0[rows].astype(ld) - m0.astype(ld)
        d1 = q1[rows].astype(ld) - m1.astype(ld)
        v = velocity(np.asarray(momentum, dtype=np.float64)[rows], imm)
        s[rows] = (((d1 * d1).sum(1) - (d0 * d0).sum(1)) * (d1 * v).sum(1)).astype(np.float64)
    return Sums(math.fsum(s[rows]), float(acc.sum()), abar, m0, m1, C * U52 * float(np.abs(s).sum()), abar_b, m0_b, m1_b)


def update(s: CheesState, is_last, S, A, abar, target=0.651, lr=0.025, max_steps=1000) -> CheesState:
    """One update from the sums (``sums`` above, or a device's own)."""
    n, h = s.step, s.h
    T = math.exp(s.log_T)
    with np.errstate(all="ignore"):
        G = float(np.float64(h * T) * np.float64(S) / max(A, 1.0))
    if A == 0 or not math.isfinite(G):
        G = 0.0
    m = 0.9 * s.adam_m + 0.1 * G
    v = 0.999 * s.adam_v + 0.001 * (G * G)
    mhat, vhat = m / (1.0 - 0.9 ** n), v / (1.0 - 0.999 ** n)
    log_T = s.log_T + lr * (mhat / (math.sqrt(vhat) + 1e-8))
    # dual averaging with the mean acceptance probability (algorithms.py:78-115)
    eta = 1.0 / (s.da_step + T0)
    g_avg = (1.0 - eta) * s.da_g_avg + eta * (target - abar)
    x = s.da_mu - (math.sqrt(s.da_step) / GAMMA) * g_avg
    x_eta = float(s.da_step) ** (-KAPPA)
    x_avg = x_eta * s.da_x + (1.0 - x_eta) * s.da_x_avg
    eps = math.exp(x)
    log_T = min(max(log_T, math.log(eps)), math.log(max_steps * eps))
    w = float(n) ** (-KAPPA)
    log_T_avg = w * log_T + (1.0 - w) * s.log_T_avg
    if is_last:
        eps, log_T = math.exp(x_avg), log_T_avg
    h1 = halton(n + 1)
    return CheesState(n + 1, log_T, log_T_avg, m, v, h1, num_steps_of(h1, math.exp(log_T), eps, max_steps), s.da_step + 1,
                      x, x_avg, g_avg, s.da_mu, eps)


def update_from_arrays(s, is_last, q0, q1, momentum, imm, accepted, a, **kw) -> CheesState:
    t = sums(q0, q1, momentum, imm, accepted, a)
    return update(s, is_last, t.S, t.A, t.abar, **kw)


# ---- a numpy HMC for N(0, diag(sigma^2)), all chains at once ----
def hmc_transition(rng, q, sigma, imm, eps, L):
    """One static-HMC transition with a diagonal (or scalar) inverse mass matrix.  Returns the state the reference's
    kernel returns: ``(position, momentum, accepted, acceptance probability)`` -- on accept the proposal with the
    momentum flipped (hmc.py:185), otherwise the start."""
    imm = np.broadcast_to(np.asarray(imm, dtype=np.float64), q.shape[1:])
    prec = 1.0 / (sigma * sigma)
    p0 = rng.normal(size=q.shape) / np.sqrt(imm)
    x, p = q.copy(), p0 - 0.5 * eps * (q * prec)
    for i in range(L):
        x = x + eps * (imm * p)
        p = p - (eps if i < L - 1 else 0.5 * eps) * (x * prec)
    H0 = 0.5 * (q * q * prec).sum(1) + 0.5 * (p0 * p0 * imm).sum(1)
    H1 = 0.5 * (x * x * prec).sum(1) + 0.5 * (p * p * imm).sum(1)
    d = H0 - H1
    d = np.where(np.isnan(d), -np.inf, d)
    with np.errstate(over="ignore"):
        alpha = np.clip(np.exp(d), 0.0, 1.0)
    acc = rng.random(q.shape[0]) < alpha
    return np.where(acc[:, None], x, q), np.where(acc[:, None], -p, p0), acc, alpha


def warmup(sigma, imm, C, num_steps, seed, **kw):
    """A whole ChEES warm-up on the CPU from standard-normal starts; returns ``(T, eps)``."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(C, len(sigma)))
    s = init()
    for i in range(num_steps):
        q1, mom, acc, alpha = hmc_transition(rng, q, sigma, imm, s.step_size, s.num_steps)
        s = update_from_arrays(s, i == num_steps - 1, q, q1, mom, imm, acc, alpha, **kw)
        q = q1
    return math.exp(s.log_T), s.step_size
