"""numpy restatement of generalised HMC and the MEADS update (Hoffman & Sountsov, "Tuning-Free Generalized Hamiltonian
Monte Carlo", AISTATS 2022; the all-chains variant), written from the description of the method, not from the kernels.

``lam`` takes the eigenvalue estimate in its literal C x C form (the device goes through the D x D matrix);
``transition`` draws from per-chain ``np.random.Generator(PCG64(...))`` objects built as oracle/np_oracle.py builds the
two HMC call sites (``SeedSequence(seed).spawn(2)``); ``update`` and ``warmup`` complete it."""
from typing import NamedTuple, Optional

import numpy as np

LOG_SQRT_2PI = 0.91893853320467267


# ---- targets: potential energy [C] and its gradient [C, D], in the elementwise order the kernels use -----------------
class StdNormal:
    name = "std_normal"

    def __init__(self, D):
        self.D = D

    def __call__(self, q):
        return np.sum(0.5 * (q * q) + LOG_SQRT_2PI, axis=1), q.copy()


class Isotropic:
    name = "isotropic"

    def __init__(self, D):
        self.D = D

    def __call__(self, q):
        return 0.5 * np.sum(q * q, axis=1), q.copy()


class DiagGaussian:
    name = "diag_gaussian"

    def __init__(self, mu, sigma):
        self.mu, self.sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        self.D = self.mu.size

    def __call__(self, q):
        z = (q - self.mu) / self.sigma
        return np.sum(0.5 * (z * z) + np.log(self.sigma) + LOG_SQRT_2PI, axis=1), z / self.sigma


class Funnel:
    """Neal's funnel, v = q[0], x = q[1:]: logp = -v^2 / 18 + sum_i (-x_i^2 exp(-v) / 2 - v / 2); analytic gradient."""
    name = "funnel"

    def __init__(self, D):
        self.D = D

    def __call__(self, q):
        v, x = q[:, 0], q[:, 1:]
        e = np.exp(-v)
        U = v * v / 18.0 + np.sum(0.5 * x * x * e[:, None] + 0.5 * v[:, None], axis=1)
        g = np.empty_like(q)
        g[:, 0] = v / 9.0 + np.sum(-0.5 * x * x * e[:, None] + 0.5, axis=1)
        g[:, 1:] = x * e[:, None]
        return U, g


def funnel_logp(q):
    """The same density as a Python function of one chain's position (traced by aehmc_amd.tracing)."""
    v, x = q[0], q[1:]
    return -v * v / 18.0 + (-0.5 * x * x * np.exp(-v) - 0.5 * v).sum()


# ---- generators ------------------------------------------------------------------------------------------------------
def sites(seeds):
    """Per chain the two call sites of a kernel built first from ``RandomStream(seeds=seeds)``: (#1 momentum, #2 slice)."""
    g1, g2 = [], []
    for s in seeds:
        a, b = np.random.SeedSequence(int(s)).spawn(2)
        g1.append(np.random.Generator(np.random.PCG64(a)))
        g2.append(np.random.Generator(np.random.PCG64(b)))
    return g1, g2


def site_states(gens1, gens2):
    """uint64 [C, 2, 4] as RandomStream.sites lays generator states out: (state hi, state lo, inc hi, inc lo)."""
    M = (1 << 64) - 1
    out = np.empty((len(gens1), 2, 4), dtype=np.uint64)
    for c, pair in enumerate(zip(gens1, gens2)):
        for k, g in enumerate(pair):
            st = g.bit_generator.state["state"]
            out[c, k] = (st["state"] >> 64, st["state"] & M, st["inc"] >> 64, st["inc"] & M)
    return out


# ---- the transition --------------------------------------------------------------------------------------------------
class Chains(NamedTuple):
    q: np.ndarray             # [C, D]
    U: np.ndarray             # [C]
    g: np.ndarray             # [C, D]
    v: Optional[np.ndarray]   # [C, D] whitened momentum, None before the first transition
    u: Optional[np.ndarray]   # [C] slice variable, None before the first transition


class Info(NamedTuple):
    accepted: np.ndarray
    acceptance_probability: np.ndarray
    is_diverging: np.ndarray
    margin: np.ndarray        # |log|u| - Delta|: how far the accept test was from flipping
    energy_change: np.ndarray  # Delta = H0 - H1 (-inf for NaN)


def start(target, q0) -> Chains:
    q = np.array(q0, dtype=np.float64)
    U, g = target(q)
    return Chains(q, U, g, None, None)


def transition(ch: Chains, gens1, gens2, target, eps, alpha, delta, s, threshold=1000.0):
    """One generalised-HMC transition of every chain; ``s``: the scale, a scalar or [D]."""
    C, D = ch.q.shape
    z = np.stack([g.standard_normal(D) for g in gens1])
    v = z if ch.v is None else np.sqrt(1.0 - alpha) * ch.v + np.sqrt(alpha) * z
    u = ch.u
    if u is None:
        u = np.array([2.0 * g.random() - 1.0 for g in gens2])
    u = np.fmod((u + 1.0) + delta, 2.0) - 1.0
    H0 = ch.U + 0.5 * np.sum(v * v, axis=1)
    b = 0.5 * eps
    vh = v - b * (s * ch.g)
    qn = ch.q + eps * (s * vh)
    Un, gn = target(qn)
    vn = vh - b * (s * gn)
    with np.errstate(all="ignore"):
        d = H0 - (Un + 0.5 * np.sum(vn * vn, axis=1))
        d = np.where(np.isnan(d), -np.inf, d)
        logu = np.log(np.abs(u))
        acc = (d > -np.inf) & (logu <= d)
        pa = np.minimum(1.0, np.exp(d))
        un = np.where(acc, u * np.exp(-d), u)
        margin = np.abs(logu - d)
    a = acc[:, None]
    new = Chains(np.where(a, qn, ch.q), np.where(acc, Un, ch.U), np.where(a, gn, ch.g), np.where(a, vn, -v), un)
    return new, Info(acc, pa, np.abs(d) > threshold, margin, d)


# ---- the adaptation --------------------------------------------------------------------------------------------------
def slice_step(u_in, info: Info, delta):
    """The slice one transition makes of ``u_in``, given the transition's accept flags and energy change."""
    u = np.fmod((u_in + 1.0) + delta, 2.0) - 1.0
    with np.errstate(all="ignore"):
        return np.where(info.accepted, u * np.exp(-info.energy_change), u)


def lam(X):
    """The largest-eigenvalue estimate of X [n, d] from its n x n Gram matrix, as written."""
    n = X.shape[0]
    S = X @ X.T
    d = np.diag(S)
    return ((np.sum(S * S) - np.sum(d * d)) / (n * (n - 1))) / (np.sum(d) / n)


def lam_dxd(X):
    """The same number through the d x d matrix: sum_ab S_ab^2 = |X^T X|_F^2, S_aa = |x_a|^2."""
    n = X.shape[0]
    M = X.T @ X
    d = np.sum(X * X, axis=1)
    return ((np.sum(M * M) - np.sum(d * d)) / (n * (n - 1))) / (np.sum(d) / n)


class Meads(NamedTuple):
    eps: float
    alpha: float
    delta: float
    scale: np.ndarray
    count: int
    skipped: int


def init(D, initial_step_size=0.01) -> Meads:
    return Meads(float(initial_step_size), 1.0, 0.5, np.ones(D), 0, 0)


def statistics(Q, G):
    """What an update sums, by name (the device's optional copy holds the same numbers)."""
    C = Q.shape[0]
    m = Q.mean(axis=0)
    var = np.sum((Q - m) ** 2, axis=0) / C
    with np.errstate(all="ignore"):
        sd = np.sqrt(var)
        Z = (Q - m) / sd
        Gs = G * sd
        nz, ng = np.sum(Z * Z, axis=1), np.sum(Gs * Gs, axis=1)
        Mz, Mg = Z.T @ Z, Gs.T @ Gs
        return dict(z4=np.sum(nz * nz), z2=np.sum(nz), g4=np.sum(ng * ng), g2=np.sum(ng), Fz=np.sum(Mz * Mz),
                    Fg=np.sum(Mg * Mg), lam_z=lam(Z), lam_g=lam(Gs), m=m, sd=sd)


def update(st: Meads, Q, G, step_size_multiplier=0.5, damping_slowdown=1.0) -> Meads:
    t = statistics(Q, G)
    with np.errstate(all="ignore"):
        eps = min(1.0, step_size_multiplier / np.sqrt(t["lam_g"]))
        gamma = max(1.0 / np.sqrt(t["lam_z"]), 1.0 / ((st.count + 1) ** damping_slowdown * eps))
        alpha = 1.0 - np.exp(-2.0 * eps * gamma)
        delta = alpha / 2.0
    sd = t["sd"]
    ok = (np.isfinite([eps, alpha, delta]).all() and np.isfinite(sd).all() and eps > 0 and (sd != 0).all())
    if not ok:
        return st._replace(count=st.count + 1, skipped=st.skipped + 1)
    return Meads(float(eps), float(alpha), float(delta), sd, st.count + 1, st.skipped)


def warmup(target, q0, seeds, num_steps, step_size_multiplier=0.5, damping_slowdown=1.0, initial_step_size=0.01,
           record=None):
    """An update on the starting state, then ``num_steps`` x (transition on the current parameters, update).  Returns
    ``(Chains, Meads, (gens1, gens2), smallest margin)``; ``record``: a list that receives the Meads state after every
    update."""
    g1, g2 = sites(seeds)
    ch = start(target, q0)
    st = update(init(ch.q.shape[1], initial_step_size), ch.q, ch.g, step_size_multiplier, damping_slowdown)
    if record is not None:
        record.append(st)
    margin = np.inf
    for _ in range(int(num_steps)):
        ch, info = transition(ch, g1, g2, target, st.eps, st.alpha, st.delta, st.scale)
        margin = min(margin, float(info.margin.min()))
        st = update(st, ch.q, ch.g, step_size_multiplier, damping_slowdown)
        if record is not None:
            record.append(st)
    return ch, st, (g1, g2), margin


# ---- fixtures shared by the host and the GPU tests -------------------------------------------------------------------
PARITY = dict(eps=0.37, alpha=0.6, delta=0.3, steps=12)
PARITY_SHAPES = [(1, 1), (3, 1), (5, 7), (64, 64), (65, 65), (6, 129), (5, 257), (5, 1000), (4, 1024)]
PARITY_TARGETS = ("diag_gaussian", "isotropic", "std_normal")
FUNNEL_DIMS = (10, 100, 1000)
LOOP = dict(C=8, D=5, steps=20)
GOLDEN = dict(C=256, D=20, steps=300, seeds=16)
GOLDEN_SIGMA = {"std_normal": np.ones(20), "diag_gaussian": np.linspace(1.0, 10.0, 20)}


def parity_scale(D):
    return np.linspace(0.8, 1.6, D)


def parity_target(name, D):
    if name == "std_normal":
        return StdNormal(D)
    if name == "isotropic":
        return Isotropic(D)
    r = np.random.default_rng(7 * D + 1)
    return DiagGaussian(r.normal(size=D), 0.5 + r.random(D))


def parity_seeds(name, C, D):
    """The chains' seeds of one parity case (chosen so that no accept test is within 1e-6 of flipping:
    tests/test_meads_host.py checks that)."""
    base = 100000 * (1 + PARITY_TARGETS.index(name)) + 1000 * C + D
    return [base + c for c in range(C)]


def parity_start(name, C, D):
    r = np.random.default_rng(31 * C + D)
    t = parity_target(name, D)
    q0 = r.normal(size=(C, D))
    if name == "diag_gaussian":
        q0 = t.mu + t.sigma * q0
    return t, q0


def parity_run(name, C, D, steps=None):
    """The reference of one parity case: the chains after every transition, the infos, the generators."""
    t, q0 = parity_start(name, C, D)
    g1, g2 = sites(parity_seeds(name, C, D))
    ch, hist = start(t, q0), []
    for _ in range(PARITY["steps"] if steps is None else steps):
        ch, info = transition(ch, g1, g2, t, PARITY["eps"], PARITY["alpha"], PARITY["delta"], parity_scale(D))
        hist.append((ch, info))
    return t, q0, hist, (g1, g2)


def funnel_start(D, C=4):
    r = np.random.default_rng(900 + D)
    q0 = 0.3 * r.normal(size=(C, D))
    return Funnel(D), q0, [7000 + 10 * D + c for c in range(C)]


def funnel_run(D, steps=6):
    t, q0, seeds = funnel_start(D)
    g1, g2 = sites(seeds)
    ch, hist = start(t, q0), []
    for _ in range(steps):
        ch, info = transition(ch, g1, g2, t, 0.05, PARITY["alpha"], PARITY["delta"], 1.0)
        hist.append((ch, info))
    return t, q0, seeds, hist


def loop_start():
    C, D = LOOP["C"], LOOP["D"]
    sigma = np.linspace(1.0, 3.0, D)
    r = np.random.default_rng(4242)
    return DiagGaussian(np.zeros(D), sigma), r.normal(size=(C, D)) * sigma, [555 + c for c in range(C)]


def golden_start(name, k):
    """Target, starting positions and chain seeds of golden run ``k`` on target ``name``."""
    C, D = GOLDEN["C"], GOLDEN["D"]
    sigma = GOLDEN_SIGMA[name]
    t = StdNormal(D) if name == "std_normal" else DiagGaussian(np.zeros(D), sigma)
    q0 = np.random.default_rng(1000 + k).normal(size=(C, D))
    return t, q0, [100000 * (k + 1) + c for c in range(C)]


def golden_run(name, k):
    """``(eps, alpha, log(scale / sigma) [D])`` after the golden warm-up ``k``."""
    t, q0, seeds = golden_start(name, k)
    _, st, _, _ = warmup(t, q0, seeds, GOLDEN["steps"])
    return st.eps, st.alpha, np.log(st.scale / GOLDEN_SIGMA[name])


if __name__ == "__main__":  # python tests/meads_ref.py: rewrites tests/golden/meads_ref_runs.json (about a minute)
    import json
    import os
    doc = dict(GOLDEN)
    for name in GOLDEN_SIGMA:
        runs = [golden_run(name, k) for k in range(GOLDEN["seeds"])]
        doc[name] = dict(eps=[r[0] for r in runs], alpha=[r[1] for r in runs], log_scale_ratio=[r[2].tolist() for r in runs])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meads_ref_runs.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", path)
