"""Case tables and helpers of the non-finite-energy tests (tests/test_nonfinite_host.py, tests/test_gpu_nonfinite.py).

The reference's rules for a density that overflows or returns NaN: a NaN energy difference becomes -inf, the step
diverges and p_accept is 0 (aehmc/hmc.py:189-195, proposals.py:43-45); a NaN expit becomes 0 (proposals.py:95-97); after
a first step that diverged the scan still runs and still draws (trajectory.py:336).  The tables below reach them three
ways: by the start position, by the step size, and by a density with a wall that the trajectory crosses in mid-tree."""
import numpy as np

from oracle import c_oracle as co
from oracle import np_oracle as no

RTOL = 1e-9  # the suite's parity tolerance (tests/test_gpu_parity.py)
NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF], dtype=np.uint64).view(np.float64)[0]  # a quiet NaN that can be recognised

# ---------------------------------------------------------------------------------------------- 1. poisoned starts
GAUSS_POISONS = ("scale", "overflow", "nan_last", "nan_first", "inf_last")
LINREG_POISONS = ("logn800", "nan_last", "nan_first", "inf_last")
C_DEFAULT, C_TEAMS = 23, 70  # neither a multiple of 4 nor of 16; 70: a wavefront of sub-wavefront teams holds both kinds


def is_poisoned(C):
    return np.arange(C) % 3 == 1


def scale_for(D):
    """|q0| ~ 1e150: every value finite and H0 about 1e300.  Divided by sqrt(D) so that the exact sum of squares of a chain
    is about 1e300 at every D: with 1 / sigma^2 <= 4, the largest eigenvalue of a metric of the tables below 10 and a
    64-step momentum sum, no sum of products of the transition exceeds 1e304 in ANY summation order (asserted by
    `assert_scale_is_order_safe`), so no reduction can overflow where another does not."""
    return 1e150 / np.sqrt(D)


def assert_scale_is_order_safe(q0):
    sq = np.array([sum(float(x) ** 2 for x in row if np.isfinite(x) and abs(x) < 1e155) for row in q0])
    assert sq.max() * 1e4 < 1e305, sq.max()


def poison_starts(q0, poisons, rnd, scale=None):
    """A copy of the healthy starts ``q0`` [C, D] with the chains c % 3 == 1 poisoned, the poisons cycled over them;
    returns it with the list of each chain's label ("healthy" or the poison)."""
    C, D = q0.shape
    q, labels = q0.copy(), ["healthy"] * C
    scale = scale_for(D) if scale is None else scale
    for k, c in enumerate(np.flatnonzero(is_poisoned(C))):
        kind = poisons[k % len(poisons)]
        labels[c] = kind
        if kind == "scale":
            q[c] = scale * rnd.normal(size=D)
        elif kind == "overflow":
            q[c] = 1e160 * rnd.normal(size=D)
        elif kind == "nan_last":
            q[c, D - 1] = NAN_PAYLOAD
        elif kind == "nan_first":
            q[c, 0] = NAN_PAYLOAD
        elif kind == "inf_last":
            q[c, D - 1] = np.inf
        elif kind == "logn800":  # (LinearRegression: q = [w, log n], exp(800) overflows)
            q[c, 1] = 800.0
        else:
            raise KeyError(kind)
    assert set(labels) == set(poisons) | {"healthy"}, "the call must see every poison"
    return q, labels


# ---------------------------------------------------------------------------------------------- 3. poisoned step sizes
EPS_POISONS = (1e154, 1e200, 1e308, np.inf, np.nan)
NEVER_FIRES = ((np.inf, 1e38), (np.inf, 1e60), (1e308, 1e38), (1e308, 1e60))  # (divergence_threshold, step size)


def poison_step_sizes(C, eps):
    out = np.full(C, float(eps))
    for k, c in enumerate(np.flatnonzero(is_poisoned(C))):
        out[c] = EPS_POISONS[k % len(EPS_POISONS)]
    return out


# ---------------------------------------------------------------------------------------------- comparisons
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def assert_reals(got, want, atol=0.0, what=""):
    """`equal_nan` parity: finite entries at RTOL, non-finite entries of the same class and sign."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    bad = np.flatnonzero((np.isfinite(got) != fin).reshape(-1))
    assert bad.size == 0, (what, "finite on one side only", bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
    np.testing.assert_allclose(got[fin], want[fin], rtol=RTOL, atol=atol, err_msg=str(what))
    assert np.array_equal(np.isnan(got[~fin]), np.isnan(want[~fin])), (what, "NaN against inf")
    inf = ~fin & np.isinf(want)
    assert np.array_equal(np.sign(got[inf]), np.sign(want[inf])), (what, "sign of inf")


def stayed(q_before, q_after):
    """chains [C] whose position the oracle left in place (bitwise, NaN payloads included)"""
    return (bits(q_before) == bits(q_after)).all(axis=1)


# ---------------------------------------------------------------------------------------------- oracle runners
class SiteStream:
    """np_oracle.RandomStream look-alike over explicit PCG64 states ([n_sites, 4] uint64 as c_oracle.site_states lays them
    out): the k-th call site is the k-th state; keeps the generators so that their states can be read back."""

    def __init__(self, states):
        self.gens = []
        for st in states:
            bg = np.random.PCG64()
            bg.state = {"bit_generator": "PCG64", "has_uint32": 0, "uinteger": 0,
                        "state": {"state": (int(st[0]) << 64) | int(st[1]), "inc": (int(st[2]) << 64) | int(st[3])}}
            self.gens.append(np.random.Generator(bg))
        self.k = 0

    def site(self):
        self.k += 1
        return self.gens[self.k - 1]

    def words(self):
        M = (1 << 64) - 1
        out = np.empty((len(self.gens), 2), dtype=np.uint64)
        for k, g in enumerate(self.gens):
            s = g.bit_generator.state["state"]["state"]
            out[k] = (s >> 64, s & M)
        return out


def np_chain_run(sampler, target, rng_c, q0_c, eps, imm, T, L=7, max_exp=6, thr=1000.0):
    """T transitions of ONE chain on oracle/np_oracle.py from the site states ``rng_c`` [n_sites, 4]; returns per
    transition a dict of the outputs and the generator words afterwards."""
    srng = SiteStream(rng_c)
    kern = (no.nuts_kernel(srng, target, max_num_expansions=max_exp, divergence_threshold=thr) if sampler == "nuts"
            else no.hmc_kernel(srng, target, divergence_threshold=thr))
    with np.errstate(all="ignore"):
        state = no.new_state(np.array(q0_c, dtype=np.float64), target)
        out = []
        for _ in range(T):
            trace = []
            d = kern(state, eps, imm, trace) if sampler == "nuts" else kern(state, eps, imm, L)
            state = d.state._replace(momentum=None)
            # the last sub-trajectory diverged at its FIRST step (its scan then ran on as a phantom, trajectory.py:336)
            first_step = bool(trace and trace[-1]["is_div"] and trace[-1]["sub_len"] == 1)
            out.append(dict(position=np.array(d.state.position), potential_energy=float(d.state.potential_energy),
                            potential_energy_grad=np.array(d.state.potential_energy_grad), momentum=np.array(d.state.momentum),
                            acceptance_probability=float(d.acceptance_probability), is_diverging=bool(d.is_diverging),
                            is_turning=bool(d.is_turning) if sampler == "nuts" else False,
                            num_doublings=int(d.num_doublings) if sampler == "nuts" else 0,
                            n_leapfrog=int(d.n_leapfrog), words=srng.words(), first_step_divergence=first_step))
    return out


def np_run(sampler, target, rng, q0, eps, imm, T, **kw):
    """every chain of ``np_chain_run``, stacked: a list over transitions of dicts of [C, ...] arrays; ``eps`` a scalar or
    one step size per chain"""
    C = q0.shape[0]
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64), (C,))
    chains = [np_chain_run(sampler, target, rng[c], q0[c], float(eps[c]), imm, T, **kw) for c in range(C)]
    return [{k: np.stack([np.asarray(chains[c][t][k]) for c in range(C)]) for k in chains[0][t]} for t in range(T)]


def c_run(sampler, otgt, imm, rng, q0, eps, T, L=7, max_exp=6, thr=1000.0, per_chain_imm=False):
    """T transitions on the C oracle; ``eps`` a scalar or one step size per chain and ``imm`` one metric or (per_chain_imm)
    one per chain: chain by chain then.  Returns (list over transitions of output dicts with the state arrays and
    generator words after it, final rng)."""
    D, C = otgt.D, q0.shape[0]
    rng = rng.copy()
    q, U, g = co.new_state(otgt, q0.copy())
    eps_c = np.broadcast_to(np.asarray(eps, dtype=np.float64), (C,))
    alone = per_chain_imm or np.ndim(eps) > 0

    def call(metric, r, e, qq, UU, gg):
        return (co.nuts_step(otgt, metric, r, e, qq, UU, gg, max_exp=max_exp, thr=thr) if sampler == "nuts"
                else co.hmc_step(otgt, metric, r, e, L, qq, UU, gg, thr=thr))

    out = []
    for _ in range(T):
        if not alone:
            res = call(co.Metric(imm, D), rng, float(eps), q, U, g)
        else:
            parts = []
            for c in range(C):
                metric = co.Metric(imm[c] if per_chain_imm else imm, D)
                qc, Uc, gc, rc = q[c:c + 1].copy(), U[c:c + 1].copy(), g[c:c + 1].copy(), rng[c:c + 1].copy()
                parts.append(call(metric, rc, float(eps_c[c]), qc, Uc, gc))
                q[c], U[c], g[c], rng[c] = qc[0], Uc[0], gc[0], rc[0]
            res = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        res.update(position=q.copy(), potential_energy=U.copy(), potential_energy_grad=g.copy(), words=rng[:, :, :2].copy())
        out.append(res)
    return out


DISCRETE = ("is_diverging", "is_turning", "num_doublings", "n_leapfrog")
REALS = (("position", 1e-12), ("potential_energy", 0.0), ("potential_energy_grad", 1e-9), ("momentum", 1e-12),
         ("acceptance_probability", 0.0))  # (name, atol): the absolute terms of test_kernel_family_with_planted_momentum_states


def assert_same_transition(a, b, sampler, what=""):
    """two runs reduced to the same dicts (two oracles, an oracle and a device run, two device routes) agree on one
    transition, in every output that ``a`` holds"""
    for k in DISCRETE:
        if k not in a or (sampler == "hmc" and k in ("is_turning", "num_doublings")):
            continue
        assert np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)), (what, k, a[k], b[k])
    if "words" in a:
        assert np.array_equal(a["words"], b["words"]), (what, "generator words", np.flatnonzero((a["words"] != b["words"]).any(axis=(1, 2))))
    for k, atol in REALS:
        if k in a:
            assert_reals(a[k], b[k], atol=atol, what=(what, k))


def as_sampled(ref):
    """the transitions of an oracle run as a one-launch `sample` call reports them: position, acceptance and divergence of
    every transition; everything else after the last one only, n_leapfrog summed"""
    out = [dict(position=r["position"], acceptance_probability=r["acceptance_probability"], is_diverging=r["is_diverging"])
           for r in ref[:-1]]
    last = dict(ref[-1])
    last["n_leapfrog"] = sum(np.asarray(r["n_leapfrog"]) for r in ref)
    return out + [last]


def assert_same_run(a, b, sampler, what=""):
    assert len(a) == len(b)
    for t in range(len(a)):
        assert_same_transition(a[t], b[t], sampler, what=(what, "transition", t))


class CallableTarget:
    """a Python log-density with its gradient by hand, as np_oracle takes a target: (U, dU/dq) = (-logp, -dlogp/dq)"""

    def __init__(self, logp, grad):
        self.logp, self.grad = logp, grad

    def __call__(self, q):
        q = np.asarray(q, dtype=np.float64)
        with np.errstate(all="ignore"):
            return -float(self.logp(q)), -np.asarray(self.grad(q), dtype=np.float64)


# ---------------------------------------------------------------------------------------------- decision margins
class Margins:
    """Records, while np_oracle runs, how far every decision was from flipping: `|delta| - thr` of every energy difference
    (hmc.py:189-191, proposals.py:41-46) relative to the energies it is the difference of, and every binomial(1, p) draw's
    uniform against its decision point.  A case is safe when each is non-finite, saturated or further than 1e-6 relative."""
    REL = 1e-6

    def __init__(self):
        self.unsafe = []
        self.n = 0

    def delta(self, H0, E, delta, thr):
        self.n += 1
        if not (np.isfinite(H0) and np.isfinite(E) and np.isfinite(delta)):
            return
        size = max(abs(H0), abs(E), 1.0)
        if np.isfinite(thr) and abs(abs(delta) - thr) <= self.REL * max(size, thr):
            self.unsafe.append(("threshold", H0, E, delta))
        # exp(delta) and expit(delta - w) of a difference of huge energies: settled only where delta is far from 0
        if size > 1e6 and abs(delta) <= self.REL * size:
            self.unsafe.append(("cancelled", H0, E, delta))

    def draw(self, gen, p):
        self.n += 1
        if not (0.0 < p < 1.0):
            return
        u = np.random.Generator(gen.bit_generator.__class__())  # a copy of the generator: the uniform the draw will use
        u.bit_generator.state = gen.bit_generator.state
        U = u.random()
        point = 1.0 - p if p <= 0.5 else p  # binomial(1, p): U <= 1 - p -> 0; p > 0.5 draws 1 - binomial(1, 1 - p)
        if abs(U - point) <= self.REL * max(point, U):
            self.unsafe.append(("draw", p, U))


def with_margins(fn):
    """Run ``fn()`` with np_oracle's `bernoulli`, `proposal_generator` and HMC energy difference observed; returns
    (fn's result, Margins)."""
    m = Margins()
    real_bern, real_gen, real_hmc = no.bernoulli, no.proposal_generator, no.hmc_kernel
    real_metric, real_verlet = no.gaussian_metric, no.velocity_verlet
    seen = {"K": [], "U": None}

    def metric(imm):
        mg, ke, turning, vel = real_metric(imm)

        def kinetic(p):
            k = ke(p)
            seen["K"].append(k)
            return k
        return mg, kinetic, turning, vel

    def verlet(target, velocity_fn):
        one = real_verlet(target, velocity_fn)

        def one_step(state, step_size):
            new = one(state, step_size)
            seen["U"] = new.potential_energy
            return new
        return one_step

    def bern(gen, p):
        m.draw(gen, float(p))
        return real_bern(gen, p)

    def gen(kinetic_energy, thr):
        upd = real_gen(kinetic_energy, thr)

        def update(initial_energy, state):
            prop, div = upd(initial_energy, state)
            with np.errstate(all="ignore"):
                m.delta(initial_energy, prop.energy, initial_energy - prop.energy, thr)
            return prop, div
        return update

    def hmc_kernel(srng, target, divergence_threshold=1000):
        step = real_hmc(srng, target, divergence_threshold)

        def observed(state, step_size, imm, L):
            seen["K"] = []
            d = step(state, step_size, imm, L)  # kinetic_energy: of the drawn momentum, then of the last one (hmc.py:186-188)
            with np.errstate(all="ignore"):
                H0, E = state.potential_energy + seen["K"][0], seen["U"] + seen["K"][1]
                m.delta(H0, E, H0 - E, divergence_threshold)
            return d
        return observed

    no.bernoulli, no.proposal_generator, no.hmc_kernel = bern, gen, hmc_kernel
    no.gaussian_metric, no.velocity_verlet = metric, verlet
    try:
        return fn(), m
    finally:
        no.bernoulli, no.proposal_generator, no.hmc_kernel = real_bern, real_gen, real_hmc
        no.gaussian_metric, no.velocity_verlet = real_metric, real_verlet


# ---------------------------------------------------------------------------------------------- 2. the wall density
# U = sum_i (q_i < w ? 0.5 q_i^2 : poison), dU/dq_i = q_i everywhere (so the dynamics are the Gaussian's and known); w and
# the poison are PARAMETERS: one compilation per kernel family serves NaN, +inf and -inf.
WALL_POISONS = {"nan": np.nan, "plus_inf": np.inf, "minus_inf": -np.inf}
# measured with np_oracle on the inputs of `wall_inputs` (tests/test_nonfinite_host.py asserts the condition they are for)
WALLS = {3: 1.9, 24: 2.6, 40: 2.8, 70: 2.9, 72: 2.9, 130: 3.0, 700: 3.4, 1500: 3.8}
HMC_WALLS = {3: 1.6, 24: 2.4, 40: 2.8, 70: 2.8, 72: 2.8, 130: 3.0, 700: 3.4, 1500: 3.5}  # (trajectories of a quarter period)
WALL_SOURCE = """
__device__ void aehmc_custom_elem(double q, long long i, const double *const *prm, double &u, double &g) {
  u = q < prm[0][0] ? 0.5 * q * q : prm[1][0];
  g = q;
}
"""


class Wall:
    """the wall density for np_oracle: U summed in coordinate order"""

    def __init__(self, w, poison):
        self.w, self.poison = float(w), float(poison)

    def __call__(self, q):
        q = np.asarray(q, dtype=np.float64)
        with np.errstate(all="ignore"):
            u = 0.0
            for x in q:
                u += 0.5 * (x * x) if x < self.w else self.poison
        return float(u), q.copy()


def wall_metric(D):
    """a unit metric; at D = 72 (the block kernels' shape) a shared dense one close to it"""
    if D != 72:
        return np.ones(D)
    B = np.random.default_rng(72).normal(size=(D, D))
    return np.eye(D) + 0.1 * (B + B.T) / np.sqrt(2 * D)


# the same wall behind a JOINT density (neighbours weakly coupled), written once for numpy and for aehmc_amd.tracing: the
# poison is ADDED outside the wall (0.5 q^2 + poison is the poison, for all three), so the gradient stays the Gaussian's
def wall_joint_logp(q, wv, pv):
    from aehmc_amd import tracing
    base = -0.5 * (q @ q) - 0.05 * np.sum(q[1:] * q[:-1])
    return base - tracing.where(q < wv[0], 0.0, pv[0]).sum()


def wall_joint_target(w, poison):
    wv, pv = np.array([float(w)]), np.array([float(poison)])

    def grad(q):
        g = -q.copy()
        g[1:] -= 0.05 * q[:-1]
        g[:-1] -= 0.05 * q[1:]
        return g
    return CallableTarget(lambda q: wall_joint_logp(q, wv, pv), grad)


JOINT_WALLS = {70: 2.9, 600: 3.6}
JOINT_HMC_WALLS = {70: 2.8, 600: 3.4}

# a GLM whose row loss is poisoned beyond z > w: Gaussian rows 0.5 (z - y)^2 inside, N(0, tau^2) prior
WALL_GLM_SOURCE = """
__device__ void aehmc_glm_row(double z, double y, long long n, const double *const *prm, double &l, double &d) {
  l = z > prm[1][0] ? prm[2][0] : 0.5 * (z - y) * (z - y);
  d = z - y;
}
__device__ void aehmc_glm_prior(double q, long long i, const double *const *prm, double &u, double &g) {
  const double tau = prm[0][0];
  u = 0.5 * q * q / (tau * tau);
  g = q / (tau * tau);
}
"""
GLM_TAU = 2.0


class WallGLM:
    def __init__(self, X, y, w, poison):
        self.X, self.y, self.w, self.poison = X, y, float(w), float(poison)

    def __call__(self, q):
        q = np.asarray(q, dtype=np.float64)
        with np.errstate(all="ignore"):
            z = self.X @ q
            loss = np.where(z > self.w, self.poison, 0.5 * (z - self.y) ** 2)
            U = float(loss.sum() + (0.5 * q * q / GLM_TAU ** 2).sum())
            g = self.X.T @ (z - self.y) + q / GLM_TAU ** 2
        return U, g


def wall_glm_inputs(N, D=10, sampler="nuts"):
    """(X, y, C, seeds, q0, imm, eps, wall): rows z = x . q of a linear model; the metric 1 / N makes the posterior's
    frequencies about 1, so the step sizes of the unit Gaussian are stable"""
    r = np.random.default_rng(N)
    X = r.normal(size=(N, D))
    y = X @ (0.3 * r.normal(size=D)) + 0.5 * r.normal(size=N)
    C = 24
    q0 = 0.3 * r.normal(size=(C, D))
    return X, y, C, list(range(5000 + N, 5000 + N + C)), q0, np.full(D, 1.0 / N), 0.25, (GLM_WALLS if sampler == "nuts" else GLM_HMC_WALLS)[N]


GLM_WALLS = {900: 3.5, 300: 3.5}   # (some chains START beyond the wall: H0 is the poison, the first leapfrog diverges)
GLM_HMC_WALLS = {900: 3.5, 300: 3.0}
GLM_L = 7


def wall_eps(D):
    return 0.25 / D ** 0.25


def wall_length(D):
    """HMC: about a quarter period of the unit Gaussian"""
    return int(round(1.6 / wall_eps(D)))


def wall_inputs(D, sampler="nuts", joint=False):
    """(C, seeds, q0, wall) of the wall case at D coordinates: q0 ~ U(-1, 1), and in the first four chains one coordinate
    a hair inside the wall, so that a first leapfrog (of the transition or of a later sub-trajectory) crosses it"""
    C = 24 if D < 1000 else 20
    w = ((JOINT_WALLS if joint else WALLS) if sampler == "nuts" else (JOINT_HMC_WALLS if joint else HMC_WALLS))[D]
    q0 = np.random.default_rng(D).uniform(-1.0, 1.0, size=(C, D))
    for c in range(4):
        q0[c, c % D] = w - 1e-4 * (c + 1)
    return C, list(range(3000 + D, 3000 + D + C)), q0, w


def wall_condition(outs, C):
    """The condition of a wall case on the ORACLE's outputs alone (a list over transitions of [C] arrays): at least four
    transitions that diverge in mid-tree, at least one that diverges on the first leapfrog or in a phantom scan, at least
    a third of the chains healthy throughout.  Returns the three counts."""
    div = np.stack([o["is_diverging"] for o in outs]).astype(bool)
    nl = np.stack([o["n_leapfrog"] for o in outs])
    deep = int((div & (nl >= 3)).sum())
    early = int(np.stack([o["first_step_divergence"] for o in outs]).sum())
    healthy = int((~div).all(axis=0).sum())
    return deep, early, healthy


def assert_wall_condition(outs, C, what=""):
    deep, early, healthy = wall_condition(outs, C)
    assert deep >= 4 and early >= 1 and 3 * healthy >= C, (what, deep, early, healthy)
