"""The reverse-mode programs of aehmc_amd/tracing.py on MANY lanes, on the host (tests/simt_ref.py: one std::thread per
lane, 64 or 512 of them, barriers for AEHMC_SYNC / AEHMC_WSUM, std::atomic_ref for AEHMC_ATOMIC_ADD).  What makes a
program right on many lanes -- which lane owns a gradient entry, which additions are atomic, where a barrier separates a
write from another lane's read -- is invisible to tests/test_tracing.py, which runs every program on one lane.

Per model and lane count: the plain build against the one-lane run of the same program and against central differences
of the Python function; the -fsanitize=thread build for zero reports.  A race loses an update once in many runs, so a
comparison of values does not see it; the sanitizer sees the missing order itself, in every run.  (The sanitizer is on a
stand-alone host program; nothing here needs a GPU.)"""
import re

import numpy as np
import pytest

import simt_ref
from test_tracing import CASES, random_density, random_shared_density
from aehmc_amd import tracing

LANES = (64, 512)
SIZES = (63, 64, 65, 511, 512, 513, 600)  # loop iterations: a lane short of one pass, one pass, one more, at both lane counts; and 600


# ---- index-map mixtures over ONE position vector: n = the iterations of the loop that mixes them
def gather_direct(n, r):
    G = r.integers(0, n, size=n)
    return n, lambda q: -0.5 * np.sum((q[G] - q) ** 2) - 0.5 * q @ q


def two_gathers(n, r):
    G1, G2, w = r.integers(0, n, size=n), r.integers(0, n, size=n), 0.5 + r.random(n)
    return n, lambda q: -0.5 * np.sum(w * (q[G1] - q[G2]) ** 2) - 0.5 * q @ q


def gather_shifted(n, r):
    G = r.integers(0, n + 1, size=n)
    return n + 1, lambda q: -0.5 * np.sum((q[G] - q[1:]) ** 2) - 0.5 * q @ q


def gather_centred(n, r):
    G, y = r.integers(0, n, size=n), r.normal(size=n)
    return n, lambda q: -0.5 * np.sum((y - q[G] + q.mean()) ** 2) - 0.5 * q @ q


def reversed_strided(n, r):  # (the strided loop runs n iterations, the reversed one 2 n)
    return 2 * n, lambda q: 0.3 * np.sum(q[::-1] * q) - 0.5 * np.sum((q[1::2] - q[::2]) ** 2) - 0.5 * q @ q


def second_differences(n, r):
    return n + 2, lambda q: -0.5 * np.sum((q[2:] - 2 * q[1:-1] + q[:-2]) ** 2) - 0.5 * q @ q


def normal_equations(n, r):
    # (the tracer does not spread this one: EVERY lane runs the n x n double loop whole and lane 0 alone adds into g, between
    # the prior's distributed loops -- 512 sanitized lanes of it are this module's longest runs, hence the single row)
    A = r.normal(size=(1, n)) / np.sqrt(n)
    return n, lambda q: -0.5 * (q @ (A.T @ (A @ q))) - 0.5 * q @ q


def softmax_normaliser(n, r):
    w = r.normal(size=n)
    return n, lambda q: np.sum(w * (np.exp(q) / np.exp(q).sum())) - 0.5 * q @ q


MIXTURES = {f.__name__: f for f in (gather_direct, two_gathers, gather_shifted, gather_centred, reversed_strided, second_differences,
                                    normal_equations, softmax_normaliser)}
# test_tracing's seeds and sizes, thinned to what the module's time allows: between them every term of random_density and of
# random_shared_density, the long sizes first (D = 70: 67 iterations, a second pass on 64 lanes)
RANDOM = ((5, 70), (8, 70), (10, 17), (12, 9))   # (seed, D = [9, 17, 70][seed % 3]): terms 4 2 1 6 / 4 5 7 3 / 6 2 5 4 / 8 7 7 5
RANDOM_SHARED = ((1, 70), (3, 70), (7, 17))      # terms 4 6 0 / 1 3 2 / 3 5 6


def model(name):
    """-> (the Python density, its dimension, a position)"""
    kind, _, rest = name.partition(":")
    if kind == "case":
        fn, D, _ = CASES[rest]
        return fn, D, 0.7 * np.random.default_rng(0).normal(size=D)   # (test_tracing's first trial)
    if kind == "mix":
        what, n = rest.split(":")
        r = np.random.default_rng(int(n) + sum(map(ord, what)))
        D, fn = MIXTURES[what](int(n), r)
        return fn, D, 0.6 * r.normal(size=D)
    seed, D = map(int, rest.split(":"))
    fn = (random_density if kind == "random" else random_shared_density)(seed, D)
    return fn, D, 0.6 * np.random.default_rng(100 + seed).normal(size=D)


MODELS = ([f"case:{name}" for name in sorted(CASES) if not CASES[name][2]]
          + [f"mix:{what}:{n}" for what in MIXTURES for n in SIZES]
          + [f"random:{seed}:{D}" for seed, D in RANDOM] + [f"shared:{seed}:{D}" for seed, D in RANDOM_SHARED])


def central_differences(fn, q, h=1e-6):
    """of the Python function, in extended precision where numpy has it and the density takes it (the rounding of a
    float64 difference quotient, ~ 1e-16 |f| / h, is what the tolerance below would otherwise go to at 600 coordinates)"""
    def grad(x):
        out = np.empty(len(x), dtype=x.dtype)
        for i in range(len(x)):
            e = np.zeros_like(x)
            e[i] = h
            out[i] = (fn(x + e) - fn(x - e)) / (2 * h)
        return out.astype(np.float64)
    try:
        return grad(q.astype(np.longdouble))
    except TypeError:  # (a scipy.special function in the density)
        return grad(q)


class Programs:
    """every model traced, built (plain and sanitized side by side) and run (every lane count of both builds together) ONCE
    for all its parametrisations: the tests below only look at what came out"""

    def __init__(self, directory, tsan):
        self.dir, self.tsan, self.models = directory, tsan, {}

    def get(self, name):
        if name not in self.models:
            fn, D, q = model(name)
            tr = tracing.trace(fn, D, reverse=True)
            assert not tr.elementwise and "aehmc_logp_grad" in tr.grad_source
            exes = simt_ref.build(tr, q, self.dir, f"m{len(self.models)}", tsan=(False, True) if self.tsan else (False,))
            jobs = [(exe, lanes) for exe in exes[1:] for lanes in LANES] + [(exes[0], lanes) for lanes in (1,) + LANES + LANES]
            out = simt_ref.run(jobs)  # (the sanitized runs, the long ones, first)
            tsan, out = out[:-1 - 2 * len(LANES)], out[-1 - 2 * len(LANES):]
            self.models[name] = dict(fn=fn, q=q, tr=tr, fd=central_differences(fn, q), one_lane=simt_ref.value_and_gradient(out[0]),
                                     plain=dict(zip(LANES, out[1:1 + len(LANES)])), again=dict(zip(LANES, out[1 + len(LANES):])),
                                     tsan=dict(zip(LANES, tsan)))
        return self.models[name]


@pytest.fixture(scope="module")
def tsan_unavailable(tmp_path_factory):
    return simt_ref.tsan_probe(tmp_path_factory.mktemp("tsan_probe"))


@pytest.fixture(scope="module")
def programs(tmp_path_factory, tsan_unavailable):
    return Programs(tmp_path_factory.mktemp("lanes"), not tsan_unavailable)


def has_atomics(tr):
    return "AEHMC_ATOMIC_ADD(&" in tr.grad_source


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", MODELS)
def test_many_lanes_equal_one_lane_and_central_differences(name, lanes, programs):
    m = programs.get(name)
    v1, g1 = m["one_lane"]
    assert v1 == pytest.approx(float(m["fn"](m["q"])), rel=1e-12, abs=1e-12)
    v, g = simt_ref.value_and_gradient(m["plain"][lanes])
    assert v == pytest.approx(v1, rel=1e-14, abs=1e-14)    # (only the order of the sums differs)
    np.testing.assert_allclose(g, g1, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(g, m["fd"], rtol=2e-7, atol=2e-8)
    np.testing.assert_allclose(g1, m["fd"], rtol=2e-7, atol=2e-8)
    v2, g2 = simt_ref.value_and_gradient(m["again"][lanes])
    if not has_atomics(m["tr"]):  # every sum's order is fixed: the same bits in every run
        assert v2 == v and np.array_equal(g2, g)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", MODELS)
def test_thread_sanitizer_reports_nothing_on_many_lanes(name, lanes, programs, tsan_unavailable):
    """gather_direct is what _mixed_owners missed: AEHMC_ATOMIC_ADD(&g[G[i]], ...) of one lane against the plain
    g[i] += ... of the lane that owns i, with no barrier between them -- reported at both lane counts before a gather
    counted as an index map of its own"""
    if tsan_unavailable:
        pytest.skip(tsan_unavailable)
    code, out, err = programs.get(name)["tsan"][lanes]
    assert "ThreadSanitizer" not in err and code == 0, (code, err[:6000])
    assert len(out.split()) == 1 + len(programs.get(name)["q"])


def test_the_mixture_loops_are_spread_over_the_lanes_and_straddle_the_lane_counts():
    """what the sizes are for: each mixture has a loop of the stated iterations that runs on the lanes, not on lane 0 alone
    (normal_equations: the prior's, beside the products that every lane runs whole)"""
    for what in MIXTURES:
        for n in SIZES:
            fn, D, _ = model(f"mix:{what}:{n}")
            src = tracing.trace(fn, D, reverse=True).grad_source
            assert re.search(rf"= lane; i\d+ < {n}; i\d+ \+= AEHMC_LANES", src), (what, n)
    assert has_atomics(tracing.trace(model("mix:gather_direct:65")[0], 65, reverse=True))
    assert "g[i0] +=" not in tracing.trace(model("mix:gather_direct:65")[0], 65, reverse=True).grad_source
