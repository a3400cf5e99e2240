"""aehmc_constrain (csrc/constrain.cuh) and what sits on it -- ``Model.constrain``, ``summary.run(constrain=...)``, a
NUTS run of a constrained model -- on the device, against the 50-digit values and allowances of tests/transforms_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import transforms_ref as tr  # noqa: E402
from transforms_ref import INTERVAL, LOWER, ORDERED, REAL, SIMPLEX, UPPER, Spec  # noqa: E402

torch = pytest.importorskip("torch")
from test_gpu_summary import RTOL, dev, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 771)
BASE = 7  # distinct rows of a case (a prime: row r of a call is base row r % 7, so a wrong row stride shows); the 50-digit
#           reference is computed once per case for these and shared by every R


def _bounds(seed, n):
    r = np.random.default_rng(seed)
    lo = r.normal(0.0, 10.0, n) * 10.0 ** r.integers(-3, 4, n)
    return lo, lo + np.exp(r.normal(0.0, 3.0, n))


def specs():
    lo10, hi10 = _bounds(1, 10)
    lo40, hi40 = _bounds(2, 40)
    lo400, hi400 = _bounds(3, 400)
    return {
        "d1": Spec([(SIMPLEX, 2, 0.0, 0.0)]),  # D_in = 1, D_out = 2
        "d65": Spec([(REAL, 3, 0.0, 0.0), (LOWER, 10, lo10, 0.0), (UPPER, 5, 0.0, 2.5), (INTERVAL, 10, lo10, hi10),
                     (ORDERED, 2, 0.0, 0.0), (SIMPLEX, 3, 0.0, 0.0), (ORDERED, 20, 0.0, 0.0), (LOWER, 1, 0.0, 0.0),
                     (INTERVAL, 1, -1.0, 1.0), (REAL, 11, 0.0, 0.0)]),
        # the Simplex(64) segment starts at input coordinate 33
        "d300": Spec([(REAL, 33, 0.0, 0.0), (SIMPLEX, 64, 0.0, 0.0), (ORDERED, 64, 0.0, 0.0), (LOWER, 50, -3.0, 0.0),
                      (INTERVAL, 40, lo40, hi40), (UPPER, 30, 0.0, 1e3), (REAL, 20, 0.0, 0.0)]),
        # the Ordered(64) ends on input coordinate 1024, the last of the row; its outputs are 962 ... 1025
        "d1025": Spec([(LOWER, 400, lo400, 0.0), (INTERVAL, 400, lo400, hi400), (SIMPLEX, 64, 0.0, 0.0), (UPPER, 98, 0.0, hi10[0]),
                       (ORDERED, 64, 0.0, 0.0)]),
        # an Ordered(64) across coordinate 1024 (the fifth workgroup of 256 outputs begins inside it)
        "straddle": Spec([(REAL, 1000, 0.0, 0.0), (ORDERED, 64, 0.0, 0.0), (LOWER, 36, 1.5, 0.0)]),
        "real": Spec([(REAL, 130, 0.0, 0.0)]),
        "simplex3": Spec([(SIMPLEX, 3, 0.0, 0.0), (REAL, 2, 0.0, 0.0), (SIMPLEX, 64, 0.0, 0.0), (SIMPLEX, 5, 0.0, 0.0)]),
    }


SPECS = specs()
_CASES = {}


def base_rows(name):
    """(x [7, D_in], want [7, D_out], allowance [7, D_out]): ordinary rows, the edge arguments, NaN and both infinities"""
    if name not in _CASES:
        spec = SPECS[name]
        r = np.random.default_rng(sum(map(ord, name)))
        D = spec.d_in
        x = np.empty((BASE, D))
        x[0] = r.normal(0.0, 1.0, D)
        x[1] = r.normal(0.0, 3.0, D)
        x[2] = np.resize([750.0, -750.0, 0.3, -750.0, -750.0], D)
        x[3] = np.resize([0.0, 1e-300, -1e-300, 40.0, -40.0, 708.0, -708.0], D)
        x[4] = r.normal(0.0, 1.0, D)
        x[4, r.integers(0, D, max(1, D // 16))] = np.nan
        x[5] = r.normal(0.0, 1.0, D)
        x[5, r.integers(0, D, max(1, D // 16))] = np.inf
        x[6] = r.uniform(-40.0, 40.0, D)
        x[6, r.integers(0, D, max(1, D // 16))] = -np.inf
        ref = [spec.reference(row) for row in x]
        _CASES[name] = (x, np.stack([w for w, _ in ref]), np.stack([a for _, a in ref]))
    return _CASES[name]


def rows(a, R):
    return a[np.arange(R) % BASE]


def check(got, want, allow, what):
    ok = tr.within(got, want, allow)
    if not ok.all():
        i = np.argwhere(~ok)[:5]
        raise AssertionError((what, [(tuple(k), got[tuple(k)], want[tuple(k)], allow[tuple(k)]) for k in i]))
    fin = np.isfinite(want) & (allow > 0)
    print(what, "largest |error| / allowance", float((np.abs(got[fin] - want[fin]) / allow[fin]).max()) if fin.any() else 0.0)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_constrain_against_50_digits(name):
    from aehmc_amd.engine import get_engine
    spec, (x, want, allow) = SPECS[name], base_rows(name)
    model = spec.model()
    assert (model.dim, model.constrained_dim) == (spec.d_in, spec.d_out)
    eng = get_engine()
    table = model._table_on(eng)
    for R in ROWS:
        xr = dev(rows(x, R))
        y = eng.constrain(xr, table, spec.d_out)
        assert tuple(y.shape) == (R, spec.d_out)
        got = y.cpu().numpy()
        check(got, rows(want, R), rows(allow, R), f"{name} R={R}")
        again = eng.constrain(xr, table, spec.d_out)
        assert same_bits(again, y)
        if R > 1:  # [R, D] as one call and as two halves, into one buffer
            out = torch.empty_like(y)
            h = R // 2
            eng.constrain(xr[:h], table, spec.d_out, out=out[:h])
            eng.constrain(xr[h:], table, spec.d_out, out=out[h:])
            assert same_bits(out, y)
        if name == "real":
            assert same_bits(y, xr)  # a copy, NaN payloads and signed infinities included
    # the model's own entry: leading axes kept
    R = 2 * 65
    y3 = model.constrain(dev(rows(x, R)).reshape(2, 65, spec.d_in))
    assert tuple(y3.shape) == (2, 65, spec.d_out) and same_bits(y3.reshape(R, -1), eng.constrain(dev(rows(x, R)), table, spec.d_out))


def test_constrain_edges_and_errors():
    """the specified edge behaviour, value by value, and what the wrapper refuses"""
    from aehmc_amd import transforms as tf
    from aehmc_amd.engine import EngineError, get_engine
    nan, inf = np.nan, np.inf
    m = tf.Model({"a": tf.LowerBound(1.0), "b": tf.UpperBound(2.0), "c": tf.Interval(0.1, 0.3), "s": tf.Simplex(3), "o": tf.Ordered(3)},
                 lambda **kw: 0.0)
    x = dev([[750.0, 750.0, 750.0, 0.0, inf, 1.0, 0.0, 750.0],
             [-750.0, -750.0, -750.0, 0.0, -inf, 1.0, nan, 0.0],
             [nan, nan, nan, nan, 0.0, 0.0, 0.0, 0.0],
             [inf, inf, inf, 750.0, -750.0, -inf, 2.0, 3.0]])
    y = m.constrain(x).cpu().numpy()
    assert y[0, :3].tolist() == [inf, -inf, 0.3] and np.isnan(y[0, 3:6]).all() and y[0, 6:].tolist() == [1.0, 2.0, inf]
    assert y[1, :3].tolist() == [1.0, 2.0, 0.1] and y[1, 4] == 0.0 and y[1, 6] == 1.0 and np.isnan(y[1, 7:]).all()
    assert abs(y[1, 3] - 0.5) <= 2.0 ** -52 and y[1, 5] == y[1, 3]  # exp(-log 2): the allowance of test_constrain_against_50_digits
    assert np.isnan(y[2, :6]).all() and y[2, 6:].tolist() == [0.0, 1.0, 2.0]
    assert y[3, :3].tolist() == [inf, -inf, 0.3] and y[3, 3:6].tolist() == [1.0, 0.0, 0.0] and y[3, 6:].tolist() == [-inf, -inf, -inf]
    eng = get_engine()
    tab = m._table_on(eng)
    with pytest.raises(ValueError, match="overlap"):
        buf = torch.zeros(4 * 9 + 8, dtype=torch.float64, device="cuda")
        eng.constrain(buf[:32].view(4, 8), tab, 9, out=buf[8:44].view(4, 9))
    with pytest.raises(EngineError, match="overlap"):  # the C entry checks on its own
        buf = torch.zeros(4 * 9 + 8, dtype=torch.float64, device="cuda")
        eng._check(eng.lib.aehmc_constrain(eng.ctx, 4, 8, 9, buf.data_ptr(), tab.data_ptr(), buf.data_ptr() + 64, eng.stream), "aehmc_constrain")
    with pytest.raises(ValueError, match="40 bytes"):
        eng.constrain(x, tab[:40], 9)
    with pytest.raises(ValueError, match="out must be"):
        m.constrain(x, out=torch.empty(4, 8, dtype=torch.float64, device="cuda"))
    # an entry that points outside the row writes NaN and reads nothing
    bad = m.table.copy()
    bad["first"][3:6] = 7  # the Simplex(3) would read inputs 7 and 8 of 8
    y = eng.constrain(x[:1], torch.from_numpy(bad.view(np.uint8).copy()).cuda(), 9).cpu().numpy()
    assert np.isnan(y[0, 3:6]).all() and y[0, 2] == 0.3


# ---- a model with known constrained marginals (the issue's): sigma ~ Gamma(3, 2), rho = 2 Beta(2, 3) - 1,
# pi ~ Dirichlet(2, 3, 4), mu = two ordered standard normals, w ~ N(0, I_3)
def marginals_logprob(sigma, rho, pi, mu, w):
    return (2.0 * np.log(sigma) - 2.0 * sigma + np.log1p(rho) + 2.0 * np.log1p(-rho) + np.sum(np.array([1.0, 2.0, 3.0]) * np.log(pi))
            - 0.5 * np.sum(mu * mu) - 0.5 * np.sum(w * w))


_MODEL = []


def marginals_model():
    from aehmc_amd import transforms as tf
    if not _MODEL:  # one instance: traced and compiled once for every test below
        _MODEL.append(tf.Model({"sigma": tf.Positive(), "rho": tf.Interval(-1.0, 1.0), "pi": tf.Simplex(3), "mu": tf.Ordered(2),
                                "w": tf.Real(3)}, marginals_logprob))
    return _MODEL[0]


EXACT_MEAN, EXACT_SQUARE = tr.EXACT_MEAN, tr.EXACT_SQUARE


def start(model, C, seed):
    r = np.random.default_rng(seed)
    return dev(r.normal(0.0, 0.5, (C, model.dim)))


def close(got, want, name):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    rel = np.abs(g - w) / np.where(w != 0, np.abs(w), 1.0)
    print(name, "max rel diff", rel.max())
    assert np.all(rel <= RTOL), (name, rel.max())


def test_run_with_constrain_equals_stored_constrained_draws():
    """summary.run(constrain=model, sketch=...) against kernel.sample on a twin kernel, model.constrain of the stored
    draws, summarize and a sketch folded from them: the run, seeds, chunk and RTOL of tests/test_gpu_summary_stream.py
    (test_run_with_max_lag_nuts: 64 chains, seeds 50 000 + c, 100 draws, chunk 37, step size 0.3, 20 lags)."""
    from aehmc_amd import RandomStream, nuts, summary
    model = marginals_model()
    C, N, L = 64, 100, 20
    state = nuts.new_state(start(model, C, 41), model)
    imm = np.ones(model.dim)
    k1, k2 = (nuts.new_kernel(RandomStream(seeds=[50_000 + c for c in range(C)]), model) for _ in range(2))
    samples, info, acc, div = k1.sample(state, 0.3, imm, N)
    theta = model.constrain(samples)
    assert tuple(theta.shape) == (N, C, model.constrained_dim)
    want = summary.summarize(theta, max_lag=L)
    grid = (torch.full((10,), -6.0, dtype=torch.float64), torch.full((10,), 6.0, dtype=torch.float64))
    sk_want = summary.QuantileSketch(C, (10,), bins=256, grid=grid).update(theta)
    sk = summary.QuantileSketch(C, (10,), bins=256, grid=grid)
    got, info2, acc2, div2 = summary.run(k2, state, 0.3, imm, N, chunk=37, max_lag=L, sketch=sk, constrain=model)
    assert tuple(got.mean.shape) == (10,)
    for f in ("mean", "sd", "rhat", "ess", "mcse", "ess_chains", "mcse_chains"):
        close(getattr(got, f), getattr(want, f), f)
    assert torch.equal(got.lag_truncated, want.lag_truncated)
    assert torch.equal(sk.counts, sk_want.counts) and sk.num_draws == N * C
    assert same_bits(sk.quantiles([0.05, 0.5, 0.95]), sk_want.quantiles([0.05, 0.5, 0.95]))
    # the chain state that comes back is the unconstrained one of the twin run
    for f in ("position", "potential_energy", "potential_energy_grad"):
        assert same_bits(getattr(info2.state, f), getattr(info.state, f)), f
    assert same_bits(acc2, acc) and torch.equal(div2, div)
    assert same_bits(model.constrain(info2.state.position), theta[-1])
    with pytest.raises(ValueError, match=r"sketch must be a QuantileSketch of 64 chains and shape \(10,\)"):
        summary.run(k2, state, 0.3, imm, N, sketch=summary.QuantileSketch(C, (9,), bins=256, grid=(-6.0, 6.0)), constrain=model)


def test_run_without_constrain_is_unchanged():
    """summary.run without ``constrain`` returns what it returned before the keyword existed.  The comparison is bitwise
    against a second call path that does not go through run's loop -- kernel.sample of a twin kernel into one buffer, cut
    into the same chunks and folded into an Accumulator and a sketch by hand, which is what run did at the parent commit
    (procedure: check the parent out, run this test's body without the `constrain=None` argument; the same assertions
    hold there) -- and with ``constrain=None`` spelled out against left out."""
    from aehmc_amd import RandomStream, nuts, summary, targets
    r = np.random.default_rng(41)
    C, D, N = 64, 10, 100
    mu, sigma = r.normal(size=D) * 2.0, 0.5 + r.random(D)
    tgt = targets.DiagGaussian(mu, sigma)
    state = nuts.new_state(dev(mu + sigma * r.normal(size=(C, D))), tgt)
    k1, k2, k3 = (nuts.new_kernel(RandomStream(seeds=[50_000 + c for c in range(C)]), tgt) for _ in range(3))
    grid = (-12.0, 12.0)
    sk2, sk3, sk_hand = (summary.QuantileSketch(C, (D,), bins=256, grid=grid) for _ in range(3))
    got = summary.run(k2, state, 0.3, sigma**2, N, chunk=37, sketch=sk2)
    spelled = summary.run(k3, state, 0.3, sigma**2, N, chunk=37, sketch=sk3, constrain=None)
    samples, info, acc, div = k1.sample(state, 0.3, sigma**2, N)
    hand = summary.Accumulator(N, C, (D,))
    for lo in range(0, N, 37):
        hand.update(samples[lo:lo + 37])
        sk_hand.update(samples[lo:lo + 37])
    want = hand.result()
    for res in (got, spelled):
        for f in ("mean", "sd", "rhat", "ess_chains", "mcse_chains"):
            assert same_bits(getattr(res[0], f), getattr(want, f)), f
        assert res[0].ess is None and same_bits(res[1].state.position, info.state.position)
        assert same_bits(res[2], acc) and torch.equal(res[3], div) and torch.equal(res[1].n_leapfrog, info.n_leapfrog)
    assert torch.equal(sk2.counts, sk_hand.counts) and torch.equal(sk3.counts, sk_hand.counts)


def test_nuts_on_a_constrained_model_recovers_the_exact_marginals():
    """NUTS, 1024 chains, 200 pooled warm-up steps, 200 draws: every constrained mean and second moment within |z| < 4 of
    its exact value with summarize's mcse_chains (the criterion of tests/test_gpu_statistics.py), rhat below 1.01, pi on
    the simplex within 4 ulp per draw, mu ordered in every draw."""
    from aehmc_amd import RandomStream, nuts, summary, window_adaptation
    model = marginals_model()
    C, N = 1024, 200
    kernel = nuts.new_kernel(RandomStream(seeds=[70_000 + c for c in range(C)]), model)
    state = nuts.new_state(start(model, C, 5), model)
    state, (step_size, imm), _ = window_adaptation.run(kernel, state, num_steps=200, pooled=True)
    samples, info, acc, div = kernel.sample(state, step_size, imm, N)
    theta = model.constrain(samples)
    s = summary.summarize(torch.cat([theta, theta * theta], dim=-1))
    mean, se, rhat = s.mean.cpu().numpy(), s.mcse_chains.cpu().numpy(), s.rhat.cpu().numpy()
    z = (mean - np.concatenate([EXACT_MEAN, EXACT_SQUARE])) / se
    p = model.unravel(theta)
    off = float((p["pi"].sum(dim=-1) - 1.0).abs().max())
    print("z", z, "rhat", rhat[:10].max(), "rhat of the squares", rhat[10:].max(), "divergent", int(div.sum()), "pi sum - 1 in ulp", off * 2.0 ** 52)
    assert np.all(np.abs(z) < 4.0), z
    assert rhat[:10].max() < 1.01
    assert off <= 4 * 2.0 ** -52
    assert bool((p["mu"][..., 0] < p["mu"][..., 1]).all())
    assert bool((p["sigma"] > 0).all()) and bool((p["rho"].abs() < 1).all())
