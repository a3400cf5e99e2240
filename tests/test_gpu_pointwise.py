"""Traced pointwise log-likelihoods and the streaming WAIC on the device (csrc/pointwise.cuh; summary.Pointwise /
WaicAccumulator / run(waic=); transforms.Model.pointwise): against the host-compiled source and 50-digit values of
tests/test_pointwise_host.py, the numpy restatement of tests/waic_ref.py and summary.waic / summary.loo of stored arrays.
Shapes sit at the kernel's edges: entries 1 / tile - 1 / tile + 1 (tile 256), rows 1 / batch - 1 / batch + 1 /
2 parts + 3 (batch 32, part 256), positions of 1 / 6 / 65 coordinates staged in LDS and 9000 read from global memory."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_pointwise_host as ph  # noqa: E402
import waic_ref as wr  # noqa: E402
from test_waic_stream_host import SIZES, columns  # noqa: E402

torch = pytest.importorskip("torch")
from test_gpu_summary import dev, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
TILE, BATCH, PART = 256, 32, wr.PART
ROWS = (1, BATCH - 1, BATCH + 1, 2 * PART + 3)


# ---------------------------------------------------------------------------------------------- 1. evaluate
@pytest.mark.parametrize("name", sorted(ph.CASES))
def test_evaluate_against_the_host_build_and_50_digits(name, tmp_path):
    from aehmc_amd import summary
    fn, dim, ref, n_out = ph.CASES[name]
    pw = summary.Pointwise(fn, dim)
    assert (pw.dim, pw.n_out) == (dim, n_out)
    q = 0.7 * np.random.default_rng(5).normal(size=(3, dim))
    host, _ = ph.run_pointwise_cpp(pw._traced, q, tmp_path, name)
    got = pw(dev(q)).cpu().numpy()
    assert got.shape == (3, n_out)
    mp = ph._mp()
    for r in range(3):
        rows = ref(mp, q[r])
        want, allow = np.array([float(v) for v, _ in rows]), ph.allowance(rows)
        print(name, r, "device error / allowance", (np.abs(got[r] - want) / allow).max(), "device - host / allowance",
              (np.abs(got[r] - host[r]) / allow).max())
        assert np.all(np.abs(got[r] - want) <= allow) and np.all(np.abs(got[r] - host[r]) <= allow)
    lead = pw(dev(np.stack([q, q]).reshape(2, 3, dim)))  # [..., dim] -> [..., n_out]
    assert tuple(lead.shape) == (2, 3, n_out) and same_bits(lead[1], pw(dev(q)))


_MODEL = []


def mixed():
    if not _MODEL:  # (one instance: traced and compiled once)
        model = ph.mixed_model()
        _MODEL.append((model, model.pointwise(ph.model_loglik)))
    return _MODEL[0]


def test_model_pointwise_against_50_digits_and_torch(tmp_path):
    model, pw = mixed()
    q = 0.7 * np.random.default_rng(6).normal(size=(BATCH + 1, model.dim))
    got = pw(dev(q))
    theta = model.constrain(dev(q))
    un = model.unravel(theta)
    Xd, Yd, Zd = dev(ph.X), dev(ph.Y), dev(ph.Z)
    as_torch = (-0.5 * ((Yd - un["w"] @ Xd.T) / un["sigma"][:, None]) ** 2 - torch.log(un["sigma"])[:, None] - ph.HALF_LOG_2PI
                + torch.log(un["pi"]) @ Zd.T)
    mp = ph._mp()
    th = theta.cpu().numpy()
    for r in (0, BATCH):
        rows = ph.model_mp(mp, th[r])
        want, allow = np.array([float(v) for v, _ in rows]), ph.allowance(rows)
        g = got[r].cpu().numpy()
        print("model row", r, "device error / allowance", (np.abs(g - want) / allow).max())
        assert np.all(np.abs(g - want) <= allow)
        assert np.all(np.abs(as_torch[r].cpu().numpy() - g) <= 2 * allow)  # (both within the allowance of the exact value)


# programs at the kernel's edges: (fn, dim, n_out, torch expression of rows [R, dim], A [R, n_out], roundings N)
def _edge(name):
    r = np.random.default_rng(sum(map(ord, name)))
    if name == "d1":
        return (lambda q: -0.5 * q[0] * q[0] + 1.5 * q[0], 1, 1, lambda x: -0.5 * x * x + 1.5 * x, lambda x: 0.5 * x * x + 1.5 * x.abs(), 8)
    if name == "d65":
        A, y = r.normal(size=(TILE - 1, 65)) / 8.0, r.normal(size=TILE - 1)
        Ad, yd = dev(A), dev(y)
        return (lambda q: -0.5 * (y - A @ q) ** 2, 65, TILE - 1, lambda x: -0.5 * (yd - x @ Ad.T) ** 2,
                lambda x: 0.5 * (yd.abs() + x.abs() @ Ad.abs().T) ** 2, 2 * (2 * 65 + 1) + 2)
    if name == "d6":
        X, y = r.normal(size=(TILE + 1, 5)), r.normal(size=TILE + 1)
        Xd, yd = dev(X), dev(y)

        def fn(q):
            w, sigma = q[:5], np.exp(q[5])
            return -0.5 * ((y - X @ w) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2 * np.pi)

        def ref(x):
            s = torch.exp(x[:, 5:6])
            return -0.5 * ((yd - x[:, :5] @ Xd.T) / s) ** 2 - torch.log(s) - ph.HALF_LOG_2PI

        def mag(x):
            s = torch.exp(x[:, 5:6])
            return 0.5 * ((yd.abs() + x[:, :5].abs() @ Xd.abs().T) / s) ** 2 + torch.log(s).abs() + ph.HALF_LOG_2PI
        return fn, 6, TILE + 1, ref, mag, ph.N_ROUNDINGS
    assert name == "d9000"  # three slices of a row too long for LDS: read from global memory
    return (lambda q: [q[:3000].sum(), (q[3000:6000] ** 2).sum(), np.exp(q[8999]) * q[0]], 9000, 3,
            lambda x: torch.stack([x[:, :3000].sum(1), (x[:, 3000:6000] ** 2).sum(1), torch.exp(x[:, 8999]) * x[:, 0]], dim=1),
            lambda x: torch.stack([x[:, :3000].abs().sum(1), (x[:, 3000:6000] ** 2).sum(1), (torch.exp(x[:, 8999]) * x[:, 0]).abs()], dim=1),
            3000 + 8)


_EDGE = {}


def edge(name):
    if name not in _EDGE:
        from aehmc_amd import summary
        fn, dim, n_out, ref, mag, n = _edge(name)
        pw = summary.Pointwise(fn, dim)
        assert (pw.dim, pw.n_out) == (dim, n_out)
        _EDGE[name] = (pw, ref, mag, n)
    return _EDGE[name]


def edge_rows(name, R):
    pw = edge(name)[0]
    return dev(0.7 * np.random.default_rng(R).normal(size=(R, pw.dim)))


@pytest.mark.parametrize("name", ["d1", "d6", "d65", "d9000"])
def test_evaluate_at_the_edges_of_the_kernel(name):
    """every row count against the same expression in torch: both lie within N U A of the exact value (N roundings, A the
    sum of the absolute addends, as in tests/test_pointwise_host.py), so they differ by 2 N U A at most"""
    pw, ref, mag, n = edge(name)
    for R in ROWS:
        x = edge_rows(name, R)
        got, want, allow = pw(x), ref(x).reshape(R, pw.n_out), 2 * n * U * mag(x).reshape(R, pw.n_out)
        assert tuple(got.shape) == (R, pw.n_out)
        ratio = ((got - want).abs() / allow).max().item()
        print(name, R, "|device - torch| / allowance", ratio)
        assert ratio <= 1.0
        if R > 1:  # a row's values do not depend on its neighbours or on the call's geometry
            assert same_bits(pw(x[R // 2:].contiguous()), got[R // 2:])


# ---------------------------------------------------------------------------------------------- 2. fold from stored values
def ref_fold(x, cut):
    f = wr.Fold(x.shape[1])
    for r0 in range(0, x.shape[0], cut):
        f.update(x[r0:r0 + cut])
    return f


@pytest.mark.parametrize("cut", [7, None], ids=["cut7", "whole"])
@pytest.mark.parametrize("S", SIZES)
def test_stored_fold_against_the_restatement_and_waic(S, cut):
    from aehmc_amd import summary
    r = np.random.default_rng(S)
    x = np.concatenate([columns(S), -2.0 + r.normal(size=(S, TILE + 1 - 7))], axis=1)  # tile + 1 observations; 4 ... 6 non-finite
    n_obs, step = x.shape[1], S if cut is None else cut
    acc = summary.WaicAccumulator(n_obs)
    for r0 in range(0, S, step):
        acc.update_log_lik(dev(x[r0:r0 + step]))
    assert acc.n_samples == S
    ref = ref_fold(x, step)
    m, s, mean, m2 = (v.cpu().numpy() for v in acc.state)
    assert np.array_equal(m, ref.state[0])
    assert np.array_equal(mean.view(np.int64), ref.state[2].view(np.int64))  # + - * / alone: the same bits
    assert np.array_equal(m2.view(np.int64), ref.state[3].view(np.int64))
    ok = ~np.isnan(ref.state[1])
    assert np.array_equal(np.isnan(s), ~ok) and np.all(np.abs(s[ok] - ref.state[1][ok]) <= 4 * (S + 64) * U * ref.state[1][ok])
    got, want = acc.result(), summary.waic(dev(x).reshape(S, 1, n_obs))
    lppd, p, kappa = wr.exact(x[:, :8])
    fin = np.array([0, 1, 2, 3, 7])
    tol_lppd, tol_p = wr.allowances(S, p[fin], kappa[fin])
    g_l, g_p = got.lppd_i.cpu().numpy(), got.p_i.cpu().numpy()
    w_l, w_p = want.lppd_i.reshape(-1).cpu().numpy(), want.p_i.reshape(-1).cpu().numpy()
    print(f"S={S} cut={cut} fold error / allowance: lppd", (np.abs(g_l[fin] - lppd[fin]) / tol_lppd).max(), "p",
          (np.abs(g_p[fin] - p[fin]) / tol_p).max(), "| fold - summary.waic | / 2 allowances: lppd",
          (np.abs(g_l[fin] - w_l[fin]) / (2 * tol_lppd)).max(), "p", (np.abs(g_p[fin] - w_p[fin]) / (2 * tol_p)).max())
    assert np.all(np.abs(g_l[fin] - lppd[fin]) <= tol_lppd) and np.all(np.abs(g_p[fin] - p[fin]) <= tol_p)
    assert np.all(np.abs(g_l[fin] - w_l[fin]) <= 2 * tol_lppd) and np.all(np.abs(g_p[fin] - w_p[fin]) <= 2 * tol_p)
    # non-finite columns as summary.waic has them; the well-scaled neighbours (7 ...) to the project's tolerance
    for col in (4, 5, 6):
        assert np.isnan(g_p[col]) and np.isnan(w_p[col]) and np.isnan(g_l[col]) == np.isnan(w_l[col])
    np.testing.assert_allclose(g_l[[4, 5]], w_l[[4, 5]], rtol=0, atol=8 * (S + 64) * U)
    np.testing.assert_allclose(g_l[7:], w_l[7:], rtol=0, atol=8 * (S + 64) * U)
    np.testing.assert_allclose(g_p[7:], w_p[7:], rtol=1e-12)
    assert tuple(got.elpd_i.shape) == (n_obs,) and np.isnan(got.elpd)  # (an observation with a NaN: the sum says so, as waic's)


def test_merge_and_argument_checks():
    from aehmc_amd import summary
    S = SIZES[-1]
    x = columns(S)[:, :4]
    whole = summary.WaicAccumulator(4).update_log_lik(dev(x))
    a = summary.WaicAccumulator(4).update_log_lik(dev(x[:3 * PART]))
    b = summary.WaicAccumulator(4).update_log_lik(dev(x[3 * PART:]))
    assert a.merge(b).n_samples == S and same_bits(a.state, whole.state)  # (the tail is one part: the merge the fold did)
    with pytest.raises(ValueError, match="update_log_lik"):
        summary.WaicAccumulator(4).update(dev(x))
    with pytest.raises(ValueError, match="no draw"):
        summary.WaicAccumulator(4).result()
    with pytest.raises(ValueError, match=r"\[\.\.\., 4\]"):
        whole.update_log_lik(dev(x[:, :3]))
    with pytest.raises(ValueError, match="merge takes"):
        whole.merge(summary.WaicAccumulator(5))


# ---------------------------------------------------------------------------------------------- 3. fused fold
@pytest.mark.parametrize("name", ["d1", "d6", "d65", "d9000", "model"])
def test_fused_fold_is_the_stored_fold_of_the_evaluated_rows(name):
    from aehmc_amd import summary
    pw = mixed()[1] if name == "model" else edge(name)[0]
    for R in ROWS:
        x = dev(0.7 * np.random.default_rng(R).normal(size=(R, pw.dim)))
        fused, again, stored = (summary.WaicAccumulator(pw) for _ in range(3))
        fused.update(x)
        again.update(x)
        stored.update_log_lik(pw(x))
        assert fused.n_samples == stored.n_samples == R
        assert same_bits(fused.state, stored.state), (name, R)  # the same arithmetic in the same order
        assert same_bits(fused.state, again.state), (name, R)
    fused.update(x[:BATCH + 1].reshape(1, BATCH + 1, pw.dim))  # [T, C, dim]; a second fold goes behind the first
    stored.update_log_lik(pw(x[:BATCH + 1]))
    assert fused.n_samples == ROWS[-1] + BATCH + 1 and same_bits(fused.state, stored.state)


# ---------------------------------------------------------------------------------------------- 4. summary.run(..., waic=)
N_DATA = 50
EXACT_COLS = 6
_REG = []
_RUN = {}


def regression_model():
    if not _REG:
        from aehmc_amd import transforms as tf
        r = np.random.default_rng(3)
        X = r.normal(size=(N_DATA, 5))
        y = X @ r.normal(size=5) + 0.7 * r.normal(size=N_DATA)

        def logprob(w, sigma):
            return (np.sum(-0.5 * ((y - X @ w) / sigma) ** 2 - np.log(sigma)) - 0.5 * np.sum(w * w) / 25.0 - sigma)
        model = tf.Model({"w": tf.Real(5), "sigma": tf.Positive()}, logprob)
        loglik = model.pointwise(lambda w, sigma: -0.5 * ((y - X @ w) / sigma) ** 2 - np.log(sigma) - 0.5 * np.log(2 * np.pi))
        _REG.append((model, loglik))
    return _REG[0]


@pytest.mark.parametrize("constrained", [True, False], ids=["constrain", "plain"])
def test_run_with_waic(constrained):
    from aehmc_amd import RandomStream, nuts, summary
    model, loglik = regression_model()
    C, N = 64, 40
    state = nuts.new_state(dev(np.random.default_rng(8).normal(0.0, 0.3, (C, model.dim))), model)
    imm, kw = np.ones(model.dim), ({"constrain": model} if constrained else {})
    kernels = [nuts.new_kernel(RandomStream(seeds=[70_000 + c for c in range(C)]), model, max_num_expansions=5) for _ in range(4)]
    samples, info, acc_hist, div = kernels[0].sample(state, 0.05, imm, N)
    log_lik = loglik(samples)
    assert tuple(log_lik.shape) == (N, C, N_DATA)
    want = summary.waic(log_lik)
    plain = summary.run(kernels[1], state, 0.05, imm, N, chunk=7, **kw)
    x = log_lik.reshape(N * C, N_DATA).cpu().numpy()
    if "exact" not in _RUN:  # (both cases draw the same samples; 50 digits for the first observations, once)
        _RUN["exact"] = wr.exact(x[:, :EXACT_COLS])
    lppd, p, kappa = _RUN["exact"]
    tol_lppd, tol_p = wr.allowances(N * C, p, kappa)
    var = x.var(axis=0, ddof=1)  # (every observation against summary.waic: the allowance from the fp64 moments)
    _, tol_p_all = wr.allowances(N * C, var, np.sqrt(1.0 + x.mean(axis=0) ** 2 / var))
    for kern, chunk in ((kernels[2], 7), (kernels[3], 40)):
        acc = summary.WaicAccumulator(loglik)
        got = summary.run(kern, state, 0.05, imm, N, chunk=chunk, waic=acc, **kw)
        assert acc.n_samples == N * C
        if chunk == 7:  # run's own four return values: those of a call without waic=
            for f in ("mean", "sd", "rhat", "ess_chains", "mcse_chains"):
                assert same_bits(getattr(got[0], f), getattr(plain[0], f)), f
            assert same_bits(got[1].state.position, plain[1].state.position) and torch.equal(got[1].n_leapfrog, plain[1].n_leapfrog)
            assert same_bits(got[2], plain[2]) and torch.equal(got[3], plain[3])
            assert same_bits(got[1].state.position, info.state.position) and same_bits(got[2], acc_hist)
        # the state is the restatement's fold of the stored array cut as the run cut it: mean and M2 to the bit
        ref = ref_fold(x, chunk * C)
        assert np.array_equal(acc.state[0].cpu().numpy(), ref.state[0])
        for k in (2, 3):
            assert np.array_equal(acc.state[k].cpu().numpy().view(np.int64), ref.state[k].view(np.int64)), (chunk, k)
        res = acc.result()
        all_l, all_p = res.lppd_i.cpu().numpy(), res.p_i.cpu().numpy()
        g_l, g_p = all_l[:EXACT_COLS], all_p[:EXACT_COLS]
        print(f"run chunk={chunk} constrain={constrained}: fold error / allowance lppd", (np.abs(g_l - lppd) / tol_lppd).max(), "p",
              (np.abs(g_p - p) / tol_p).max())
        assert np.all(np.abs(g_l - lppd) <= tol_lppd) and np.all(np.abs(g_p - p) <= tol_p)
        assert np.all(np.abs(all_l - want.lppd_i.cpu().numpy()) <= 2 * tol_lppd) and np.all(np.abs(all_p - want.p_i.cpu().numpy()) <= 2 * tol_p_all)
        assert abs(res.elpd - want.elpd) <= 2 * (tol_lppd * N_DATA + tol_p_all.sum()) and abs(res.p - want.p) <= 2 * tol_p_all.sum()
    other = summary.Pointwise(lambda q: q[:3] * 2.0, 3)
    with pytest.raises(ValueError, match="positions of 3 coordinates"):
        summary.run(kernels[1], state, 0.05, imm, N, waic=summary.WaicAccumulator(other))
    with pytest.raises(ValueError, match="built from a Pointwise"):
        summary.run(kernels[1], state, 0.05, imm, N, waic=summary.WaicAccumulator(N_DATA))


# ---------------------------------------------------------------------------------------------- 5. the target's binding
def test_the_samplers_target_survives_pointwise_binds():
    from aehmc_amd import RandomStream, nuts, summary
    from aehmc_amd.engine import EngineError, get_engine
    model, loglik = regression_model()
    C = 16
    state = nuts.new_state(dev(np.random.default_rng(9).normal(0.0, 0.3, (C, model.dim))), model)
    step = lambda: nuts.new_kernel(RandomStream(seeds=list(range(C))), model, max_num_expansions=5)(state, 0.05, np.ones(model.dim))[0]  # noqa: E731
    before = step()
    x = dev(np.random.default_rng(10).normal(0.0, 0.3, (BATCH + 1, model.dim)))
    good = loglik(x)
    after_bind = step()
    bad = summary.Pointwise(lambda q: q[:3] * 2.0, model.dim)
    bad._traced.source += "\nthis is not HIP;\n"
    eng = get_engine()
    with pytest.raises(EngineError, match="compilation failed"):
        eng.set_pointwise(bad, bad._traced)
    with pytest.raises(EngineError, match="compilation failed"):
        bad(x)
    assert eng._keep["pointwise"][0] is loglik and same_bits(loglik(x), good)  # the previous program is still the one bound
    after_failure = step()
    for f in ("position", "potential_energy", "potential_energy_grad"):
        assert same_bits(getattr(after_bind.state, f), getattr(before.state, f)), f
        assert same_bits(getattr(after_failure.state, f), getattr(before.state, f)), f
    assert torch.equal(after_failure.n_leapfrog, before.n_leapfrog)


def test_pointwise_programs_are_kept_on_disk_across_processes(tmp_path):
    """a second process evaluates and folds the same program without compiling: the library's own count
    (aehmc_rtc_stats), not a time"""
    prog = r"""
import sys, json
sys.path.insert(0, %r)
import numpy as np, torch
from aehmc_amd import summary
from aehmc_amd.engine import get_engine
y = np.linspace(-1.0, 1.0, 40)
pw = summary.Pointwise(lambda q: -0.5 * ((y - q[0]) / np.exp(q[1])) ** 2 - q[1], 2)
x = torch.as_tensor(np.linspace(-0.5, 0.5, 66).reshape(33, 2), device="cuda")
acc = summary.WaicAccumulator(pw).update(x)
torch.cuda.synchronize()
print(json.dumps({"rtc": list(get_engine().rtc_stats()), "v": pw(x).cpu().numpy().tolist(), "s": acc.state.cpu().numpy().tolist()}))
""" % (ROOT,)
    env = dict(os.environ, AEHMC_AMD_RTC_CACHE=str(tmp_path))
    runs = []
    for _ in range(2):
        out = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        runs.append(json.loads(out.stdout.strip().splitlines()[-1]))
    assert runs[0]["rtc"][0] >= 2 and runs[0]["rtc"][1] == 0  # (the evaluate and the fold program, compiled)
    assert runs[1]["rtc"] == [0, runs[0]["rtc"][0]]             # (both from the cache)
    assert runs[0]["v"] == runs[1]["v"] and runs[0]["s"] == runs[1]["s"]


# ---------------------------------------------------------------------------------------------- 6. loo of the kernel's array
def test_loo_of_the_evaluated_array():
    """summary.loo(pw(samples)) against loo of the array formed with torch: the two arrays differ by 2 N U A per entry
    (test 1's allowance on both sides); elpd_i is a weighted log-mean-exp of a column, so it moves by no more than the
    column's largest difference, up to the change of the smoothed weights, which is of the same order: 64 times that."""
    from aehmc_amd import summary
    model, loglik = regression_model()
    N, C = 25, 16
    r = np.random.default_rng(12)
    samples = dev(np.concatenate([0.3 * r.normal(size=(N, C, 5)), -0.2 + 0.1 * r.normal(size=(N, C, 1))], axis=2))
    got_arr = loglik(samples)
    un = model.unravel(model.constrain(samples))
    X, y = (dev(a) for a in _regression_data())
    want_arr = -0.5 * ((y - un["w"] @ X.T) / un["sigma"][..., None]) ** 2 - torch.log(un["sigma"])[..., None] - ph.HALF_LOG_2PI
    A = 0.5 * ((y.abs() + un["w"].abs() @ X.abs().T) / un["sigma"][..., None]) ** 2 + torch.log(un["sigma"]).abs()[..., None] + ph.HALF_LOG_2PI
    allow = 2 * ph.N_ROUNDINGS * U * A
    assert bool(((got_arr - want_arr).abs() <= allow).all())
    got, want = summary.loo(got_arr.contiguous(), reff=1.0), summary.loo(want_arr.contiguous(), reff=1.0)
    tol = 64 * allow.reshape(N * C, N_DATA).amax(dim=0)
    diff = (got.elpd_i - want.elpd_i).abs()
    print("loo: |elpd_i difference| / allowance", (diff / tol).max().item(), "rtol", (tol / want.elpd_i.abs()).max().item())
    assert bool((diff <= tol).all()) and torch.equal(got.tail_len, want.tail_len)
    assert bool(((got.pareto_k - want.pareto_k).abs() <= 1e-9).all())


def _regression_data():
    r = np.random.default_rng(3)  # (the draws of regression_model, in its order)
    X = r.normal(size=(N_DATA, 5))
    return X, X @ r.normal(size=5) + 0.7 * r.normal(size=N_DATA)
