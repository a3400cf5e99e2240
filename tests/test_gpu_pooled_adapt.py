"""Pooled window adaptation on the GPU: the symmetric rank-C update alone, the pooled update with fed inputs against the
numpy restatement (tests/pooled_adapt_ref.py) and np.cov, the fused loop against the step-by-step one, end to end against
the oracle's NUTS kernel, and the covariance it recovers."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pooled_adapt_ref as pr  # noqa: E402

from oracle import c_oracle as co  # noqa: E402

LD = np.longdouble
U53 = 2.0 ** -53


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _syrk_case(eng, C, D, seed):
    r = np.random.default_rng(seed)
    X = r.normal(size=(C, D)) * (1 + r.random(D)) + r.normal(size=D)
    centre, delta, w = r.normal(size=D), r.normal(size=D), float(3 * r.random())
    S_in = r.normal(size=(D, D))
    got = eng.syrk_tn(_dev(X), _dev(S_in), _dev(centre), w, _dev(delta))
    again = eng.syrk_tn(_dev(X), _dev(S_in), _dev(centre), w, _dev(delta))
    Xc = X - centre  # fp64: the same single rounding as on the device
    ref = S_in.astype(LD) + Xc.astype(LD).T @ Xc.astype(LD) + LD(w) * np.outer(delta.astype(LD), delta.astype(LD))
    bound = (C + 8) * U53 * (np.abs(S_in) + np.abs(Xc).T @ np.abs(Xc) + np.abs(w * np.outer(delta, delta)))
    low = np.tril(np.ones((D, D), dtype=bool))
    err = np.abs(got.cpu().numpy().astype(LD) - ref).astype(np.float64)
    print(f"syrk C={C} D={D}: max err / bound = {(err[low] / bound[low]).max():.3g}")
    assert (err[low] <= bound[low]).all(), (C, D, (err[low] / bound[low]).max())
    assert torch.equal(torch.tril(got), torch.tril(again)), (C, D)
    plain = eng.syrk_tn(_dev(X), _dev(S_in))
    zeros = eng.syrk_tn(_dev(X), _dev(S_in), _dev(np.zeros(D)), w, _dev(np.zeros(D)))
    assert torch.equal(torch.tril(plain), torch.tril(zeros)), (C, D)


@pytest.mark.parametrize("D", [1, 15, 16, 17, 64, 65, 130, 257])
def test_syrk_tn_against_longdouble(D):
    """S += Xc^T Xc + w d d^T on the lower triangle, K tails (C % 16), partial and diagonal / off-diagonal tiles, against
    products and sums in longdouble under the running-sum bound (C + 8) 2^-53 (|S_in| + |Xc|^T |Xc| + |w d d^T|); a
    second call is bit-equal; NULL centre / delta equal zeros."""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    for C in (1, 3, 16, 17, 63, 200, 1000):
        _syrk_case(eng, C, D, 1000 * D + C)


@pytest.mark.parametrize("D", [1500, 2100, 2820])
def test_syrk_tn_every_tile_size(D):
    """The tile is chosen by D: 64 x 64 with the epilogue in the product kernel (1500: 276 tiles), 128 x 128 in parts
    (2100) and 128 x 128 with the epilogue in the kernel (2820: 276 tiles); the shapes above cover 32 x 32 and 64 x 64 in
    parts.  17 chains: one full K-tile and a tail."""
    from aehmc_amd.engine import get_engine
    _syrk_case(get_engine(), 17, D, D)


def _check_state(st, s, full, D):
    """All fields of the device state against the restatement (tolerances of test_adapt_update_kernel_matches_oracle)."""
    h = {k: v.cpu().numpy() for k, v in st.items()}
    low = np.tril(np.ones((D, D), dtype=bool)) if full else np.ones(D, dtype=bool)
    np.testing.assert_allclose(h["step_size"], np.full_like(h["step_size"], s.step_size), rtol=1e-12)
    assert (h["step_size"] == h["step_size"][0]).all()
    assert h["da_step"][0] == s.step and h["wc_n"][0] == s.n
    assert h["da_x"][0] == pytest.approx(s.x, rel=1e-12, abs=1e-15)
    assert h["da_x_avg"][0] == pytest.approx(s.x_avg, rel=1e-12, abs=1e-15)
    assert h["da_g_avg"][0] == pytest.approx(s.g_avg, rel=1e-12, abs=1e-15)
    assert h["da_mu"][0] == pytest.approx(s.mu, rel=1e-12)
    np.testing.assert_allclose(h["wc_mean"], s.mean, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(h["wc_m2"][low], s.m2[low], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(h["imm"], s.imm, rtol=1e-12)
    return h


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("C,D", [(1, 7), (5, 1), (64, 70), (257, 130)])
def test_pooled_update_with_fed_inputs(C, D, full):
    """Identical (acceptance probability, position) sequences in, identical pooled warm-up state out; at a window end
    imm is the shrunk np.cov of the window's stacked draws, bitwise symmetric, and sqrt_mass its factor.  C = 1: the
    per-chain kernel's result.  The draws share a common factor, so that every covariance is far from zero: an
    element-wise RELATIVE tolerance holds for sums of like-signed terms, not for sums that cancel."""
    from aehmc_amd.engine import get_engine
    eng = get_engine()
    num_steps = 150
    r = np.random.default_rng(17 * C + D)
    load = 1 + np.arange(D) / D
    st, cst = eng.pooled_adapt_alloc(C, D, full)
    eng.pooled_adapt_init(C, D, 0.37, cst)
    s = pr.init(D, full, 0.37)
    _check_state(st, s, full, D)
    if C == 1:
        st1, cst1 = eng.adapt_alloc(1, D, full)
        eng.adapt_init(1, D, 0.37, cst1)
    window, ends = [], 0
    for i, (stage, wend) in enumerate(pr.build_schedule(num_steps)):
        pa = r.random(C)
        pos = 2 * r.normal(size=(C, 1)) * load + 0.3 * r.normal(size=(C, D)) + 0.5
        last = i == num_steps - 1
        eng.pooled_adapt_update(C, D, stage, wend, last, 0.8, _dev(pa), _dev(pos), cst)
        s = pr.update(s, stage, wend, last, pos, pa)
        if C == 1:
            eng.adapt_update(1, D, stage, wend, last, 0.8, _dev(pa), _dev(pos), cst1)
        if stage:
            window.append(pos)
        if not (wend or i % 37 == 0 or last):
            continue
        h = _check_state(st, s, full, D)
        if C == 1:
            # (sqrt_mass is checked below as a factor of imm: the conditioning of imm multiplies its rounding)
            for k in ("step_size", "da_x", "da_x_avg", "da_g_avg", "da_mu", "imm"):
                np.testing.assert_allclose(h[k].reshape(-1), st1[k].cpu().numpy().reshape(-1), rtol=1e-12, atol=1e-15)
        if wend:
            ends += 1
            stacked = np.concatenate(window)
            window = []
            cov = np.atleast_2d(np.cov(stacked.T, ddof=1))
            np.testing.assert_allclose(h["imm"], pr.shrink(cov if full else np.diag(cov), stacked.shape[0], full), rtol=1e-10)
            S = h["sqrt_mass"]
            if full:
                assert np.array_equal(h["imm"], h["imm"].T)
                assert np.array_equal(S, np.triu(S))
                np.testing.assert_allclose(S.T @ h["imm"] @ S, np.eye(D), atol=1e-8)
                np.testing.assert_allclose(S, s.sqrt_mass, rtol=1e-8, atol=1e-10 * np.abs(s.sqrt_mass).max())
                assert not h["wc_m2"].any() and not h["wc_mean"].any()
            else:
                np.testing.assert_allclose(S, np.sqrt(1 / h["imm"]), rtol=1e-12)
    assert ends == 1


def _kernels(kind, srng, tgt):
    from aehmc_amd import hmc, nuts
    if kind == "nuts":
        return nuts.new_kernel(srng, tgt), nuts.new_state, {}, ()
    return hmc.new_kernel(srng, tgt), hmc.new_state, {"num_integration_steps": 5}, (5,)


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
@pytest.mark.parametrize("full,D,C,dense_target", [(False, 30, 7, False), (True, 6, 5, False), (True, 80, 3, False),
                                                   (True, 600, 5, True)])
def test_fused_pooled_warmup_equals_step_by_step(kind, full, D, C, dense_target):
    """run(pooled=True) through aehmc_*_warmup_pooled issues the launches of the step-by-step Python loop in the same
    order: identical position, step size, metric, next transition and RNG.  (600, dense target: the whitened lock-step
    path, whose operator the loop drops at a window end by binding the metric again.)"""
    from aehmc_amd import RandomStream, targets, window_adaptation
    from aehmc_amd.engine import get_engine
    r = np.random.default_rng(D + C)
    mu, sigma = r.normal(size=D), 0.5 + r.random(D)
    if dense_target:
        B = r.normal(size=(D, D)) / np.sqrt(D)
        prec = B @ B.T + np.diag(1 / sigma ** 2)
        tgt = targets.DenseMVN(mu, 0.5 * (prec + prec.T))
    else:
        tgt = targets.DiagGaussian(mu, sigma)
    q0 = mu + sigma * r.normal(size=(C, D))
    outs = []
    for fused in (True, False):
        srng = RandomStream(seeds=[300 + c for c in range(C)])
        kernel, new_state, kw, extra = _kernels(kind, srng, tgt)
        state = new_state(torch.as_tensor(q0, device="cuda"), tgt)
        state, (eps, imm), upd = window_adaptation.run(kernel, state, 130, is_mass_matrix_full=full, fused=fused,
                                                       pooled=True, **kw)
        assert isinstance(eps, float) and imm.shape == ((D, D) if full else (D,))
        info, upd = kernel(state, eps, imm, *extra)
        sqrt_mass = get_engine()._keep["metric"][2]  # (what the engine bound for imm)
        outs.append((state.position.clone(), torch.tensor(eps), imm.clone(), sqrt_mass.clone(),
                     info.state.position.clone(), upd[srng].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[0][4]).all() and outs[0][1].item() > 0


@pytest.mark.parametrize("full", [False, True])
def test_pooled_window_adaptation_matches_oracle(full):
    """End to end on identical seeds: the numpy pooled restatement driven by the oracle's NUTS kernel over all chains
    with the shared metric.  60 steps, the horizon test_window_adaptation_matches_oracle explains."""
    from aehmc_amd import RandomStream, nuts, targets, window_adaptation
    C, D, num_steps = 4, 3, 60
    r = np.random.default_rng(5 + full)
    mu, sigma = r.normal(size=D), 0.5 + 2 * r.random(D)
    tgt, otgt = targets.DiagGaussian(mu, sigma), co.Target(co.T_DIAG_GAUSSIAN, D, mu=mu, sigma=sigma)
    seeds = [300 + c for c in range(C)]
    q0 = r.normal(size=(C, D))
    kernel = nuts.new_kernel(RandomStream(seeds=seeds), tgt)
    state = nuts.new_state(torch.as_tensor(q0, device="cuda"), tgt, num_chains=C)
    last, (eps, imm), _ = window_adaptation.run(kernel, state, num_steps, is_mass_matrix_full=full, pooled=True)

    rng = co.site_states(seeds, 4)
    q, U, g = co.new_state(otgt, q0)

    def transition(X, step_size, imm_o):
        res = co.nuts_step(otgt, co.Metric(imm_o, D), rng, float(step_size), q, U, g)
        return q.copy(), res["acceptance_probability"].copy()

    X, s = pr.run(transition, q.copy(), num_steps, full)
    assert eps == pytest.approx(s.step_size, rel=1e-6)
    np.testing.assert_allclose(imm.cpu().numpy(), s.imm, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(last.position.cpu().numpy(), X, rtol=1e-6, atol=1e-9)


def test_pooled_full_adaptation_recovers_covariance():
    """The target and thresholds of test_window_adaptation_full_recovers_covariance, for the ONE pooled matrix; the
    adapted parameters are plain shared values and go straight into sample()."""
    from aehmc_amd import RandomStream, nuts, targets, window_adaptation
    C, D = 48, 3
    r = np.random.default_rng(2)
    A = r.normal(size=(D, D))
    cov = A @ A.T + 0.5 * np.eye(D)
    prec = np.linalg.inv(cov)
    prec = 0.5 * (prec + prec.T)
    tgt = targets.DenseMVN(np.zeros(D), prec)
    kernel = nuts.new_kernel(RandomStream(seeds=[900 + c for c in range(C)]), tgt)
    state = nuts.new_state(torch.as_tensor(r.normal(size=(C, D)), device="cuda"), tgt)
    last, (eps, imm), _ = window_adaptation.run(kernel, state, 600, pooled=True, is_mass_matrix_full=True)
    assert imm.shape == (D, D) and isinstance(eps, float) and isinstance(imm, torch.Tensor)
    m = imm.cpu().numpy()
    assert np.isfinite(m).all() and np.isfinite(eps) and np.array_equal(m, m.T)
    rel = np.abs(m - cov) / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    assert rel.max() < 0.35, rel
    samples, info, acc, div = kernel.sample(last, eps, imm, 200)
    assert not div.any().item() and acc.mean().item() > 0.6
    emp = np.cov(samples.cpu().numpy().reshape(-1, D).T)
    assert (np.abs(emp - cov) / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))).max() < 0.25


def test_pooled_init_update_pair_equals_run():
    """window_adaptation(num_steps, pooled=True) gives the (init, update) pair of the same adaptation: driving the loop by
    hand ends where run(pooled=True, fused=False) does."""
    from aehmc_amd import RandomStream, nuts, targets, window_adaptation
    C, D, num_steps = 6, 4, 110
    r = np.random.default_rng(9)
    tgt = targets.DiagGaussian(r.normal(size=D), 0.5 + r.random(D))
    q0 = r.normal(size=(C, D))
    k1 = nuts.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    s1, (eps, imm), _ = window_adaptation.run(k1, nuts.new_state(_dev(q0), tgt), num_steps, pooled=True, fused=False,
                                              is_mass_matrix_full=True)
    k2 = nuts.new_kernel(RandomStream(seeds=list(range(C))), tgt)
    state = nuts.new_state(_dev(q0), tgt)
    init, update = window_adaptation.window_adaptation(num_steps, is_mass_matrix_full=True, pooled=True)
    ws, params = init(state)
    for i in range(num_steps):
        info, _ = k2(state, *params)
        state = info.state._replace(momentum=None)
        ws, params = update(i, ws, params, info)
    assert torch.equal(state.position, s1.position) and torch.equal(params[1], imm)
    assert float(params[0].value[0]) == eps
