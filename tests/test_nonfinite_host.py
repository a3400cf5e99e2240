"""The reference side of the non-finite-energy tests (tests/nonfinite_cases.py), on the CPU: oracle/np_oracle.py and
oracle/c/aehmc_oracle.c agree on every case table that tests/test_gpu_nonfinite.py compares a kernel family against --
positions, energies, flags, n_leapfrog, acceptance and every site's generator words -- the wall inputs meet their
condition, and no decision of a case sits within rounding of flipping (the device may then differ in the last bits of
an energy without changing a flag or a draw).  Rules under test: aehmc/hmc.py:189-195, proposals.py:43-45, 95-97,
trajectory.py:336."""
import numpy as np
import pytest

import nonfinite_cases as nc
from oracle import c_oracle as co
from oracle import np_oracle as no

T = 2
MAX_UNSAFE_SHARE = 0.02


def gaussian_case(D, metric, seed):
    r = np.random.default_rng(seed)
    mu, sigma = r.normal(size=D), 0.5 + r.random(D)
    if metric == "dense":
        A = r.normal(size=(D, D))
        imm = A @ A.T / D + np.eye(D)
        imm = 0.5 * (imm + imm.T)
    else:
        imm = 0.5 + r.random(D)
    return r, no.DiagGaussian(mu, sigma), co.Target(co.T_DIAG_GAUSSIAN, D, mu=mu, sigma=sigma), imm


def linreg_case(seed, N=700):
    r = np.random.default_rng(seed)
    X = r.normal(size=N)
    y = 3 * X + 0.5 * r.normal(size=N)
    return r, no.LinearRegression(X, y), co.Target(co.T_LINREG, 2, X=X, y=y), np.array([1.0 / N, 0.5 / N]), N


def both_oracles(sampler, tgt, otgt, imm, q0, eps, seeds, thr=1000.0):
    """np_oracle (margins observed) against the C oracle; returns the C oracle's transitions"""
    rng = co.site_states(seeds, 4 if sampler == "nuts" else 2)
    ref, m = nc.with_margins(lambda: nc.np_run(sampler, tgt, rng, q0, eps, imm, T, thr=thr))
    got = nc.c_run(sampler, otgt, imm, rng, q0, eps, T, thr=thr)
    for t in range(T):
        nc.assert_same_transition(got[t], ref[t], sampler, what=(sampler, t))
    # (no case is dropped: the seeds below leave no decision within 1e-6 relative of its decision point)
    assert m.n > 0 and len(m.unsafe) <= MAX_UNSAFE_SHARE * m.n and not m.unsafe, m.unsafe[:5]
    return got


@pytest.mark.parametrize("sampler", ["nuts", "hmc"])
@pytest.mark.parametrize("D,metric", [(3, "diag"), (24, "diag"), (24, "dense")])
def test_oracles_agree_on_poisoned_starts(sampler, D, metric):
    r, tgt, otgt, imm = gaussian_case(D, metric, 100 + D)
    C = nc.C_DEFAULT
    q0, labels = nc.poison_starts(r.normal(size=(C, D)), nc.GAUSS_POISONS, r)
    nc.assert_scale_is_order_safe(q0)
    out = both_oracles(sampler, tgt, otgt, imm, q0, 0.25 / D ** 0.25, list(range(500, 500 + C)))
    bad = nc.is_poisoned(C)
    nonfinite = bad & (np.array(labels) != "scale")  # (a finite H0 of 1e300 may also DROP by 1e298: diverging, yet accepted)
    for t in range(T):  # the rules: a non-finite energy diverges with p_accept = 0 and the chain stays, bit for bit
        assert out[t]["is_diverging"][bad].all() and (out[t]["acceptance_probability"][nonfinite] == 0).all(), labels
        assert nc.stayed(q0, out[t]["position"])[nonfinite].all()
        assert not out[t]["is_diverging"][~bad].any()


@pytest.mark.parametrize("sampler", ["nuts", "hmc"])
def test_oracles_agree_on_poisoned_regression_starts(sampler):
    r, tgt, otgt, imm, N = linreg_case(7)
    C = nc.C_DEFAULT
    q0 = np.array([3.0, np.log(0.5)]) + (0.5 / np.sqrt(N)) * r.normal(size=(C, 2))
    q0, labels = nc.poison_starts(q0, nc.LINREG_POISONS, r)
    out = both_oracles(sampler, tgt, otgt, imm, q0, 0.3, list(range(700, 700 + C)))
    bad = nc.is_poisoned(C)
    for t in range(T):
        assert out[t]["is_diverging"][bad].all() and nc.stayed(q0, out[t]["position"])[bad].all(), labels


@pytest.mark.parametrize("sampler", ["nuts", "hmc"])
@pytest.mark.parametrize("D,metric", [(3, "diag"), (24, "diag"), (24, "dense")])
def test_oracles_agree_on_poisoned_step_sizes(sampler, D, metric):
    r, tgt, otgt, imm = gaussian_case(D, metric, 200 + D)
    C = nc.C_DEFAULT
    q0 = r.normal(size=(C, D))
    eps = nc.poison_step_sizes(C, 0.25 / D ** 0.25)
    out = both_oracles(sampler, tgt, otgt, imm, q0, eps, list(range(900, 900 + C)))
    bad = nc.is_poisoned(C)
    for t in range(T):
        assert out[t]["is_diverging"][bad].all() and nc.stayed(q0, out[t]["position"])[bad].all()


@pytest.mark.parametrize("thr,eps", nc.NEVER_FIRES)
@pytest.mark.parametrize("D", [3, 24])
def test_oracles_agree_where_the_threshold_never_fires(D, thr, eps):
    """divergence_threshold = inf: nothing diverges, and infinite weights reach the logaddexp's and the biased draw"""
    r, tgt, otgt, imm = gaussian_case(D, "diag", 300 + D)
    C = 10
    out = both_oracles("nuts", tgt, otgt, imm, r.normal(size=(C, D)), eps, list(range(40, 40 + C)), thr=thr)
    if np.isinf(thr):
        assert not any(o["is_diverging"].any() for o in out)


@pytest.mark.parametrize("sampler", ["nuts", "hmc"])
@pytest.mark.parametrize("D,poison", [(D, p) for D in sorted(nc.WALLS) for p in nc.WALL_POISONS if D <= 200 or p == "nan"])
def test_wall_inputs_meet_their_condition(D, poison, sampler):
    """The wall cases of tests/test_gpu_nonfinite.py on np_oracle alone: enough transitions that meet the poison in
    mid-tree, one at least at a first step, a third of the chains untouched.  HMC has no tree: at least four diverging
    transitions and a third of the chains untouched.  With U = -inf the reference ACCEPTS with probability 1 and flags a
    divergence (hmc.py:189-195: delta = +inf); the chain then sits at H0 = -inf and every later delta is NaN -> -inf.
    (The shapes above 200 coordinates run one poison here: np_oracle is a Python loop over coordinates.)"""
    out = wall_case(D, poison, sampler)
    C = out[0]["position"].shape[0]
    if sampler == "nuts":
        nc.assert_wall_condition(out, C, what=(D, poison))
    else:
        div = np.stack([o["is_diverging"] for o in out])
        assert div.sum() >= 4 and 3 * (~div).all(axis=0).sum() >= C, (D, poison, div.sum())
        if poison == "minus_inf":
            hit = div[0]
            assert hit.any() and (out[0]["acceptance_probability"][hit] == 1).all()
            assert np.isneginf(out[0]["potential_energy"][hit]).all() and div[1][hit].all()


def wall_case(D, poison, sampler, form="elementwise"):
    p = nc.WALL_POISONS[poison]
    if form == "glm":
        X, y, C, seeds, q0, imm, eps, w = nc.wall_glm_inputs(D, sampler=sampler)
        tgt, L = nc.WallGLM(X, y, w, p), nc.GLM_L
    else:
        C, seeds, q0, w = nc.wall_inputs(D, sampler, joint=form == "joint")
        tgt = nc.wall_joint_target(w, p) if form == "joint" else nc.Wall(w, p)
        imm, eps, L = (np.ones(D) if form == "joint" else nc.wall_metric(D)), nc.wall_eps(D), nc.wall_length(D)
    rng = co.site_states(seeds, 4 if sampler == "nuts" else 2)
    out, m = nc.with_margins(lambda: nc.np_run(sampler, tgt, rng, q0, eps, imm, T, L=L))
    assert not m.unsafe, m.unsafe[:5]
    return out


@pytest.mark.parametrize("sampler", ["nuts", "hmc"])
@pytest.mark.parametrize("form,size,poison", [("joint", 70, p) for p in nc.WALL_POISONS] + [("joint", 600, "nan")]
                         + [("glm", N, p) for N in (900, 300) for p in nc.WALL_POISONS])
def test_joint_and_glm_wall_inputs_meet_their_condition(form, size, poison, sampler):
    out = wall_case(size, poison, sampler, form)
    C = out[0]["position"].shape[0]
    if sampler == "nuts":
        nc.assert_wall_condition(out, C, what=(form, size, poison))
    else:
        div = np.stack([o["is_diverging"] for o in out])
        assert div.sum() >= 4 and 3 * (~div).all(axis=0).sum() >= C, (form, size, poison, div.sum())


def c_literal(x):
    return "NAN" if np.isnan(x) else ("-INFINITY" if x < 0 else "INFINITY") if np.isinf(x) else repr(float(x))


@pytest.mark.parametrize("poison", list(nc.WALL_POISONS))
def test_traced_wall_reads_its_poison_from_the_parameters(poison, tmp_path):
    """The wall density traced with tracing.where: a joint density whose emitted source, forward and reverse program,
    gives the Python function's value (the poison, same class and sign) and the Gaussian's gradient on both sides of the
    wall -- the tracer has not folded the poison away, and its adjoint passes no 0 * inf on."""
    import os
    import subprocess
    import test_tracing as tt
    from aehmc_amd import tracing
    D, w, p = 6, 1.5, nc.WALL_POISONS[poison]
    tr = tracing.trace(nc.wall_joint_logp, D, args=(np.array([w]), np.array([p])), reverse=True)
    assert not tr.elementwise and "prm[1][0]" in tr.source and "prm1[0]" in tr.grad_source
    ref = nc.wall_joint_target(w, p)
    params = "".join(f"static const double prm{k}[] = {{{', '.join(c_literal(x) for x in a)}}};\n" for k, a in enumerate(tr.params))
    params += "static const double *const prm[] = {prm0, prm1, nullptr};\n"
    inc = os.path.join(tt.ROOT, "aehmc_amd", "csrc")
    for name, q in (("inside", np.array([0.3, -1.2, 1.4, 0.0, 1.49, -3.0])), ("outside", np.array([0.3, -1.2, 1.6, 0.0, 0.5, -3.0])),
                    ("at", np.array([1.5, 0.1, 0.2, 0.3, 0.4, 0.5]))):
        U, g = ref(q)
        assert np.isfinite(U) == (name == "inside")
        for harness, source, tag in ((tt.HARNESS, tr.source, "fwd"), (tt.REV_HARNESS, tr.grad_source, "rev")):
            src = tmp_path / f"{name}_{tag}.cpp"
            src.write_text(harness % dict(source=source, params=params, D=D, q=", ".join(repr(float(x)) for x in q), elem=0))
            exe = tmp_path / f"{name}_{tag}"
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", inc, "-o", str(exe), str(src)])
            out = [float(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
            nc.assert_reals(np.array([-out[0]]), np.array([U]), what=(poison, name, tag, "value"))
            nc.assert_reals(-np.array(out[1:]), g, atol=1e-15, what=(poison, name, tag, "gradient"))


def test_meads_ref_applies_the_nan_rule():
    """tests/meads_ref.py restates hmc.py:190 for generalised HMC: a NaN energy difference is -inf, the proposal is rejected
    (momentum flipped), p_accept = 0 and the step counts as diverging."""
    import meads_ref as mr
    D, C = 7, 6
    r = np.random.default_rng(0)
    t = mr.DiagGaussian(r.normal(size=D), 0.5 + r.random(D))
    q0 = r.normal(size=(C, D))
    q0[1, D - 1], q0[2, 0], q0[4] = np.nan, np.inf, 1e160
    g1, g2 = mr.sites(list(range(C)))
    with np.errstate(all="ignore"):
        ch, info = mr.transition(mr.start(t, q0), g1, g2, t, 0.1, 0.5, 0.3, mr.parity_scale(D))
    bad = np.array([0, 1, 1, 0, 1, 0], dtype=bool)
    assert np.isneginf(info.energy_change[bad]).all() and not info.accepted[bad].any()
    assert (info.acceptance_probability[bad] == 0).all() and info.is_diverging[bad].all()
    assert (nc.bits(ch.q[bad]) == nc.bits(q0[bad])).all()
    assert info.accepted[~bad].any() and not info.is_diverging[~bad].any()
