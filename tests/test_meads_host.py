"""Host-side checks of generalised HMC and the MEADS warm-up: the numpy restatement (tests/meads_ref.py) against numbers
worked out by hand, the golden reference runs, the margins of the fixtures the GPU tests compare flag for flag, the
argument errors of aehmc_amd.ghmc / aehmc_amd.meads, and the C declarations against aehmc_amd._lib."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meads_ref as mr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "meads_ref_runs.json")


def test_lam_in_both_forms():
    X = np.random.default_rng(0).normal(size=(37, 5))
    a, b = mr.lam(X), mr.lam_dxd(X)
    assert abs(a - b) <= 1e-12 * abs(a), (a, b)
    # rank one: every row the same direction -> the one non-zero eigenvalue of X^T X / n, up to the (n - 1) / n of the
    # dropped diagonal: sum_ab (r_a r_b)^2 - sum_a r_a^4 over n (n - 1), over sum r_a^2 / n
    r = np.arange(1.0, 6.0)
    want = ((np.sum(r * r) ** 2 - np.sum(r ** 4)) / 20.0) / (np.sum(r * r) / 5.0)
    assert abs(mr.lam(np.outer(r, [0.6, 0.8])) - want) <= 1e-12 * want


def test_update_by_hand():
    """Three chains, two coordinates.  Q = [[0, 0], [1, 2], [2, 4]]: m = (1, 2), var = (2/3, 8/3), so
    Z = [[-a, -a], [0, 0], [a, a]] with a = sqrt(3/2); Z Z^T = [[3, 0, -3], [0, 0, 0], [-3, 0, 3]]: sum of squares 36,
    of the squared diagonal 18, lam(Z) = (18 / 6) / (6 / 3) = 3/2.
    G chosen so that Gs = G sd = [[1, 1], [1, -1], [2, 0]]: Gs Gs^T = [[2, 0, 2], [0, 2, 2], [2, 2, 4]]: sum of squares
    40, of the squared diagonal 24, lam(Gs) = (16 / 6) / (8 / 3) = 1.
    eps = min(1, 0.5 / 1) = 0.5; gamma = max(1 / sqrt(3/2), 1 / (1^1 0.5)) = 2; alpha = 1 - exp(-2); delta = alpha / 2."""
    Q = np.array([[0.0, 0.0], [1.0, 2.0], [2.0, 4.0]])
    sd = np.sqrt([2.0 / 3.0, 8.0 / 3.0])
    G = np.array([[1.0, 1.0], [1.0, -1.0], [2.0, 0.0]]) / sd
    t = mr.statistics(Q, G)
    for got, want in ((t["lam_z"], 1.5), (t["lam_g"], 1.0), (t["z4"], 18.0), (t["z2"], 6.0), (t["g4"], 24.0), (t["g2"], 8.0),
                      (t["Fz"], 36.0), (t["Fg"], 40.0)):
        assert abs(got - want) <= 1e-13 * want, (got, want)
    st = mr.update(mr.init(2), Q, G)
    assert abs(st.eps - 0.5) <= 1e-14 and abs(st.alpha - (1.0 - math.exp(-2.0))) <= 1e-14
    assert st.delta == st.alpha / 2 and np.allclose(st.scale, sd, rtol=1e-15) and (st.count, st.skipped) == (1, 0)
    # the slowdown term: at the second update it is 1 / (2^1 0.5) = 1, still above 1 / sqrt(3/2): gamma = 1
    st2 = mr.update(st, Q, G)
    assert abs(st2.alpha - (1.0 - math.exp(-2.0 * 0.5 * max(1.0 / math.sqrt(1.5), 1.0)))) <= 1e-14 and st2.count == 2


def test_guard_keeps_the_parameters():
    Q = np.array([[1.0, 2.0], [1.0, 2.0]])  # two identical chains: sd = 0
    st0 = mr.init(2, 0.01)
    st = mr.update(st0, Q, np.ones((2, 2)))
    assert (st.eps, st.alpha, st.delta) == (0.01, 1.0, 0.5) and (st.scale == 1.0).all() and (st.count, st.skipped) == (1, 1)
    assert mr.update(st, Q, np.full((2, 2), np.nan)).skipped == 2


class _Fixed:
    """A generator that returns what it was given."""

    def __init__(self, normals, uniform=None):
        self.normals, self.uniform = normals, uniform

    def standard_normal(self, D):
        return np.asarray(self.normals, dtype=np.float64)

    def random(self):
        return self.uniform


def test_transition_branches_by_hand():
    """Standard normal, D = 1, q = 0, eps = 0.5, s = 1, alpha = 1 (v = z = 1), delta = 0.3.  Leapfrog: vh = 1, q' = 0.5,
    g' = 0.5, v' = 0.875; Delta = 0.5 - (0.125 + 0.5 0.765625) = -0.0078125.
    Chain 0: u = 0.9 -> fmod(1.9 + 0.3, 2) - 1 = -0.8 (wrapped); log 0.8 < Delta: accept, u' = -0.8 exp(0.0078125).
    Chain 1: u = 0.699 -> 0.999; log 0.999 > Delta: reject, q stays, v = -1, u stays."""
    t = mr.StdNormal(1)
    ch = mr.start(t, np.zeros((2, 1)))._replace(v=np.array([[5.0], [5.0]]), u=np.array([0.9, 0.699]))
    g1 = [_Fixed([1.0]), _Fixed([1.0])]
    new, info = mr.transition(ch, g1, [None, None], t, 0.5, 1.0, 0.3, 1.0)
    assert info.accepted.tolist() == [True, False]
    assert np.allclose(info.acceptance_probability, math.exp(-0.0078125), rtol=1e-15)
    assert new.q[:, 0].tolist() == [0.5, 0.0] and new.g[:, 0].tolist() == [0.5, 0.0] and new.v[:, 0].tolist() == [0.875, -1.0]
    assert abs(new.u[0] + 0.8 * math.exp(0.0078125)) <= 1e-15 and abs(new.u[1] - 0.999) <= 1e-15
    assert abs(new.U[0] - (0.125 + mr.LOG_SQRT_2PI)) <= 1e-15 and new.U[1] == mr.LOG_SQRT_2PI
    assert np.array_equal(mr.slice_step(ch.u, info, 0.3), new.u)  # (the one-step map the GPU test applies to the device's slice)
    # partial refreshment and the first slice: v = sqrt(1 - alpha) v + sqrt(alpha) z, u = 2 r - 1 then the drift
    ch = mr.start(t, np.zeros((1, 1)))._replace(v=np.array([[2.0]]))
    new, info = mr.transition(ch, [_Fixed([1.0])], [_Fixed(None, 0.25)], t, 1e-3, 0.36, 0.1, 1.0)
    v = 0.8 * 2.0 + 0.6 * 1.0
    assert info.accepted[0] and abs(new.v[0, 0] - (v - 0.5e-3 * (1e-3 * v))) <= 1e-15
    assert abs(abs(new.u[0]) - 0.4 * math.exp(-(math.log(info.acceptance_probability[0])))) <= 1e-12 or info.acceptance_probability[0] == 1.0
    # a NaN energy difference rejects, whatever u
    bad = mr.start(t, np.zeros((1, 1)))._replace(U=np.array([np.nan]), u=np.array([1e-300]))
    new, info = mr.transition(bad, [_Fixed([1.0])], [None], t, 0.5, 1.0, 0.0, 1.0)
    assert not info.accepted[0] and info.acceptance_probability[0] == 0.0 and new.v[0, 0] == -1.0


def test_fixture_margins():
    """The GPU tests compare accept flags for equality and leave no chain out: no accept test of the reference may be
    within 1e-6 of flipping (log|u| - Delta), in the fixed-parameter parity cases, the funnel cases and the loop."""
    for name in mr.PARITY_TARGETS:
        for C, D in mr.PARITY_SHAPES:
            _, _, hist, _ = mr.parity_run(name, C, D)
            assert min(float(i.margin.min()) for _, i in hist) > 1e-6, (name, C, D)
            assert any(i.accepted.any() for _, i in hist)
    assert any(not i.accepted.all() for _, i in mr.parity_run("diag_gaussian", 65, 65)[2])  # both branches are run
    for D in mr.FUNNEL_DIMS:
        assert min(float(i.margin.min()) for _, i in mr.funnel_run(D)[3]) > 1e-6, D
    t, q0, seeds = mr.loop_start()
    assert mr.warmup(t, q0, seeds, mr.LOOP["steps"])[3] > 1e-6


def test_golden_reference_runs():
    """tests/golden/meads_ref_runs.json (python tests/meads_ref.py writes it): final eps, alpha and log(scale / sigma) of
    16 seeds of the restatement, 300 steps, C = 256, on the 20-dimensional standard normal and on
    DiagGaussian(linspace(1, 10, 20)).  The first seed of each target is run again here and must give the file's numbers
    (to 1e-6 relative: a whole warm-up repeats to rounding unless an accept test falls within rounding of its threshold,
    and the matrix products inside ``lam`` may round differently on another machine); the spread of eps is positive and
    below 10 % of its mean."""
    gold = json.load(open(GOLDEN))
    assert (gold["C"], gold["D"], gold["steps"], gold["seeds"]) == (256, 20, 300, 16)
    for name in mr.GOLDEN_SIGMA:
        g = gold[name]
        eps, alpha, ratio = np.array(g["eps"]), np.array(g["alpha"]), np.array(g["log_scale_ratio"])
        assert eps.shape == alpha.shape == (16,) and ratio.shape == (16, 20)
        e0, a0, r0 = mr.golden_run(name, 0)
        assert abs(e0 - eps[0]) <= 1e-6 * eps[0] and abs(a0 - alpha[0]) <= 1e-6 * alpha[0]
        assert np.abs(r0 - ratio[0]).max() <= 1e-6
        assert 0 < eps.std(ddof=1) < 0.1 * eps.mean() and 0 < alpha.std(ddof=1) < 0.1 * alpha.mean(), name
        assert np.abs(ratio).max() < 0.25, name
        print(name, f"eps = {eps.mean():.4f} +- {eps.std(ddof=1):.4f}, alpha = {alpha.mean():.4f} +- {alpha.std(ddof=1):.4f}, "
                    f"max |log(scale / sigma)| = {np.abs(ratio).max():.3f}")


def test_argument_errors_come_before_any_device_work(monkeypatch):
    """The ValueErrors of ghmc and meads; with no device everything else raises the engine's no-device error, which
    shows that they came first."""
    import torch
    import aehmc_amd as aa
    from aehmc_amd import ghmc, meads, targets
    from aehmc_amd.engine import EngineError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    C, D = 3, 2
    f64 = torch.float64
    state = ghmc.GhmcState(torch.zeros(C, D, dtype=f64), None, torch.zeros(C, dtype=f64), torch.zeros(C, D, dtype=f64), None)
    assert state.momentum is None and state.slice is None
    kernel = ghmc.new_kernel(aa.RandomStream(seeds=range(C)), targets.StdNormal())
    hmc_kernel = aa.hmc.new_kernel(aa.RandomStream(seeds=range(C)), targets.StdNormal())
    nuts_kernel = aa.nuts.new_kernel(aa.RandomStream(seeds=range(C)), targets.StdNormal())
    for other in (hmc_kernel, nuts_kernel, lambda *a: None):
        with pytest.raises(ValueError, match="generalised-HMC kernel"):
            meads.run(other, state, 10)
        with pytest.raises(ValueError, match="generalised-HMC kernel"):
            meads.sample(other, state, 0.5, 1.0, 0.5, 0.25, 4)
    with pytest.raises(ValueError, match="static HMC kernel"):
        aa.chees.run(kernel, state, 10)  # and a GHMC kernel is not taken for an HMC one
    one = ghmc.GhmcState(torch.zeros(1, D, dtype=f64), None, torch.zeros(1, dtype=f64), torch.zeros(1, D, dtype=f64), None)
    with pytest.raises(ValueError, match="at least 2"):
        meads.run(ghmc.new_kernel(aa.RandomStream(seeds=[0]), targets.StdNormal()), one, 10)
    with pytest.raises(ValueError, match="at least 2"):
        meads.adaptation()[0](one)
    with pytest.raises(ValueError, match="PerChain"):
        kernel(state, 0.5, aa.PerChain(torch.ones(C, D, dtype=f64)), 0.5, 0.25)
    with pytest.raises(ValueError, match="dense"):
        kernel.sample(state, 0.5, torch.eye(D, dtype=f64), 0.5, 0.25, 4)
    for eps, alpha, delta, what in ((0.0, 0.5, 0.25, "step_size"), (-1.0, 0.5, 0.25, "step_size"), (0.5, 0.0, 0.25, "alpha"),
                                    (0.5, 1.5, 0.25, "alpha"), (0.5, float("nan"), 0.25, "alpha"), (0.5, 0.5, -0.1, "delta")):
        with pytest.raises(ValueError, match=what):
            kernel(state, eps, 1.0, alpha, delta)
        with pytest.raises(ValueError, match=what):
            meads.sample(kernel, state, eps, 1.0, alpha, delta, 4)
    with pytest.raises(ValueError, match="positive"):
        meads.run(kernel, state, 10, step_size_multiplier=0.0)
    with pytest.raises(ValueError, match="positive"):
        meads.adaptation(initial_step_size=-1.0)
    with pytest.raises(EngineError, match="no CPU fallback"):
        meads.run(kernel, state, 10)
    with pytest.raises(EngineError, match="no CPU fallback"):
        kernel(state, 0.5, 1.0, 0.5, 0.25)


def test_lib_declares_the_header_of_the_new_calls():
    from aehmc_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "aehmc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("aehmc_ghmc_sample", "aehmc_meads_update", "aehmc_meads_warmup"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
    fields = re.search(r"typedef struct \{([^}]*)\}\s*aehmc_meads_state;", hdr).group(1)
    names = re.findall(r"\*?\s*\**(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.CMeadsState._fields_]
    declared = set(re.findall(r"\b(aehmc_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
