"""CPU-side checks of the ChEES warm-up: the numpy restatement (tests/chees_ref.py) on cases worked out by hand, the
Halton weights, the argument errors of aehmc_amd.chees, the C-ABI declarations, and the golden file of whole reference
warm-ups (tests/golden/chees_ref_runs.json) that the GPU statistics test compares the device with."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chees_ref as cr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chees_ref_runs.json")
SIGMA = np.linspace(1.0, 10.0, 20)
TARGETS = {"identity": 1.0, "imm_sigma": SIGMA}   # the inverse mass matrix of each statistical target
C_STAT, STEPS_STAT, SEEDS = 256, 800, 16


def test_first_16_halton_values():
    want = [1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8, 1 / 16, 9 / 16, 5 / 16, 13 / 16, 3 / 16, 11 / 16, 7 / 16,
            15 / 16, 1 / 32]
    from aehmc_amd import chees
    assert [cr.halton(n) for n in range(1, 17)] == want
    assert [chees.halton(n) for n in range(1, 17)] == want
    with pytest.raises(ValueError):
        chees.halton(0)


def test_reference_update_on_a_hand_made_case():
    """3 chains, 2 coordinates, chain 2 rejected (its momentum is NaN and must not matter), imm = (2, 1/2), worked out
    by hand: m0 = (1, 0), m1 = (2, 1);
    chain 0: d0 = (-1, 0), d1 = (-2, 1), v = -(2 * 1, 0.5 * -2) = (-2, 1): s = (5 - 1) * (4 + 1) = 20;
    chain 1: d0 = (1, 0), d1 = (1, 2), v = -(2 * -1.5, 0.5 * 4) = (3, -2): s = (5 - 1) * (3 - 4) = -4;  S = 16, A = 2."""
    q0 = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 0.0]])
    q1 = np.array([[0.0, 2.0], [3.0, 3.0], [3.0, -2.0]])   # m1 = (2, 1)
    mom = np.array([[1.0, -2.0], [-1.5, 4.0], [np.nan, np.nan]])
    imm = np.array([2.0, 0.5])
    acc, a = np.array([1, 1, 0]), np.array([1.0, 0.5, 0.25])
    t = cr.sums(q0, q1, mom, imm, acc, a)
    assert t.m0.tolist() == [1.0, 0.0] and t.m1.tolist() == [2.0, 1.0]
    assert t.S == 16.0 and t.A == 2.0 and t.abar == pytest.approx(1.75 / 3, rel=1e-15)
    s0 = cr.init(1.0, 4.0)
    assert s0.step == 1 and s0.h == 0.5 and s0.num_steps == 2 and s0.step_size == 1.0 and s0.log_T == math.log(4.0)
    s = cr.update(s0, False, t.S, t.A, t.abar, target=0.651, lr=0.025, max_steps=1000)
    G = 0.5 * math.exp(math.log(4.0)) * 16.0 / 2.0   # h T S / A = 16
    assert s.adam_m == pytest.approx(0.1 * G, rel=1e-15) and s.adam_v == pytest.approx(0.001 * G * G, rel=1e-15)
    # first Adam step: m-hat / sqrt(v-hat) = G / |G| = 1, so log_T rises by the learning rate
    g_avg = (0.651 - 1.75 / 3) / 11
    x = 1.0 - 20.0 * g_avg
    assert s.da_g_avg == pytest.approx(g_avg, rel=1e-14) and s.da_x == pytest.approx(x, rel=1e-14)
    assert s.step_size == pytest.approx(math.exp(x), rel=1e-14) and s.da_x_avg == 0.0 and s.da_step == 2
    # x = 0.877: log 4 + 0.025 = 1.411 lies inside [log eps, log(1000 eps)] = [x, x + 6.9]
    assert s.log_T == pytest.approx(math.log(4.0) + 0.025, rel=1e-9)
    assert s.log_T_avg == s.log_T   # w = 1^-kappa = 1
    assert s.step == 2 and s.h == 0.25
    assert s.num_steps == math.ceil(0.25 * math.exp(s.log_T) / s.step_size)
    # the rejected chain's momentum is not read: any value gives the same bits
    mom2 = mom.copy()
    mom2[2] = 7.0
    assert cr.sums(q0, q1, mom2, imm, acc, a).S == t.S


def test_no_accepted_chain_leaves_log_T_to_the_moments():
    s0 = cr.init(1.0, 3.0)._replace(adam_m=0.4, adam_v=0.09, step=5, da_step=5, h=cr.halton(5))
    q = np.ones((4, 3))
    t = cr.sums(q, q, np.full((4, 3), np.nan), 1.0, np.zeros(4), np.full(4, 0.6))
    assert t.S == 0.0 and t.A == 0.0
    s = cr.update(s0, False, t.S, t.A, t.abar)
    assert s.adam_m == pytest.approx(0.9 * 0.4) and s.adam_v == pytest.approx(0.999 * 0.09)   # G = 0
    step = 0.025 * (s.adam_m / (1 - 0.9 ** 5)) / (math.sqrt(s.adam_v / (1 - 0.999 ** 5)) + 1e-8)
    assert s.log_T == pytest.approx(s0.log_T + step, rel=1e-14)
    # a sum that is not finite counts as no information too
    s_inf = cr.update(s0, False, float("inf"), 2.0, 0.6)
    assert (s_inf.adam_m, s_inf.adam_v, s_inf.log_T) == (s.adam_m, s.adam_v, s.log_T)


def test_clamp_to_one_and_max_num_steps_leapfrogs():
    low = cr.update(cr.init(1.0, 1e-6), False, -1.0, 1.0, 0.651)        # T far below eps: lifted to eps
    assert low.log_T == math.log(low.step_size) and low.num_steps == 1
    high = cr.update(cr.init(1.0, 1e9), False, 1.0, 1.0, 0.651, max_steps=50)
    assert high.log_T == math.log(50 * high.step_size)
    assert high.num_steps in (math.ceil(0.25 * 50), math.ceil(0.25 * 50) + 1)   # h T / eps = 12.5 up to rounding
    capped = cr.update(cr.init(1.0, 1e9)._replace(h=1.0), False, 1.0, 1.0, 0.651, max_steps=7)
    assert capped.num_steps <= 7


def test_is_last_returns_the_averages():
    s = cr.init(1.0, 2.0)
    for i in range(5):
        s = cr.update(s, False, 3.0 - i, 2.0, 0.5 + 0.05 * i)
    mid = cr.update(s, False, 1.0, 2.0, 0.7)
    last = cr.update(s, True, 1.0, 2.0, 0.7)
    assert last.log_T == last.log_T_avg == mid.log_T_avg and last.log_T != mid.log_T
    assert last.step_size == math.exp(last.da_x_avg) and last.da_x_avg == mid.da_x_avg
    assert last.num_steps == cr.num_steps_of(cr.halton(7), math.exp(last.log_T), last.step_size, 1000)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    """A NUTS kernel and a PerChain metric raise ValueError; with no device everything else raises the engine's
    no-device error, which shows that the ValueErrors came first."""
    import torch
    import aehmc_amd as aa
    from aehmc_amd import chees, targets
    from aehmc_amd.engine import EngineError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    C, D = 3, 2
    state = aa.IntegratorState(torch.zeros(C, D, dtype=torch.float64), None, torch.zeros(C, dtype=torch.float64),
                               torch.zeros(C, D, dtype=torch.float64))
    hmc_kernel = aa.hmc.new_kernel(aa.RandomStream(seeds=range(C)), targets.StdNormal())
    nuts_kernel = aa.nuts.new_kernel(aa.RandomStream(seeds=range(C)), targets.StdNormal())
    per_chain = aa.PerChain(torch.ones(C, D, dtype=torch.float64))
    with pytest.raises(ValueError, match="static HMC kernel"):
        chees.run(nuts_kernel, state, 10)
    with pytest.raises(ValueError, match="static HMC kernel"):
        chees.run(lambda *a: None, state, 10)
    with pytest.raises(ValueError, match="static HMC kernel"):
        chees.sample(nuts_kernel, state, 0.5, 1.0, 2.0, 4)
    with pytest.raises(ValueError, match="PerChain"):
        chees.run(hmc_kernel, state, 10, per_chain)
    with pytest.raises(ValueError, match="PerChain"):
        chees.sample(hmc_kernel, state, 0.5, per_chain, 2.0, 4)
    with pytest.raises(ValueError, match="PerChain"):
        chees.adaptation(10, inverse_mass_matrix=per_chain)
    with pytest.raises(ValueError, match="positive"):
        chees.adaptation(10, initial_trajectory_length=0.0)
    with pytest.raises(ValueError, match="max_num_integration_steps"):
        chees.run(hmc_kernel, state, 10, max_num_integration_steps=0)
    with pytest.raises(ValueError):
        chees.sample(hmc_kernel, state, 0.0, 1.0, 2.0, 4)
    with pytest.raises(EngineError, match="no CPU fallback"):
        chees.run(hmc_kernel, state, 10)
    with pytest.raises(EngineError, match="no CPU fallback"):
        chees.adaptation(10)[0](state)
    assert chees.num_integration_steps(0.5, 3.0, 3) == math.ceil(0.75 * 3.0 / 0.5)
    assert chees.num_integration_steps(0.5, 3.0, 3, jitter=False) == 6 and chees.num_integration_steps(9.0, 1.0, 1) == 1


def test_lib_declares_the_header_of_the_chees_calls():
    from aehmc_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "aehmc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("aehmc_chees_init", "aehmc_chees_update"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
    fields = re.search(r"typedef struct \{([^}]*)\}\s*aehmc_chees_state;", hdr).group(1)
    names = re.findall(r"\*?\s*\**(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.CCheesState._fields_]


def _reference_runs():
    return {name: [list(cr.warmup(SIGMA, imm, C_STAT, STEPS_STAT, seed)) for seed in range(SEEDS)]
            for name, imm in TARGETS.items()}


def test_golden_reference_runs():
    """tests/golden/chees_ref_runs.json: the reference's final (T, eps) of 16 seeds on each statistical target (C = 256,
    800 steps, sigma = linspace(1, 10, 20); identity metric and imm = sigma).  Written when missing.  Checked: its
    shape; that the spread of T is at most 5 % of its mean on each target (the condition under which mean +- 5 sd
    is a sharp test of the device); and that one fresh reference run per target lies within mean +- 5 sd itself
    (the arithmetic of whole warm-ups is chaotic in the last bits, so no bitwise comparison)."""
    if not os.path.exists(GOLDEN):
        with open(GOLDEN, "w") as f:
            json.dump({"C": C_STAT, "num_steps": STEPS_STAT, "sigma": "linspace(1, 10, 20)", "columns": ["T", "eps"],
                       "runs": _reference_runs()}, f, indent=1)
    gold = json.load(open(GOLDEN))
    assert gold["C"] == C_STAT and gold["num_steps"] == STEPS_STAT and set(gold["runs"]) == set(TARGETS)
    for name, imm in TARGETS.items():
        runs = np.array(gold["runs"][name])
        assert runs.shape[0] >= 16 and runs.shape[1] == 2
        mean, sd = runs.mean(0), runs.std(0, ddof=1)
        assert sd[0] / mean[0] <= 0.05, (name, mean, sd)
        fresh = np.array(cr.warmup(SIGMA, imm, C_STAT, STEPS_STAT, 1000))
        assert (np.abs(fresh - mean) <= 5 * sd).all(), (name, fresh, mean, sd)
