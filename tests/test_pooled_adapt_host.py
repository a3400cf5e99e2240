"""CPU-side checks of pooled window adaptation: the numpy restatement (tests/pooled_adapt_ref.py) against np.cov on the
stacked draws, the new C-ABI symbols, and the no-device error of ``run(pooled=True)``."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pooled_adapt_ref as pr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("aehmc_pooled_adapt_init", "aehmc_pooled_adapt_update", "aehmc_syrk_tn", "aehmc_nuts_warmup_pooled",
               "aehmc_hmc_warmup_pooled")


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("C,D,num_steps", [(1, 4, 150), (6, 5, 151), (3, 1, 300), (5, 3, 64)])
def test_reference_windows_equal_np_cov_of_the_stacked_draws(full, C, D, num_steps):
    """Chan's batch update, step by step, gives at every window end the shrunk np.cov (ddof 1) of ALL draws of that
    window stacked -- odd and even window lengths (151 / 150 steps: 26 / 25; 300: 25 + 150; 64: the short schedule's
    49) and C = 1."""
    r = np.random.default_rng(100 * C + D + num_steps)
    A = r.normal(size=(D, D)) + 2 * np.eye(D)
    schedule = pr.build_schedule(num_steps)
    assert len(schedule) == num_steps
    s = pr.init(D, full, 0.5)
    assert s.step_size == 1.0 and s.mu == 0.5
    window, ends = [], 0
    for i, (stage, wend) in enumerate(schedule):
        X = r.normal(size=(C, D)) @ A + 3.0
        s = pr.update(s, stage, wend, i == num_steps - 1, X, r.random(C))
        if stage:
            window.append(X)
        assert s.n == (0 if wend or not window else C * len(window))
        if wend:
            stacked = np.concatenate(window)
            n = stacked.shape[0]
            cov = np.atleast_2d(np.cov(stacked.T, ddof=1))
            want = pr.shrink(cov if full else np.diag(cov), n, full)
            np.testing.assert_allclose(s.imm, want, rtol=1e-10)
            S = s.sqrt_mass
            if full:
                np.testing.assert_allclose(S.T @ s.imm @ S, np.eye(D), atol=1e-10)
                assert np.array_equal(S, np.triu(S))
            else:
                np.testing.assert_allclose(S * S * s.imm, np.ones(D), rtol=1e-14)
            assert s.step == 1 and s.x == 0.0 and s.mu == s.step_size and not s.m2.any() and not s.mean.any()
            window, ends = [], ends + 1
    assert ends >= 1 and s.step_size == float(np.exp(s.x_avg))


def test_reference_with_one_chain_is_the_per_chain_adaptation():
    """C = 1: the pooled restatement and the per-chain one (oracle/np_adaptation.py) differ in rounding only."""
    from oracle import np_adaptation as na
    D, num_steps = 5, 150
    r = np.random.default_rng(3)
    init, update = na.window_adaptation(num_steps, True, 0.3)
    ws, params = init(np.zeros(D))
    s = pr.init(D, True, 0.3)
    for i, (stage, wend) in enumerate(pr.build_schedule(num_steps)):
        x, a = r.normal(size=D) * (1 + np.arange(D)), r.random()
        ws, params = update(i, ws, params, x, a)
        s = pr.update(s, stage, wend, i == num_steps - 1, x[None], np.array([a]))
        assert s.step_size == pytest.approx(params[0], rel=1e-12)
        np.testing.assert_allclose(s.imm, params[1], rtol=1e-11)
    assert pr.build_schedule(num_steps) == na.build_schedule(num_steps)


def test_library_exports_the_pooled_symbols():
    from aehmc_amd import _lib
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None


def test_lib_declares_the_header_argument_counts():
    from aehmc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aehmc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name
    fields = re.search(r"typedef struct \{([^}]*)\}\s*aehmc_pooled_adapt_state;", hdr).group(1)
    names = re.findall(r"\*?\s*\**(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in _lib.CPooledAdaptState._fields_]


def test_pooled_run_without_a_device_raises_the_no_device_error(monkeypatch):
    import torch
    from aehmc_amd import window_adaptation
    from aehmc_amd.engine import EngineError
    from aehmc_amd.integrators import IntegratorState
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    state = IntegratorState(torch.zeros(3, 2, dtype=torch.float64), None, torch.zeros(3, dtype=torch.float64),
                            torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(EngineError, match="no CPU fallback"):
        window_adaptation.run(lambda *a: None, state, 30, pooled=True)
    with pytest.raises(EngineError, match="no CPU fallback"):
        window_adaptation.window_adaptation(30, pooled=True)[0](state)
