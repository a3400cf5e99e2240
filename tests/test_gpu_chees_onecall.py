"""chees.run as ONE engine call (aehmc_chees_warmup: the transition takes its length from the adaptation state on the
device) against the hand-driven ``chees.adaptation`` loop, bit for bit, on the HMC routes ChEES runs on."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_chees import ROUTES, _dev, _diag_gaussian_kernel  # noqa: E402


def _problem(route):
    C, D, dense, _ = ROUTES[route]
    r = np.random.default_rng(D)
    if dense:
        A = r.normal(size=(D, D)) / (4 * math.sqrt(D))
        imm = _dev(np.eye(D) + (A + A.T) / 2)
    else:
        imm = _dev(1.0 + 0.2 * r.random(D))
    return (lambda: _diag_gaussian_kernel(C, np.linspace(1.0, 2.0, D), seed0=7)), imm, C


def _hand_driven(make, imm, C, n, **options):
    """The loop of the ``chees.adaptation`` docstring.  Returns (state, CheesState, step size [C], lengths run, n_leapfrog
    of the last transition, generator states)."""
    from aehmc_amd import chees
    kernel, state = make()
    init, update = chees.adaptation(n, inverse_mass_matrix=imm, **options)
    cs, (eps, L) = init(state)
    lengths, info, updates = [], None, None
    for i in range(n):
        before = state.position
        lengths.append(L)
        info, updates = kernel(state, eps, imm, L)
        state = info.state._replace(momentum=None)
        accepted = (state.position != before).reshape(C, -1).any(1)
        cs, (eps, L) = update(i, cs, before, info, accepted)
    (rng,) = updates.values()
    return state, cs, eps.value, lengths, info.n_leapfrog, rng


def _assert_run_equals_loop(make, imm, C, n, **options):
    from aehmc_amd import chees
    state, cs, eps, lengths, n_leap, rng = _hand_driven(make, imm, C, n, **options)
    kernel, state0 = make()
    opts = dict(initial_step_size=1.0, initial_trajectory_length=None, target_acceptance_rate=0.651, learning_rate=0.025,
                max_num_integration_steps=1000)
    opts.update(options)
    last, (step_size, imm_out, T), updates, got, out = chees._run(kernel, state0, n, imm, **opts)
    assert torch.equal(last.position, state.position) and torch.equal(last.potential_energy, state.potential_energy)
    assert torch.equal(last.potential_energy_grad, state.potential_energy_grad)
    assert step_size == float(eps[0]) and T == math.exp(float(cs.log_trajectory_length)) and imm_out is imm
    for name in ("step", "log_trajectory_length", "log_trajectory_length_avg", "adam_m", "adam_v", "halton_weight",
                 "num_steps", "step_size"):
        assert torch.equal(getattr(got, name), getattr(cs, name)), name
    for a, b in zip(got.da_state, cs.da_state):
        assert torch.equal(a, b)
    (got_rng,) = updates.values()
    assert torch.equal(got_rng, rng)
    assert torch.equal(out["n_leapfrog"], n_leap.reshape(-1)) and (out["n_leapfrog"] == lengths[-1]).all()
    # the public entry point returns the first three of these
    kernel2, state2 = make()
    pub = chees.run(kernel2, state2, n, imm, **options)
    assert len(pub) == 3 and torch.equal(pub[0].position, state.position) and pub[1][0] == step_size and pub[1][2] == T
    return lengths, out


@pytest.mark.timeout(120)
@pytest.mark.parametrize("route", list(ROUTES))
def test_run_is_the_hand_driven_loop(route):
    make, imm, C = _problem(route)
    lengths, _ = _assert_run_equals_loop(make, imm, C, 12, initial_trajectory_length=6.0, max_num_integration_steps=64)
    print(f"{route}: lengths {lengths}")
    assert len(set(lengths)) >= 3, "input condition: num_steps takes at least three values"


@pytest.mark.timeout(120)
@pytest.mark.parametrize("route", ["fused", "lock_step"])
def test_max_num_integration_steps_caps_every_transition(route):
    """A large initial trajectory length: the state's first num_steps is far above the cap (init applies none), and no
    transition may run more than 2 leapfrogs."""
    make, imm, C = _problem(route)
    lengths, out = _assert_run_equals_loop(make, imm, C, 5, initial_trajectory_length=500.0, max_num_integration_steps=2)
    assert max(lengths) <= 2 and lengths[0] == 2
    assert (out["n_leapfrog"] <= 2).all()
