"""The host code that drives the samplers -- the kernels' ``sample(..., into=)``, the ``(init, update)`` pairs of the
warm-up and ``window_adaptation.run`` on a scalar position -- at the smallest shapes that still take every branch:
3 chains (not a multiple of the 4 chains per workgroup), 5 coordinates, and a warm-up of 25 steps, the shortest
with a fast buffer (3 steps), a slow window (20, its end at step 22) and a final buffer (2)."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

C, D, NUM_STEPS = 3, 5, 25


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _problem(seed):
    from aehmc_amd import targets
    r = np.random.default_rng(seed)
    return targets.DiagGaussian(r.normal(size=D), 0.5 + r.random(D)), r.normal(size=(C, D)), 0.5 + r.random(D)


def _kernel(kind, srng, tgt):
    """(kernel, new_state, the trajectory length as positional arguments, the same as keyword arguments, the kernel's
    settings dict) -- five items"""
    from aehmc_amd import hmc, nuts
    if kind == "nuts":
        k = nuts.new_kernel(srng, tgt, max_num_expansions=5)
        return k, nuts.new_state, (), {}, k._nuts
    k = hmc.new_kernel(srng, tgt)
    return k, hmc.new_state, (3,), {"num_integration_steps": 3}, k._hmc


def test_schedule_of_25_steps_has_every_stage():
    from aehmc_amd import window_adaptation
    assert window_adaptation.build_schedule(NUM_STEPS) == [(0, False)] * 3 + [(1, False)] * 19 + [(1, True)] + [(0, False)] * 2


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_sample_into_a_buffer_equals_sample(kind):
    """``sample(..., into=buf)`` writes the draws to the head of ``buf`` and is otherwise the call without ``into``:
    draws, histories, final state and generator states are identical; an unfit buffer is refused."""
    from aehmc_amd import RandomStream
    tgt, q0, imm = _problem(1)
    n = 4
    outs = []
    for use_buffer in (False, True):
        kernel, new_state, length, _, settings = _kernel(kind, RandomStream(seeds=[70 + c for c in range(C)]), tgt)
        buf = torch.full((n * C * D + 7,), -1.0, dtype=torch.float64, device="cuda") if use_buffer else None
        samples, info, acc, div = kernel.sample(new_state(_dev(q0), tgt), 0.3, imm, *length, n, into=buf)
        assert samples.shape == (n, C, D)
        if use_buffer:
            assert samples.data_ptr() == buf.data_ptr()
            assert torch.equal(buf[:n * C * D].reshape(n, C, D), samples) and (buf[n * C * D:] == -1.0).all()
        outs.append((samples.clone(), acc, div, info.state.position, info.state.potential_energy,
                     info.state.potential_energy_grad, info.acceptance_probability, info.n_leapfrog,
                     settings["holder"]["rng"].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][0][-1], outs[0][3])  # (the last draw is the final position)

    kernel, new_state, length, _, _ = _kernel(kind, RandomStream(seeds=[70 + c for c in range(C)]), tgt)
    state = new_state(_dev(q0), tgt)
    for bad in (torch.empty(n * C * D - 1, dtype=torch.float64, device="cuda"),
                torch.empty(n * C * D, 2, dtype=torch.float64, device="cuda")[:, 0],
                torch.empty(n * C * D, dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError, match="samples buffer must be a contiguous float64 tensor"):
            kernel.sample(state, 0.3, imm, *length, n, into=bad)


@pytest.mark.parametrize("full", [False, True])
def test_pooled_init_update_states_are_values(full):
    """Every ``update`` of the pooled pair works on copies: after the whole warm-up -- fast steps, slow steps, the window
    end that rewrites the metric, the last step that averages the step size -- each earlier WarmupState still holds the
    step size, metric and dual-averaging step it was returned with."""
    from aehmc_amd import RandomStream, nuts, window_adaptation
    tgt, q0, _ = _problem(2)
    kernel = nuts.new_kernel(RandomStream(seeds=[40 + c for c in range(C)]), tgt, max_num_expansions=5)
    state = nuts.new_state(_dev(q0), tgt)
    init, update = window_adaptation.window_adaptation(NUM_STEPS, is_mass_matrix_full=full, pooled=True)
    ws, params = init(state)
    assert ws.imm.shape == ((D, D) if full else (D,)) and ws.step_size.shape == (C,)
    seen = []
    for i in range(NUM_STEPS):
        seen.append((ws, ws.step_size.clone(), ws.imm.clone(), ws.sqrt_mass.clone(), ws.da_state.step.clone()))
        info, _ = kernel(state, *params)
        state = info.state._replace(momentum=None)
        ws, params = update(i, ws, params, info)
    for i, (old, eps, imm, sqrt_mass, da_step) in enumerate(seen):
        assert torch.equal(old.step_size, eps) and torch.equal(old.imm, imm) and torch.equal(old.sqrt_mass, sqrt_mass), i
        assert torch.equal(old.da_state.step, da_step), i
    assert seen[0][0].da_state.step.tolist() != seen[1][0].da_state.step.tolist()  # (and the counter does move)
    assert not torch.equal(seen[22][2], seen[23][2])  # (the window end at step 22 did write a new metric)
    assert not torch.equal(ws.step_size, seen[-1][1])


@pytest.mark.parametrize("pooled", [False, True])
def test_update_refuses_a_position_of_another_shape(pooled):
    from aehmc_amd import nuts, window_adaptation
    tgt, q0, _ = _problem(3)
    state = nuts.new_state(_dev(q0), tgt)
    init, update = window_adaptation.window_adaptation(NUM_STEPS, pooled=pooled)
    ws, params = init(state)
    for other in (q0[:, :4], q0[:2], q0[0]):
        info = types.SimpleNamespace(state=types.SimpleNamespace(position=_dev(other)),
                                     acceptance_probability=torch.ones(C, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError, match="position has shape"):
            update(0, ws, params, info)


@pytest.mark.parametrize("kind", ["nuts", "hmc"])
def test_pooled_warmup_of_a_scalar_position_fused_equals_step_by_step(kind):
    """One unbatched chain with a ``()`` position: ``run(pooled=True)`` in one engine call and step by step agree bit for
    bit in position, step size, metric and generator states; the step size is a float, the metric 0-d."""
    from aehmc_amd import RandomStream, targets, window_adaptation
    tgt = targets.StdNormal()
    outs = []
    for fused in (True, False):
        srng = RandomStream(seed=11)
        kernel, new_state, _, length, settings = _kernel(kind, srng, tgt)
        state, (eps, imm), updates = window_adaptation.run(kernel, new_state(0.5, tgt), NUM_STEPS, pooled=True,
                                                           fused=fused, **length)
        assert isinstance(eps, float) and isinstance(imm, torch.Tensor) and imm.shape == ()
        assert state.position.shape == () and updates[srng] is settings["holder"]["rng"]
        outs.append((state.position, state.potential_energy, state.potential_energy_grad, torch.tensor(eps), imm,
                     updates[srng].clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.isfinite(outs[0][0]).all() and outs[0][3].item() > 0 and outs[0][4].item() > 0
