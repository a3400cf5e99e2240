"""Traced joint densities above 2048 coordinates, CPU side: the limits of targets.CustomJoint (up to 10176 coordinates with
a reverse-mode program, 2048 without) and the run-time compiled kernels that sample them -- the AEHMC_T_JOINT
instantiations of the workgroup-per-chain NUTS / HMC kernels (nuts_wide.cuh, hmc_fused.cuh) and the workgroup-per-chain
evaluation kernel of new_state and the lock-step path (engine.cuh k_target_joint_wg) -- instantiated against traced
programs by the offline compiler (`hipcc -fsyntax-only`, device pass), as tests/test_rtc_sources_compile.py does for the
other families."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aehmc_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
JOINT_T = 7  # include/aehmc_hip.h AEHMC_T_JOINT


def funnel(q):
    v, x = q[0], q[1:]
    return -v * v / 18.0 + (-0.5 * x * x * np.exp(-v) - 0.5 * v).sum()


G, N = 50, 200
_r = np.random.default_rng(3)
GROUP = _r.integers(0, G, size=N)
YOBS = _r.normal(size=N)


def gather_model(q):
    """random intercepts: q = [mu, log sigma, a_1..a_G], y_n ~ N(mu + a_{g(n)}, 1), a_g ~ N(0, sigma^2) -- a gather of
    the position by a data index (its adjoints are AEHMC_ATOMIC_ADD into the gradient row)"""
    mu, ls, a = q[0], q[1], q[2:]
    r = YOBS - mu - a[GROUP]
    return -0.5 * mu * mu - 0.5 * ls * ls + (-0.5 * a * a * np.exp(-2.0 * ls) - ls).sum() + (-0.5 * r * r).sum()


@pytest.mark.parametrize("D", [2049, 4096, 10000, 10176])
def test_traced_joint_density_above_2048_coordinates(D):
    from aehmc_amd import targets
    tgt = targets.from_callable(funnel, D)
    assert isinstance(tgt, targets.CustomJoint) and tgt.dim == D
    assert "#define AEHMC_JOINT_GRAD 1" in tgt.source


def test_joint_density_limits():
    from aehmc_amd import targets
    with pytest.raises(ValueError, match="10176"):
        targets.from_callable(funnel, 10177)
    src = targets.from_callable(funnel, 4096)
    with pytest.raises(ValueError, match="10176"):
        targets.CustomJoint(src.user_source, 10177, grad_source="#define AEHMC_JOINT_GRAD 1\n")
    # a density without a reverse-mode program keeps the forward-mode limit (and its message)
    with pytest.raises(ValueError, match="dim <= 2048"):
        targets.CustomJoint(src.user_source, dim=2049)
    with pytest.raises(ValueError, match="dim <= 2048"):
        targets.from_callable(funnel, 2049, reverse=False)
    assert targets.CustomJoint(src.user_source, dim=2048).dim == 2048


def _source(tgt, kernels):
    return ("#define AEHMC_JOINT_TARGET 1\n" + tgt.source + '#include "engine.cuh"\n#include "nuts_wide.cuh"\n'
            '#include "hmc_fused.cuh"\n' + "".join(k + ";\n" for k in kernels))


def wide_kernels():
    out = ["template __global__ void aehmc::k_target_joint_wg<8>(aehmc::EngineArgs, const double *, double *, double *, int, "
           "const int *, const int *)"]
    for R in (8, 16, 20):
        out.append(f"template __global__ void aehmc::k_nuts_wide<512, {R}, true, {JOINT_T}>(aehmc::EngineArgs)")
        out.append(f"template __global__ void aehmc::k_hmc_wide<512, {R}, {JOINT_T}, false>(aehmc::HmcFusedArgs, const double *, int)")
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("model", ["funnel", "gather"])
def test_wide_joint_kernels_instantiate_against_a_traced_program(tmp_path, model):
    from aehmc_amd import targets
    tgt = targets.from_callable(funnel, 4096) if model == "funnel" else targets.from_callable(gather_model, G + 2)
    assert isinstance(tgt, targets.CustomJoint) and "#define AEHMC_JOINT_GRAD 1" in tgt.source
    if model == "gather":
        assert "AEHMC_ATOMIC_ADD" in tgt.source
    path = tmp_path / f"{model}.hip"
    path.write_text(_source(tgt, wide_kernels()))
    out = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", CSRC, "--cuda-device-only",
                          "-fsyntax-only", "-Wno-unused-value", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]

