"""CPU-side guard, after tests/test_rtc_sources_compile.py: the source traced from a ``transforms.Model`` that mixes all
six kinds (forward-mode template and reverse-mode program, as targets.CustomJoint hands them over) instantiates the kernel
families under `hipcc -fsyntax-only` for gfx950; so does the per-coordinate form of a coordinate-wise model."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_rtc_sources_compile import CSRC, ELEMENTWISE, HIPCC, traced_program  # noqa: E402


def mixed_model():
    from aehmc_amd import transforms as tf
    a = np.linspace(0.5, 3.0, 26)

    def logprob(w, sigma, ub, rho, mu, pi):
        return (-0.5 * np.sum(w * w) + np.sum(2.0 * np.log(sigma) - 2.0 * sigma) - 0.5 * np.sum(ub * ub)
                + np.sum(np.log(rho - 1.0) + 2.0 * np.log(4.0 - rho)) - 0.5 * np.sum(mu * mu) / 100.0 + np.sum(a * np.log(pi)))

    return tf.Model({"w": tf.Real(20), "sigma": tf.LowerBound(np.linspace(0.0, 1.0, 10), 10), "ub": tf.UpperBound(2.0, 5),
                     "rho": tf.Interval(1.0, 4.0, 10), "mu": tf.Ordered(30), "pi": tf.Simplex(26)}, logprob)


def joint():
    model = mixed_model()
    assert (model.dim, model.constrained_dim) == (100, 101)
    return traced_program(model)


def elementwise():
    """the source of a coordinate-wise model (targets.Custom) in place of the hand-written density of ELEMENTWISE"""
    from aehmc_amd import targets, transforms as tf
    model = tf.Model({"s": tf.Interval(np.linspace(-1.0, 0.0, 7), 2.0, 7)}, lambda s: np.sum(2.0 * np.log1p(s * s) - s))
    tgt = targets.from_callable(model, 7)
    assert isinstance(tgt, targets.Custom)
    head, tail = ELEMENTWISE.split('#include "dual.cuh"\n')
    return head + tgt.source + tail[tail.index('#include "engine.cuh"'):]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("source", [joint, elementwise], ids=["joint", "elementwise"])
def test_kernel_templates_instantiate_against_a_traced_model(tmp_path, source):
    path = tmp_path / f"{source.__name__}.hip"
    path.write_text(source())
    out = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", CSRC, "--cuda-device-only",
                          "-fsyntax-only", "-Wno-unused-value", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
