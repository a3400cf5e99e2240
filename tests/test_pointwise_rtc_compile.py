"""CPU-side guard, after tests/test_transforms_rtc_compile.py: the program hipRTC compiles for a pointwise source -- the
mode define, dual.cuh, the traced source, csrc/pointwise.cuh, both FOLD variants of k_pointwise with and without staged
rows -- instantiates under `hipcc -fsyntax-only` for gfx950; so does the precompiled side of the header."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_rtc_sources_compile import CSRC, HIPCC  # noqa: E402

INSTANCES = "".join(f"template __global__ void aehmc::k_pointwise<{fold}, {stage}>(aehmc::PwArgs);\n"
                    for fold in ("false", "true") for stage in ("false", "true"))


def program(traced):
    return ('#define AEHMC_POINTWISE_TARGET 1\n#include "dual.cuh"\n' + traced.source + '#include "pointwise.cuh"\n' + INSTANCES)


def lazy():
    from aehmc_amd import tracing
    r = np.random.default_rng(0)
    X, y, group = r.normal(size=(300, 5)), r.normal(size=300), r.integers(0, 3, size=300)

    def loglik(q):
        w, sigma, mu = q[:5], np.exp(q[5]), q[6:9]
        return -0.5 * ((y - X @ w - mu[group]) / sigma) ** 2 - np.log(sigma) - tracing.softplus(q[9]) * y
    tr = tracing.trace_pointwise(loglik, 10)
    assert tr.n_out == 300 and tr.n_head >= 2 and "switch" not in tr.source
    return program(tr)


def unrolled():
    from aehmc_amd import tracing
    tr = tracing.trace_pointwise(lambda q: [q[:3000].sum(), (q[3000:6000] ** 2).sum(), np.exp(q[8999]) * q[0]], 9000)
    assert tr.n_out == 3 and tr.n_head == 0 and "switch (j)" in tr.source
    return program(tr)


def precompiled():
    return '#define AEHMC_POINTWISE_TU 1\n#include "pointwise.cuh"\n'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("source", [lazy, unrolled, precompiled], ids=["lazy", "unrolled", "precompiled"])
def test_pointwise_program_instantiates(tmp_path, source):
    path = tmp_path / f"{source.__name__}.hip"
    path.write_text(source())
    out = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", CSRC, "--cuda-device-only",
                          "-fsyntax-only", "-Wno-unused-value", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
