"""CPU-side guard for the run-time compiled copies of k_ghmc_fused (csrc/ghmc_fused.cuh), in the manner of
tests/test_rtc_sources_compile.py: the kernel is instantiated against a targets.Custom source and against a traced joint
density with its reverse-mode program by the offline compiler, at the smallest and the largest R -- a header edit that
breaks the AEHMC_T_CUSTOM / AEHMC_T_JOINT paths is caught without a GPU.  The sources are assembled as the engine's
rtc_function assembles them: mode macro, the user's source, engine.cuh, the family header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aehmc_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def custom_source():
    from aehmc_amd import targets
    tgt = targets.Custom('''template <class T> __device__ T aehmc_logp(T q, long long i, const double *const *prm) {
                              const double s = prm[0][i];
                              return -0.5 * (q / s) * (q / s);
                            }''', params=[[1.0]])
    return ("#define AEHMC_CUSTOM_TARGET 1\n" + tgt.source + '\n#include "engine.cuh"\n#include "ghmc_fused.cuh"\n'
            "template __global__ void aehmc::k_ghmc_fused<1, 5>(aehmc::GhmcArgs);\n"
            "template __global__ void aehmc::k_ghmc_fused<16, 5>(aehmc::GhmcArgs);\n")


def joint_source():
    import numpy as np
    from aehmc_amd import targets

    def funnel(q):
        v, x = q[0], q[1:]
        return -v * v / 18.0 + (-0.5 * x * x * np.exp(-v) - 0.5 * v).sum()

    tgt = targets.from_callable(funnel, 100)
    assert isinstance(tgt, targets.CustomJoint) and "#define AEHMC_JOINT_GRAD 1" in tgt.source
    return ("#define AEHMC_JOINT_TARGET 1\n" + tgt.source + '\n#include "engine.cuh"\n#include "ghmc_fused.cuh"\n'
            "template __global__ void aehmc::k_ghmc_fused<1, 7>(aehmc::GhmcArgs);\n"
            "template __global__ void aehmc::k_ghmc_fused<16, 7>(aehmc::GhmcArgs);\n")


def test_target_kinds_are_the_ones_the_names_spell():
    from aehmc_amd import targets
    assert (targets.T_CUSTOM, targets.T_JOINT) == (5, 7)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("source", [custom_source, joint_source], ids=["custom", "traced_joint"])
def test_ghmc_kernel_instantiates_against_a_user_density(tmp_path, source):
    path = tmp_path / "ghmc.hip"
    path.write_text(source())
    out = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", CSRC, "--cuda-device-only",
                          "-fsyntax-only", "-Wno-unused-value", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
