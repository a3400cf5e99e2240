"""CPU-side checks of the per-transition trajectory lengths: how ``kernel.sample`` reads its ``num_integration_steps``
argument, and that the kernel instantiations which read the lengths from device memory compile against a user density
(`hipcc -fsyntax-only`, device pass) beside the launch-constant ones, whose names stay what they were."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aehmc_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_trajectory_lengths_argument():
    torch = pytest.importorskip("torch")
    from aehmc_amd._common import trajectory_lengths as tl
    assert tl(5, 3) is None and tl(np.int64(5), 3) is None and tl(torch.tensor(5), 3) is None
    assert tl([3, 0, 7], 3) == [3, 0, 7] and tl((3, 0, 7), 3) == [3, 0, 7]
    assert tl(np.array([3, 0, 7], dtype=np.int32), 3) == [3, 0, 7]
    assert tl(torch.tensor([3, 0, 7]), 3) == [3, 0, 7] and tl(np.array([3.0, 1.0]), 2) == [3, 1]
    assert all(type(v) is int for v in tl(np.array([3, 0, 7]), 3))
    for bad, n in (([3, 1], 3), ([3, -1, 2], 3), (np.array([3.5, 1.0]), 2), (np.zeros((2, 2), dtype=int), 2),
                   (torch.tensor([1.0, 2.0]), 2), ([], 0 + 1)):
        with pytest.raises(ValueError):
            tl(bad, n)


def test_chees_trajectory_lengths():
    pytest.importorskip("torch")
    from aehmc_amd import chees
    got = chees.trajectory_lengths(0.37, 2.9, 6, first=3)
    assert got == [chees.num_integration_steps(0.37, 2.9, 3 + i) for i in range(6)] and min(got) >= 1
    assert chees.trajectory_lengths(0.37, 2.9, 4, jitter=False) == [8] * 4


SOURCE = r'''
#define AEHMC_CUSTOM_TARGET 1
#include "dual.cuh"
template <class T> __device__ T aehmc_logp(T q, long long i, const double *const *prm) {
  const double nu = prm[0][i];
  return -0.5 * (nu + 1.0) * log1p(q * q / nu);
}
__device__ void aehmc_custom_elem(double q, long long i, const double *const *prm, double &u, double &g) {
  const aehmc::Dual r = aehmc_logp(aehmc::Dual(q, 1.0), i, prm);
  u = -r.v;
  g = -r.d;
}
#include "engine.cuh"
#include "hmc_fused.cuh"
#include "nuts_block_reg.cuh"
template __global__ void aehmc::k_hmc_fused<2, 5, false, true>(aehmc::HmcFusedArgs);
template __global__ void aehmc::k_hmc_fused<2, 5, true, true>(aehmc::HmcFusedArgs);
template __global__ void aehmc::k_hmc_wide<256, 8, 5, false>(aehmc::HmcFusedArgs, const double *, int);
template __global__ void aehmc::k_hmc_block_reg<2, false, true>(aehmc::EngineArgs, aehmc::HmcSampleArgs);
template __global__ void aehmc::k_hmc_block_dense<false, true>(aehmc::EngineArgs, aehmc::HmcSampleArgs);
template __global__ void aehmc::k_hmc_fused_dense<true, false, false, true>(aehmc::EngineArgs, aehmc::HmcSampleArgs);
// the launch-constant kernels: LS left at its default, the names they always had
template __global__ void aehmc::k_hmc_block_reg<2, false>(aehmc::EngineArgs, aehmc::HmcSampleArgs);
template __global__ void aehmc::k_hmc_fused_dense<true, false, false>(aehmc::EngineArgs, aehmc::HmcSampleArgs);
'''


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_length_reading_instantiations_compile_against_a_user_density(tmp_path):
    path = tmp_path / "lengths.hip"
    path.write_text(SOURCE)
    out = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", CSRC, "--cuda-device-only",
                          "-fsyntax-only", "-Wno-unused-value", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-4000:]
