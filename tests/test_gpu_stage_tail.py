"""The lock-step NUTS stage kernels' passes behind the main one (slot copy, expansion end, change of direction, outputs,
further U-turn levels, chain start) against outputs RECORDED from the library before those passes were batched:
tests/golden/stage_tail_<case>.npz, written by tools/stage_tail_golden.py (cases, shapes and step sizes are defined
there, once, for the recording and for this test).  Everything is compared byte for byte: position, potential energy,
gradient, momentum, every diagnostic, the acceptance and divergence histories, a digest of all draws, generator states.

C = 6 chains with per-chain step sizes, max_num_expansions = 7, sample(T = 3).  D = 513 leaves one lane's tail in a
four-deep batch, 700 a ragged last batch, 1024 is a multiple of every batch size in use (64 x 4 and 64 x 8); the diagonal
sizes have fewer elements than lanes (5), one per lane (64), one over (65) and a ragged count (300)."""
import functools
import importlib.util
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "stage_tail_golden.py")
_spec = importlib.util.spec_from_file_location("stage_tail_golden", _TOOL)
stg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(stg)


@functools.lru_cache(maxsize=None)
def golden(name):
    return stg.load_golden(name)


def check(name, ahead=1):
    want = golden(name)
    assert not stg.covers(name, want), stg.covers(name, want)  # the recorded case exercises what it is here for
    got = stg.run_case(name, ahead)
    assert not stg.differences(got, want), (name, stg.differences(got, want))


@pytest.mark.parametrize("ahead", [1, 0])
@pytest.mark.parametrize("D", [513, 700, 1024])
def test_whitened_lock_step_equals_recorded_bytes(D, ahead):
    """k_step_white_ahead ("dense_whiten_ahead" 1) and k_step_white (0): nuts_book FUSE 4 and 3.  In the recorded last
    transition the chains make 4 ... 7 doublings (an odd step with five further U-turn levels, more than one sweep
    of four; changes of direction) and some chain ends on a U-turn."""
    check(f"a{D}", ahead)


def test_two_gemm_linear_mode_equals_recorded_bytes():
    """"dense_whiten" 0: the dense-metric instantiations of every pass (velocity and imm g' rows travel with the rest)."""
    check("b513")


@pytest.mark.parametrize("D", [5, 64, 65, 300])
def test_diagonal_lock_step_equals_recorded_bytes(D):
    """Diagonal metric, coordinate-wise target, "resident_nuts" 0: k_nuts_begin_diag and nuts_book FUSE 2; chain 5's step
    size of 3.0 makes it diverge in every transition."""
    check(f"c{D}")
