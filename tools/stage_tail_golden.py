"""Records tests/golden/stage_tail_<case>.npz: what the lock-step NUTS stage kernels give on small problems whose chains
differ in tree depth and direction (tests/test_gpu_stage_tail.py compares a build against them byte for byte).

    python tools/stage_tail_golden.py [--out DIR] # writes every case (run on the build whose outputs are the yardstick)
    python tools/stage_tail_golden.py --check    # runs every case and compares with the committed files

Cases (C = 6 chains, per-chain step sizes, max_num_expansions = 7, sample(T = 3), seeds 300..305):
  a<D>  whitened lock-step, dense-precision MVN + dense metric built as tests/test_gpu_white_ahead.py builds them,
        D = 513, 700, 1024; "dense_whiten_ahead" 1 and 0 give the same bytes (test_gpu_white_ahead.py), so one file
        serves both options
  b513  the same problem in two-GEMM linear mode ("dense_whiten" 0)
  c<D>  diagonal Gaussian + diagonal metric on the lock-step path ("resident_nuts" 0; "fused_nuts" is off by default),
        D = 5, 64, 65, 300
The step sizes were chosen with the C oracle on the CPU (oracle/c_oracle.py, one chain at a time) so that in the LAST
transition some chain makes >= 6 doublings, some chain ends on a U-turn and, in c, some chain diverges; the recording
run asserts the same of what the device returned."""
import functools
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

C, DEPTH, T = 6, 7, 3
SEEDS = [300 + c for c in range(C)]
# name -> (path, D, per-chain step sizes)
CASES = {
    "a513": ("white", 513, (0.035, 0.05, 0.07, 0.1, 0.14, 0.2)),
    "a700": ("white", 700, (0.035, 0.05, 0.07, 0.1, 0.14, 0.2)),
    "a1024": ("white", 1024, (0.035, 0.05, 0.07, 0.1, 0.14, 0.2)),
    "b513": ("linear", 513, (0.035, 0.05, 0.07, 0.1, 0.14, 0.2)),
    "c5": ("diag", 5, (0.02, 0.04, 0.08, 0.15, 0.3, 3.0)),
    "c64": ("diag", 64, (0.02, 0.04, 0.08, 0.15, 0.3, 3.0)),
    "c65": ("diag", 65, (0.02, 0.04, 0.08, 0.15, 0.3, 3.0)),
    "c300": ("diag", 300, (0.02, 0.04, 0.08, 0.15, 0.3, 3.0)),
}


def spd(r, D):
    A = r.normal(size=(D, D))
    m = A @ A.T / D + np.eye(D)
    return 0.5 * (m + m.T)


@functools.lru_cache(maxsize=None)
def dense_problem(D):
    """tests/test_gpu_white_ahead.py: unrelated random SPD precision and metric, a non-zero mu"""
    r = np.random.default_rng(D)
    mu = r.normal(size=D)
    P = np.linalg.inv(spd(r, D))
    P = 0.5 * (P + P.T)
    imm = spd(r, D)
    return mu, P, imm, r.normal(size=(C, D))


@functools.lru_cache(maxsize=None)
def diag_problem(D):
    r = np.random.default_rng(1000 + D)
    return r.normal(size=D), 0.5 + r.random(D), 0.5 + r.random(D), r.normal(size=(C, D))  # mu, sigma, imm, q0


def options(path, ahead=1):
    """engine options of a path, and the ones that put the defaults back"""
    if path == "white":
        return dict(dense_whiten=1, dense_whiten_ahead=ahead), dict(dense_whiten=1, dense_whiten_ahead=1)
    if path == "linear":
        return dict(dense_whiten=0), dict(dense_whiten=1)
    return dict(resident_nuts=0), dict(resident_nuts=2)


def run_case(name, ahead=1):
    """sample(T) of one case on the device: dict of host arrays"""
    import torch
    from aehmc_amd import PerChain, RandomStream, nuts, targets
    from aehmc_amd.engine import get_engine
    path, D, eps = CASES[name]
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")  # noqa: E731
    eng = get_engine()
    on, off = options(path, ahead)
    try:
        for k, v in on.items():
            eng.set_option(k, v)
        if path == "diag":
            mu, sigma, imm, q0 = diag_problem(D)
            tgt = targets.DiagGaussian(mu, sigma)
        else:
            mu, P, imm, q0 = dense_problem(D)
            tgt = targets.DenseMVN(dev(mu), dev(P))
        srng = RandomStream(seeds=SEEDS)
        kernel = nuts.new_kernel(srng, tgt, max_num_expansions=DEPTH)
        state = nuts.new_state(dev(q0), tgt)
        samples, info, acc_hist, div_hist = kernel.sample(state, PerChain(dev(np.asarray(eps))), dev(imm), T)
        s = info.state
        out = dict(q=s.position, U=s.potential_energy, g=s.potential_energy_grad, p=s.momentum,
                   acc=info.acceptance_probability, nl=info.n_leapfrog, nd=info.num_doublings, turn=info.is_turning,
                   div=info.is_diverging, acc_hist=acc_hist, div_hist=div_hist)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        # the earlier draws as a digest (the last one is q itself): a few KB per file
        out["samples_sha256"] = np.frombuffer(hashlib.sha256(samples.cpu().numpy().tobytes()).digest(), dtype=np.uint8)
        out["rng"] = kernel._nuts["holder"]["rng"].cpu().numpy().view(np.uint64).copy()
        return out
    finally:
        for k, v in off.items():
            eng.set_option(k, v)


def covers(name, out):
    """what a case must exercise, on its recorded diagnostics; returns the list of conditions it misses"""
    miss = []
    if not (out["nd"] >= 6).any():  # an odd step with five U-turn levels, direction changes
        miss.append(f"num_doublings >= 6: {out['nd'].tolist()}")
    if not out["turn"].any():
        miss.append(f"is_turning: {out['turn'].tolist()}")
    if CASES[name][0] == "diag" and not out["div"].any():
        miss.append(f"is_diverging: {out['div'].tolist()}")
    return miss


def golden_path(name):
    return os.path.join(GOLDEN, f"stage_tail_{name}.npz")


def load_golden(name):
    with np.load(golden_path(name)) as z:
        return {k: z[k] for k in z.files}


def differences(got, want):
    """keys whose dtype, shape or bytes differ"""
    bad = sorted(set(got) ^ set(want))
    for k in sorted(set(got) & set(want)):
        if got[k].dtype != want[k].dtype or got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes():
            bad.append(k)
    return bad


def main(argv):
    check = "--check" in argv
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    status = 0
    for name in CASES:
        out = run_case(name)
        miss = covers(name, out)
        print(name, "nd", out["nd"].tolist(), "turn", out["turn"].astype(int).tolist(), "div", out["div"].astype(int).tolist(),
              "nl", out["nl"].tolist(), "MISSING " + "; ".join(miss) if miss else "", flush=True)
        if miss:
            status = 1
        if CASES[name][0] == "white":
            off = run_case(name, ahead=0)
            if differences(off, out):
                print(name, "dense_whiten_ahead 0 differs:", differences(off, out), flush=True)
                status = 1
        if check:
            bad = differences(out, load_golden(name))
            print(name, "differs from the committed file: " + ", ".join(bad) if bad else "equal", flush=True)
            status |= 1 if bad else 0
        else:
            np.savez(os.path.join(out_dir, os.path.basename(golden_path(name))), **out)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
