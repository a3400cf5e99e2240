#!/usr/bin/env python3
"""Acceptance quantities of the eigen route ("dense_eigen"), as aehmc_white_basis_info reports them: numpy's
eigh (supplied) and the solver at D = 513 and 700, each with random SPD matrices and with imm = P^-1; with --c3 also
the solver at the benchmark's shape, with the wall time of its first three transitions.
usage: eigen_basis_probe.py [--c3]   (profiles/eigen/basis_measurements.txt)"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from aehmc_amd import RandomStream, nuts, targets  # noqa: E402
from aehmc_amd.engine import get_engine  # noqa: E402

eng = get_engine()
dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def spd(r, D):
    A = r.normal(size=(D, D))
    m = A @ A.T / D + np.eye(D)
    return 0.5 * (m + m.T)


def one(D, degenerate, supplied):
    r = np.random.default_rng(D)
    mu = r.normal(size=D)
    cov = spd(r, D)
    P = np.linalg.inv(cov)
    P = 0.5 * (P + P.T)
    imm = cov if degenerate else spd(r, D)
    q0 = r.normal(size=(6, D))
    eng.set_option("dense_eigen", 2)
    if supplied:
        L = np.linalg.cholesky(imm)
        H = L.T @ P @ L
        lam, V = np.linalg.eigh(0.5 * (H + H.T))
        eng.set_white_basis(dev(V), dev(lam))
    else:
        eng.set_white_basis(None)
    tgt = targets.DenseMVN(dev(mu), dev(P))
    k = nuts.new_kernel(RandomStream(seeds=list(range(6))), tgt, max_num_expansions=6)
    info, _ = k(nuts.new_state(dev(q0), tgt), 0.12, dev(imm))
    torch.cuda.synchronize()
    print(f"D={D} degenerate={degenerate} supplied={supplied}", eng.white_basis_info(), "nd", info.num_doublings.cpu().numpy(), flush=True)


for D in (513, 700):
    for deg in (False, True):
        for sup in (True, False):
            one(D, deg, sup)
eng.set_white_basis(None)
eng.set_option("dense_eigen", 1)

if "--c3" in sys.argv:
    from bench import build_c3
    D, C = 10_000, 4096
    device = torch.device("cuda")
    Sigma, P = build_c3(D, device)
    tgt = targets.DenseMVN(torch.zeros(D, dtype=torch.float64, device=device), P)
    q0 = np.random.default_rng(1234).standard_normal((C, D))
    k = nuts.new_kernel(RandomStream(seeds=[1000 + c for c in range(C)]), tgt, max_num_expansions=10)
    state = nuts.new_state(torch.as_tensor(q0, device=device), tgt)
    eps = 0.5 * D ** -0.25
    for t in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info, _ = k(state, eps, Sigma)
        torch.cuda.synchronize()
        print(f"c3 step {t}: {(time.perf_counter() - t0) * 1e3:.1f} ms", eng.white_basis_info(),
              "leapfrogs", int(info.n_leapfrog.sum()), flush=True)
        state = info.state._replace(momentum=None)
