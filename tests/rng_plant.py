"""Planted PCG64 states: generator states whose k-th raw output is a chosen 64-bit word.

PCG64's step s' = s * MULT + inc (mod 2^128) is invertible, and its XSL-RR output function is onto for
every value of the upper state word, so a state can be built backwards from the word it is to emit: a
ziggurat tail draw in lane 63 of a wave, a wedge test in lane 62, a uniform 16 ulps from a boundary.  The
rare paths of aehmc_amd/csrc/rng.cuh are reached by construction instead of by volume.

Plain Python integers and numpy only (no torch, no GPU).  Everything random is drawn from a seeded
``random.Random``, so the case tables built from these helpers are fixed data."""
import os
import random
import re

import numpy as np

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MULT = (2549297995355413924 << 64) | 4865540595714422341
MINV = pow(MULT, -1, 1 << 128)
RABS_END = 1 << 52


def _read_tables():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "aehmc_ziggurat_tables.h")
    text = open(path).read().replace("\\\n", " ")
    out = {}
    for name in ("KI", "WI", "FI"):
        body = re.search(r"#define AEHMC_ZIG_%s_VALUES(.*)" % name, text).group(1)
        toks = [t.strip() for t in body.split(",") if t.strip()]
        assert len(toks) == 256, (name, len(toks))
        out[name] = toks
    ki = [int(t.rstrip("UL"), 16) for t in out["KI"]]
    wi = np.array([float.fromhex(t) for t in out["WI"]])
    fi = np.array([float.fromhex(t) for t in out["FI"]])
    r = float(re.search(r"#define AEHMC_ZIG_NOR_R (\S+)", text).group(1))
    inv_r = float(re.search(r"#define AEHMC_ZIG_NOR_INV_R (\S+)", text).group(1))
    return ki, wi, fi, r, inv_r


KI, WI, FI, NOR_R, NOR_INV_R = _read_tables()


# ------------------------------------------------------------------ the generator
def step(s, inc):
    return (s * MULT + inc) & M128


def back_step(s, inc):
    return ((s - inc) * MINV) & M128


def rotl64(x, r):
    r &= 63
    return ((x << r) | (x >> ((64 - r) & 63))) & M64 if r else x


def output(s):
    """XSL-RR of a state (the value numpy returns AFTER stepping to this state)."""
    hi, lo = s >> 64, s & M64
    x, rot = hi ^ lo, hi >> 58
    return ((x >> rot) | (x << ((64 - rot) & 63))) & M64 if rot else x


def random_inc(rnd):
    return rnd.getrandbits(128) | 1


def state_with_output(raw, rnd):
    hi = rnd.getrandbits(64)
    lo = rotl64(raw, hi >> 58) ^ hi
    return (hi << 64) | lo


def plant(raw, k, inc, rnd):
    """A state whose output at stream position k (0-based: the (k+1)-th value drawn from it) is `raw`."""
    s = state_with_output(raw, rnd)
    for _ in range(k + 1):
        s = back_step(s, inc)
    return s


# ------------------------------------------------------------------ raw words (bit layout of zig_fast)
def _zig_raw(idx, rabs, rnd):
    return (rnd.getrandbits(3) << 61) | (rabs << 9) | (rnd.getrandbits(1) << 8) | idx


def tail_raw(rnd):
    """Fails the fast test in layer 0: the tail loop."""
    return _zig_raw(0, rnd.randrange(KI[0], RABS_END), rnd)


def wedge_raw(rnd, j=None):
    """Fails the fast test in layer j in [1, 255]: the wedge test, which takes one more uniform."""
    if j is None:
        j = rnd.randrange(1, 256)
    return _zig_raw(j, rnd.randrange(KI[j], RABS_END), rnd)


def uniform_raw(u_int, rnd):
    """A word from which pcg_next_double returns u_int * 2^-53."""
    assert 0 <= u_int < (1 << 53)
    return (u_int << 11) | rnd.getrandbits(11)


# ------------------------------------------------------------------ numpy side and packing
def numpy_generator(state, inc):
    bg = np.random.PCG64(0)
    bg.state = {"bit_generator": "PCG64", "state": {"state": int(state), "inc": int(inc)}, "has_uint32": 0, "uinteger": 0}
    return np.random.Generator(bg)


def generator_state(gen):
    return gen.bit_generator.state["state"]["state"]


def pack(state, inc):
    return [state >> 64, state & M64, inc >> 64, inc & M64]


def pack_sites(sites):
    """[[(state, inc), ...sites] ...chains] -> uint64 [C, n_sites, 4], the layout of oracle.c_oracle.site_states."""
    return np.array([[pack(s, i) for (s, i) in chain] for chain in sites], dtype=np.uint64)


def unpack_state(words):
    return (int(words[0]) << 64) | int(words[1])


# ------------------------------------------------------------------ case tables
NORMAL_POSITIONS = list(range(64)) + [64, 126, 127]
NORMAL_SIZES = list(range(1, 72)) + list(range(126, 131))
NORMAL_REPLICATES = 2


def normal_cases(seed=20240611, positions=NORMAL_POSITIONS, replicates=NORMAL_REPLICATES):
    """(kind, k, state, inc) for kind in tail / wedge, every planted position, `replicates` times."""
    rnd = random.Random(seed)
    cases = []
    for kind, make in (("tail", tail_raw), ("wedge", wedge_raw)):
        for k in positions:
            for _ in range(replicates):
                inc = random_inc(rnd)
                cases.append((kind, k, plant(make(rnd), k, inc, rnd), inc))
    return cases


BAND_INSIDE = (-4000, -256, -16, 16, 256, 4000)   # |j| * 2^-53 / q < 1e-12 for q >= 0.5, >= 16 ulps from q
BAND_OUTSIDE = (-20000, 20000)                    # 2e4 * 2^-53 / q > 1e-12 for q < 1: the fast exits
BAND_BELOW_ONE = (16, 256, 1000, 4000)            # U = 1 - j 2^-53, inside (1 - 1e-12, 1)


def bernoulli_cases(seed=77, n_q=300):
    """(p, state, inc, U_int, m): first uniform planted at U_int 2^-53 around q = m 2^-53 in [0.5, 1), for the
    direct call (p = 1 - q, exact) and for the mirrored one (p' = q, which numpy serves as 1 - binomial(1 - p'))."""
    rnd = random.Random(seed)
    cases = []
    for n in range(n_q):
        # (q = 0.5 itself once; below 1 - 4e4 ulps, so that every U around q is a valid uniform below the upper band)
        m = rnd.randrange(1 << 52, (1 << 53) - 40000) if n else (1 << 52)
        us = [m + j for j in BAND_INSIDE + BAND_OUTSIDE] + [(1 << 53) - j for j in BAND_BELOW_ONE]
        for u in us:
            for mirrored in (False, True):
                inc = random_inc(rnd)
                q = m * 2.0 ** -53
                p = q if mirrored else 1.0 - q
                cases.append((p, plant(uniform_raw(u, rnd), 0, inc, rnd), inc, u, m))
    return cases
