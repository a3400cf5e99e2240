"""Planted generator states (tests/rng_plant.py) on the host: the planting itself, the branch-labelling model of
`wave_normals` against numpy over the whole case table, the coverage of that table as a condition, and the C oracle --
the reference of the kernel-family tests in tests/test_gpu_rng_planted.py -- on the same rare paths."""
import random
from collections import Counter

import numpy as np
import pytest

import rng_plant as rp
import wave_normals_ref as wr
from oracle import c_oracle as co

MIN_HITS = 20  # every branch label, over the case table (seeded: the counts are fixed data)


def test_planted_word_comes_out_at_its_position():
    rnd = random.Random(1)
    for k in (0, 1, 2, 62, 63, 64, 127, 1000):
        for make in (rp.tail_raw, rp.wedge_raw, lambda r: r.getrandbits(64)):
            raw, inc = make(rnd), rp.random_inc(rnd)
            s = rp.plant(raw, k, inc, rnd)
            got = rp.numpy_generator(s, inc).bit_generator.random_raw(k + 1)
            assert int(got[k]) == raw
            # the helper's own step / output against numpy's, along the way
            t = s
            for i in range(min(k + 1, 5)):
                t = rp.step(t, inc)
                assert rp.output(t) == int(got[i])
            assert rp.back_step(rp.step(s, inc), inc) == s


def test_raw_builders_take_the_branch_they_name():
    rnd = random.Random(2)
    for _ in range(200):
        s = wr.Stream([rp.tail_raw(rnd), rp.wedge_raw(rnd)])
        assert s.idx[0] == 0 and not s.accept[0]
        assert 1 <= s.idx[1] <= 255 and not s.accept[1]
        u = rnd.randrange(1 << 53)
        inc = rp.random_inc(rnd)
        g = rp.numpy_generator(rp.plant(rp.uniform_raw(u, rnd), 0, inc, rnd), inc)
        assert g.random() == u * 2.0 ** -53


@pytest.fixture(scope="module")
def table():
    """Every (stream, request size) of the case table through the model and through numpy."""
    rows = []
    for kind, k, state, inc in rp.normal_cases():
        raws = rp.numpy_generator(state, inc).bit_generator.random_raw(1024)
        s = wr.Stream(raws)
        for n in rp.NORMAL_SIZES:
            rows.append((kind, k, state, inc, n, raws, wr.wave_normals(s, n), s))
    return rows


def test_model_equals_numpy_on_the_case_table(table):
    assert len(table) == 2 * len(rp.NORMAL_POSITIONS) * rp.NORMAL_REPLICATES * len(rp.NORMAL_SIZES)
    for kind, k, state, inc, n, raws, (z, pos, labels, tails), s in table:
        g = rp.numpy_generator(state, inc)
        ref = g.normal(size=n)
        assert np.array_equal(np.array(z), ref), (kind, k, n)
        assert int(g.bit_generator.random_raw()) == int(raws[pos]), (kind, k, n)  # the stream stands where numpy's does
        # ... and the call that follows on the same state (the device test makes it too)
        z2, pos2, _, _ = wr.wave_normals(s, 64, pos)
        g = rp.numpy_generator(state, inc)
        g.normal(size=n)
        assert np.array_equal(np.array(z2), g.normal(size=64)), (kind, k, n)
        assert int(g.bit_generator.random_raw()) == int(raws[pos2]), (kind, k, n)


EXPECTED_COUNTS = {"clean": 569, "clean_last": 10294, "wedge_acc": 8798, "wedge_rej": 8186, "wedge_lane62": 62,
                   "wedge_uniform_lane_itself_failing": 267, "redraw_lane_fails_again": 269, "tail_resolved_in_wave": 5868,
                   "tail_resolved_multi_try": 760, "restart_tail_dry": 42, "restart_lane63_tail": 37,
                   "restart_lane63_wedge": 138, "general_full": 5010, "general_full_exact_end": 272,
                   "end_general_plain": 9420, "end_on_accepted_wedge": 193, "end_on_tail": 129}


def test_case_table_reaches_every_branch(table):
    total = Counter()
    for row in table:
        total.update(row[6][2])
    assert set(total) <= set(wr.LABELS)
    short = {lab: total[lab] for lab in wr.LABELS if total[lab] < MIN_HITS}
    assert not short, f"branches reached fewer than {MIN_HITS} times: {short}; all: {dict(total)}"
    # the counts of this (seeded) table
    assert dict(total) == EXPECTED_COUNTS


def test_c_oracle_normals_on_planted_states(table):
    for kind, k, state, inc, n, raws, _, _ in table:
        st = np.array(rp.pack(state, inc), dtype=np.uint64)
        g = rp.numpy_generator(state, inc)
        assert np.array_equal(co.rng_normals(st, n), g.normal(size=n)), (kind, k, n)
        assert rp.unpack_state(st) == rp.generator_state(g)
        assert co.rng_doubles(st, 4).tolist() == g.random(4).tolist()


def test_c_oracle_and_exact_arithmetic_on_planted_bernoulli():
    cases = rp.bernoulli_cases()
    assert len(cases) == 300 * 12 * 2
    for p, state, inc, u, m in cases:
        st = np.array(rp.pack(state, inc), dtype=np.uint64)
        g = rp.numpy_generator(state, inc)
        ref = int(g.binomial(1, p))
        assert int(co.rng_bernoulli(st, np.array([p]))[0]) == ref, (p, u, m)
        # numpy's outcome is the exact-arithmetic one (0 iff U <= q; mirrored: 1 iff U <= q) after ONE uniform: at 16 ulps
        # from q an exp(log(q)) that is an ulp or two off, on any libm, cannot change it
        exact = (0 if u <= m else 1) if p <= 0.5 else (1 if u <= m else 0)
        assert ref == exact, (p, u, m)
        assert rp.generator_state(g) == rp.step(state, inc), (p, u, m)
        assert rp.unpack_state(st) == rp.generator_state(g)
        assert co.rng_doubles(st, 2).tolist() == g.random(2).tolist()
