"""Host model of `wave_normals` (aehmc_amd/csrc/rng.cuh) that labels the branches a request takes.

A restatement of the device function over an array of raw PCG64 outputs: 64 lanes look at 64 consecutive
stream positions, clean rounds, the clean partial last round, the parallel wedge evaluation with its `dropped` /
`wlive` masks, the generic path over the following lanes, the restart on the generator and the two ways a
request ends.  It is NOT the reference for values -- numpy is -- it exists so that a host test can prove that a
case table reaches every branch, and so that a device test knows which outputs came from the tail formula (`log1p`,
where the device may differ from libm by an ulp)."""
import math
from collections import Counter

import numpy as np

from rng_plant import FI, KI, NOR_INV_R, NOR_R, WI

LABELS = ("clean", "clean_last", "wedge_acc", "wedge_rej", "wedge_lane62", "wedge_uniform_lane_itself_failing",
          "redraw_lane_fails_again", "tail_resolved_in_wave", "tail_resolved_multi_try", "restart_tail_dry",
          "restart_lane63_tail", "restart_lane63_wedge", "general_full", "general_full_exact_end", "end_general_plain",
          "end_on_accepted_wedge", "end_on_tail")

_KI = np.array(KI, dtype=np.uint64)
_TWO53 = 1.0 / 9007199254740992.0


class Stream:
    """Raw outputs of a generator with zig_fast evaluated for all of them at once."""

    def __init__(self, raws):
        raws = np.asarray(raws, dtype=np.uint64)
        idx = (raws & np.uint64(0xff)).astype(np.int64)
        sign = ((raws >> np.uint64(8)) & np.uint64(1)).astype(bool)
        rabs = (raws >> np.uint64(9)) & np.uint64(0x000fffffffffffff)
        x = rabs.astype(np.float64) * WI[idx]
        self.raw = [int(r) for r in raws]
        self.idx = idx.tolist()
        self.rabs = [int(r) for r in rabs]
        self.x = np.where(sign, -x, x).tolist()
        self.accept = (rabs < _KI[idx]).tolist()
        self.unit = ((raws >> np.uint64(11)).astype(np.float64) * _TWO53).tolist()

    def __len__(self):
        return len(self.raw)


def _wedge_accepts(s, at, uniform_at):
    i = s.idx[at]
    return ((FI[i - 1] - FI[i]) * s.unit[uniform_at] + FI[i]) < math.exp(-0.5 * s.x[at] * s.x[at])


def _slow(s, at, nxt, end):
    """zig_slow_from for the failed draw at stream position `at`, reading positions nxt, nxt+1, ... < end.
    -> (value or None when the source ran dry, next unread position, tail value?, tail tries)."""
    tries = 0
    while True:
        if s.idx[at] == 0:
            while True:
                if nxt >= end:
                    return None, nxt, True, tries
                xx = -NOR_INV_R * math.log1p(-s.unit[nxt])
                nxt += 1
                if nxt >= end:
                    return None, nxt, True, tries
                yy = -math.log1p(-s.unit[nxt])
                nxt += 1
                tries += 1
                if yy + yy > xx * xx:
                    return (-(NOR_R + xx) if (s.rabs[at] >> 8) & 1 else NOR_R + xx), nxt, True, tries
        else:
            if nxt >= end:
                return None, nxt, False, tries
            ok = _wedge_accepts(s, at, nxt)
            nxt += 1
            if ok:
                return s.x[at], nxt, False, tries
        if nxt >= end:
            return None, nxt, False, tries
        at = nxt
        nxt += 1
        if s.accept[at]:
            return s.x[at], nxt, False, tries


def wave_normals(s, n, base=0):
    """n normals from stream `s` standing at position `base` (its next raw output is s.raw[base]).
    -> (values, position afterwards, Counter of branch labels, set of output indices from the tail formula)."""
    out = [None] * n
    labels = Counter()
    tails = set()
    pos = 0
    while pos < n:
        assert base + 64 <= len(s), "stream too short for this request"
        fail = [l for l in range(64) if not s.accept[base + l]]
        want = n - pos
        if not fail and want >= 64:
            out[pos:pos + 64] = s.x[base:base + 64]
            pos += 64
            base += 64
            labels["clean"] += 1
            continue
        if want < 64 and not any(l < want for l in fail):
            out[pos:pos + want] = s.x[base:base + want]
            labels["clean_last"] += 1
            return out, base + want, labels, tails
        failset = set(fail)
        wacc = {f for f in fail if f < 63 and s.idx[base + f] != 0 and _wedge_accepts(s, base + f, base + f + 1)}
        tailm = {f for f in fail if s.idx[base + f] == 0}
        x = s.x[base:base + 64]
        dropped, wlive, tail_lanes = set(), set(), set()
        cur, serial, ev_f, ev_end = 0, None, -1, -1
        while True:
            m = [f for f in fail if f >= cur]
            if not m:
                break
            f = m[0]
            before = f - sum(1 for l in dropped if l < f)
            if before >= want:
                break
            if f < 63 and f not in tailm:
                if f in wacc:
                    dropped.add(f + 1)
                    wlive.add(f)
                    labels["wedge_acc"] += 1
                else:
                    dropped.update((f, f + 1))
                    labels["wedge_rej"] += 1
                    if f + 2 in failset:
                        labels["redraw_lane_fails_again"] += 1
                if f == 62:
                    labels["wedge_lane62"] += 1
                if f + 1 in failset:
                    labels["wedge_uniform_lane_itself_failing"] += 1
                cur = f + 2
                continue
            ev_f = f
            z, nxt, is_tail, tries = _slow(s, base + f, base + f + 1, base + 64)
            if z is not None:
                dropped.update(range(f + 1, nxt - base))
                ev_end = nxt - base - 1
                cur = nxt - base
                labels["tail_resolved_in_wave"] += 1
                if tries > 1:
                    labels["tail_resolved_multi_try"] += 1
            else:
                z, nxt, is_tail, tries = _slow(s, base + f, base + f + 1, len(s))
                assert z is not None, "stream too short for this restart"
                serial = nxt
                dropped.update(range(f + 1, 64))
                cur = 64
                if f == 63:
                    labels["restart_lane63_tail" if f in tailm else "restart_lane63_wedge"] += 1
                else:
                    labels["restart_tail_dry"] += 1
            if is_tail:
                tail_lanes.add(f)
            x[f] = z
        mine = [l for l in range(64) if l not in dropped]
        produced = len(mine)
        if produced <= want:
            for o, l in enumerate(mine):
                out[pos + o] = x[l]
                if l in tail_lanes:
                    tails.add(pos + o)
            pos += produced
            base = serial if serial is not None else base + 64
            labels["general_full"] += 1
            if produced == want:
                labels["general_full_exact_end"] += 1
        else:
            for o, l in enumerate(mine[:want]):
                out[pos + o] = x[l]
                if l in tail_lanes:
                    tails.add(pos + o)
            L = mine[want - 1]
            if L in wlive:
                labels["end_on_accepted_wedge"] += 1
                return out, base + L + 2, labels, tails
            if L == ev_f:
                labels["end_on_tail"] += 1
                return out, base + ev_end + 1, labels, tails
            labels["end_general_plain"] += 1
            return out, base + L + 1, labels, tails
    return out, base, labels, tails
