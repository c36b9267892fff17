"""The GPU-free side of wfm_check_optimal / --verify-optimal: the layout of wfm_optcheck_t, the exported symbols, the process-wide counters,
and the band rule (wfmash_amd/csrc/wfa_optband.h through wfmh_test_opt_band) held against a full-matrix DP written here.

The lemma under test: every alignment of price <= S lies on the diagonals the rule returns for S.  So for a claim S at or above the
optimum a DP restricted to the band finds the optimum itself, and for S one below the optimum it finds nothing of price <= S.  The DP
below is the textbook five-matrix recurrence of oracle/wfa2p.c's dp_generic, written again in Python (no code shared with the device or
the oracle); cells outside the band are simply unreachable."""
import ctypes as C
import random

import pytest

from wfmash_amd import capi

INF = 1 << 40
# default; a second affine pair; o2 + e2 beyond the aligners' scope of 126; edit distance; a large mismatch; piece 2 never cheaper
PENS = ((5, 8, 2, 24, 1), (4, 6, 2, 12, 1), (6, 10, 3, 200, 1), (1, 0, 1, 0, 1), (33, 20, 2, 24, 1), (3, 2, 2, 9, 3))


def dp(p, t, pen, free, band=None):
    """optimal price, INF if nothing ends inside; free = (pbf, pef, tbf, tef) or None for end-to-end; band = (lo, hi) of j - i"""
    x, o1, e1, o2, e2 = pen
    plen, tlen = len(p), len(t)
    pbf, pef, tbf, tef = free if free is not None else (0, 0, 0, 0)
    best = INF
    pm = pd1 = pd2 = None
    for v in range(plen + 1):
        m, i1, i2, d1, d2 = ([INF] * (tlen + 1) for _ in range(5))
        for h in range(tlen + 1):
            if band is not None and not band[0] <= h - v <= band[1]:
                continue
            vm = INF
            if h > 0:
                i1[h] = min(m[h - 1] + o1 + e1, i1[h - 1] + e1)
                i2[h] = min(m[h - 1] + o2 + e2, i2[h - 1] + e2)
            if v > 0:
                d1[h] = min(pm[h] + o1 + e1, pd1[h] + e1)
                d2[h] = min(pm[h] + o2 + e2, pd2[h] + e2)
                if h > 0:
                    vm = pm[h - 1] + (0 if p[v - 1] == t[h - 1] else x)
            if (v == 0 and h <= tbf) or (h == 0 and v <= pbf):
                vm = 0
            m[h] = min(vm, i1[h], i2[h], d1[h], d2[h], INF)
            if (h == tlen and plen - v <= pef) or (v == plen and tlen - h <= tef):
                best = min(best, m[h])
        pm, pd1, pd2 = m, d1, d2
    return best


def draw_problem(rng):
    plen = rng.choice([0, 1, 2, 3, 5, 9, 17, 25, 33, 40, rng.randrange(0, 41)])
    p = bytes(rng.choice(b"ACGT") for _ in range(plen))
    kind = rng.randrange(4)
    if kind == 0:  # unrelated
        t = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 41)))
    else:  # mutated, with junk at either end so that free ends matter
        t = bytearray()
        for c in p:
            r = rng.random()
            if r < 0.1:
                t.append(rng.choice(b"ACGT"))
            elif r < 0.16:
                continue
            elif r < 0.22:
                t += bytes([c, rng.choice(b"ACGT")])
            else:
                t.append(c)
        if kind == 2:
            t = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 12))) + bytes(t) + bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 12)))
        if kind == 3 and len(t) > 8:
            a = rng.randrange(0, len(t) - 4)
            t = t[:a] + t[a + rng.randrange(1, 12):]
        t = bytes(t)[:40]
    def one(n):
        return rng.choice([0, n, rng.randrange(0, min(n, 8) + 1), rng.randrange(0, n + 1)])
    free = None if rng.random() < 0.3 else (one(plen), one(plen), one(len(t)), one(len(t)))
    return p, t, free


def test_layout_constants_and_symbols():
    assert C.sizeof(capi.OptCheck) == 24
    assert [f[0] for f in capi.OptCheck._fields_] == ["flags", "dp_score", "band_lo", "band_hi", "cells"]
    assert (capi.WFM_OPT_NOT_CHECKED, capi.WFM_OPT_SKIPPED, capi.WFM_OPT_CHEAPER, capi.WFM_OPT_UNREACHED) == (1, 2, 4, 8)
    assert (capi.OPT_BAND_C1, capi.OPT_BAND_C4, capi.OPT_REG_MAX) == (256, 1024, 4096)
    L = capi.load()
    assert "wfm_check_optimal" in capi.EXPORTS
    for name in ("wfm_check_optimal", "wfmh_set_verify_optimal", "wfmh_verify_optimal_counts", "wfmh_test_opt_band"):
        getattr(L, name)
    for name in ("wfmh_set_verify_optimal", "wfmh_verify_optimal_counts", "wfmh_test_opt_band"):
        assert name in capi.HOST_EXPORTS


def test_header_constants_match():
    """the numbers capi.py repeats are the header's"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wfmash_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define (WFM_OPT_[A-Z0-9_]+)\s+(\d+)u?\b", text)}
    assert got == {"WFM_OPT_NOT_CHECKED": 1, "WFM_OPT_SKIPPED": 2, "WFM_OPT_CHEAPER": 4, "WFM_OPT_UNREACHED": 8, "WFM_OPT_BAND_C1": capi.OPT_BAND_C1,
                   "WFM_OPT_BAND_C4": capi.OPT_BAND_C4, "WFM_OPT_REG_MAX": capi.OPT_REG_MAX, "WFM_OPT_ROWS_MB": capi.OPT_ROWS_MB}


def test_counts_without_a_run():
    capi.set_verify_optimal(True, 1000)
    assert capi.verify_optimal_counts() == (0, 0, 0, 0)
    capi.set_verify_optimal(False)
    assert capi.verify_optimal_counts() == (0, 0, 0, 0)


def test_band_by_hand():
    """end-to-end, default penalties (g(L) = min(8 + 2 L, 24 + L)): 10 x 14, kf = 4.  S = 0: only [0, 4].  Above: g(k - 0) + g(k - 4) <= S;
    S = 30: k = 5 costs 18 + 10 = 28, k = 6 costs 20 + 12 = 32 -> 5.  Below: g(-k) + g(4 - k); k = -1: 10 + 18 = 28, k = -2: 12 + 20 -> -1"""
    assert capi.host_opt_band(None, 10, 14, (0, 0, 0, 0), 0)[:2] == (0, 4)
    assert capi.host_opt_band(None, 10, 14, (0, 0, 0, 0), 30)[:2] == (-1, 5)
    # a huge claim: the whole matrix, and every one of its cells
    assert capi.host_opt_band(None, 10, 14, (0, 0, 0, 0), 1 << 28) == (-10, 14, 11 * 15)
    # the head patch form (everything free at the beginning): start diagonals [-10, 14] are all there at S = 0
    assert capi.host_opt_band(None, 10, 14, (10, 0, 14, 0), 0) == (-10, 14, 11 * 15)
    # free lengths are clamped to their sequence
    assert capi.host_opt_band(None, 10, 14, (99, 0, 99, 0), 0) == (-10, 14, 11 * 15)
    # empty sides
    assert capi.host_opt_band(None, 0, 0, (0, 0, 0, 0), 0) == (0, 0, 1)
    assert capi.host_opt_band(None, 0, 7, (0, 0, 0, 0), 31) == (0, 7, 8)


def test_cells_counted_against_brute_force():
    rng = random.Random(0x0C11)
    for _ in range(400):
        plen, tlen = rng.randrange(0, 30), rng.randrange(0, 30)
        free = tuple(rng.randrange(0, 35) for _ in range(4))
        S = rng.choice([0, 3, 17, 40, 90, 400])
        lo, hi, cells = capi.host_opt_band(rng.choice(PENS), plen, tlen, free, S)
        assert -plen <= lo <= hi <= tlen
        assert cells == sum(1 for i in range(plen + 1) for j in range(tlen + 1) if lo <= j - i <= hi), (plen, tlen, free, S, lo, hi)


@pytest.mark.parametrize("pen", PENS, ids=lambda p: "pen_%d_%d_%d_%d_%d" % p)
def test_band_holds_every_alignment_of_the_claimed_price(pen):
    rng = random.Random(0xBA2D + sum(pen))
    n_below = n_free = 0
    for _ in range(70):
        p, t, free = draw_problem(rng)
        f = free if free is not None else (0, 0, 0, 0)
        opt = dp(p, t, pen, free)
        assert opt < INF
        n_free += free is not None
        for S in (opt, opt + 1, opt + rng.randrange(2, 60), opt + rng.randrange(60, 600)):
            lo, hi, _ = capi.host_opt_band(pen, len(p), len(t), f, S)
            assert dp(p, t, pen, free, (lo, hi)) == opt, (p, t, free, S, lo, hi)
        if opt > 0:
            lo, hi, _ = capi.host_opt_band(pen, len(p), len(t), f, opt - 1)
            assert dp(p, t, pen, free, (lo, hi)) > opt - 1, (p, t, free, lo, hi)
            n_below += 1
    assert n_below >= 30 and n_free >= 30


def test_band_is_not_the_crude_one():
    """between its start and end diagonals a path crosses k with a single run: a rule that charged g(|k - ks|) + g(|k - ke|) there would cut
    the only alignment.  8 x 20 end-to-end with the optimum one insertion of 12: price 8 + 2 x 12 = 32, and at S = 32 all of [0, 12] is kept"""
    p = b"ACGTACGT"
    t = p[:4] + b"TTTTTTTTTTTT" + p[4:]
    opt = dp(p, t, (5, 8, 2, 24, 1), None)
    assert opt == 32
    lo, hi, _ = capi.host_opt_band(None, len(p), len(t), (0, 0, 0, 0), opt)
    assert (lo, hi) == (0, 12)
    assert dp(p, t, (5, 8, 2, 24, 1), None, (lo, hi)) == opt
