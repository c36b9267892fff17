"""wfm_check_optimal: every score held against a banded gap-affine DP on the device (wfmash_amd/csrc/wfa_optcheck.hip).

The reference is the CPU oracle's full-matrix DP (oracle.dp_score / dp_score_endsfree), which shares nothing with the kernel; its cost is
O(plen x tlen), so every test keeps the sum of plen x tlen under 10^8.  Problems come from tests/fuzz_align.py (gen_pair, draw_free) and
are made once per module.  No test passes by skipping: except in the cap test, no result may carry SKIPPED, and NOT_CHECKED only where the
test made the problem unalignable on purpose."""
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fuzz_align as F
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

BI, EF, UNI = capi.WFM_MODE_END2END_BIWFA, capi.WFM_MODE_ENDSFREE, capi.WFM_MODE_END2END_UNI
SO, LIMIT = capi.WFM_MODE_SCORE_ONLY, capi.WFM_MODE_SCORE_LIMIT
NOT_CHECKED, SKIPPED, CHEAPER, UNREACHED = capi.WFM_OPT_NOT_CHECKED, capi.WFM_OPT_SKIPPED, capi.WFM_OPT_CHEAPER, capi.WFM_OPT_UNREACHED
DEFAULT = (5, 8, 2, 24, 1)
# the default; a second affine pair; edit distance; o2 + e2 = 201, beyond the aligners' scope of 126
PENS = (DEFAULT, (4, 6, 2, 12, 1), (1, 0, 1, 0, 1), (6, 10, 3, 200, 1))
DP_BUDGET = 9 * 10 ** 7   # sum of plen x tlen one test gives the oracle


def _oracle_scores(oracle, items, pen):
    """the oracle's DP score of every item (p, t, mode, pbf, pef, tbf, tef), on a thread pool (ctypes releases the GIL)"""
    assert sum(len(it[0]) * len(it[1]) for it in items) <= DP_BUDGET
    def one(it):
        if it[2] & 0xff == EF:
            return oracle.dp_score_endsfree(it[0], it[1], it[3], it[4], it[5], it[6], pen)
        return oracle.dp_score(it[0], it[1], pen)
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(one, items))


def _fuzz_items(seed, n, budget):
    """n problems of gen_pair (max_len 1500), four in ten ends-free under draw_free lengths, one in ten END2END_UNI; a pair that would take the
    test's DP cells past `budget` is passed over"""
    rng = random.Random(seed)
    items, cells = [], 0
    k = 0
    while len(items) < n:
        p, t = F.gen_pair(rng, k, 1500)
        k += 1
        u = rng.random()
        if cells + len(p) * len(t) > budget:
            continue
        cells += len(p) * len(t)
        if u < 0.4:
            items.append((p, t, EF) + F.draw_free(rng, len(p), len(t)))
        else:
            items.append((p, t, UNI if u < 0.5 else BI, 0, 0, 0, 0))
    return items


def _check(gpu, items, claims, pen=None, max_cells=0):
    ss = gpu.upload(items)
    try:
        return gpu.check_optimal(ss, claims, pen, max_cells)
    finally:
        ss.free()


def _free_of(it):
    return tuple(it[3:7]) if it[2] & 0xff == EF else (0, 0, 0, 0)


def _hold_bands(items, claims, got, pen):
    """band_lo / band_hi / cells are the host rule's for the claim"""
    for it, s, g in zip(items, claims, got):
        assert (g.band_lo, g.band_hi, g.cells) == capi.host_opt_band(pen, len(it[0]), len(it[1]), _free_of(it), s)


@pytest.fixture(scope="module")
def fuzz(oracle):
    """per penalty set: about a hundred problems and the oracle's DP scores; made once, never changed"""
    out = {}
    for q, pen in enumerate(PENS):
        items = _fuzz_items(0x0C0C + q, 100, DP_BUDGET)
        out[pen] = (items, _oracle_scores(oracle, items, pen))
    return out


@pytest.mark.parametrize("pen", PENS, ids=lambda p: "pen_%d_%d_%d_%d_%d" % p)
def test_against_the_oracles_dp(gpu, fuzz, pen):
    items, scores = fuzz[pen]
    assert sum(1 for it in items if it[2] == EF) >= 25 and sum(1 for it in items if not it[0] or not it[1]) >= 3
    got = _check(gpu, items, scores, pen)
    bad = [(i, g.flags, g.dp_score, s) for i, (g, s) in enumerate(zip(got, scores)) if g.flags != 0 or g.dp_score != s]
    assert not bad, bad[:10]
    _hold_bands(items, scores, got, pen)
    assert all(g.cells > 0 for g in got)


def test_over_the_aligners(gpu, oracle):
    """a mixed batch through align_resident_rle: BiWFA, UNI, both patch forms, score-only of each, a score limit kept and one exceeded"""
    rng = random.Random(0xA11)
    items = []
    for k, (n, rate) in enumerate([(300, 0.05), (1500, 0.02), (5000, 0.03), (9000, 0.01), (2500, 0.2), (700, 0.0)]):
        p = synth.random_dna(0xA1100 + k, n)
        t = synth.mutate(p, rate, 0xA1200 + k)
        items.append((p, t, BI, 0, 0, 0, 0))
        items.append((p[:1200], t[:1150], UNI, 0, 0, 0, 0))
        items.append((p[:400], t[:380], EF, min(len(p), 400), 0, min(len(t), 380), 0))           # head patch form
        items.append((p[-400:], t[-390:], EF, 0, min(len(p), 400), 0, min(len(t), 390)))        # tail patch form
        items.append((p, t, BI | SO, 0, 0, 0, 0))
        items.append((p[:300], t[:310], EF | SO, 300, 0, min(len(t), 310), 0))
    for k in range(12):
        p, t = F.gen_pair(rng, k, 1500)
        items.append((p, t, BI, 0, 0, 0, 0))
    p = synth.random_dna(0xA1300, 3000)
    t = synth.mutate(p, 0.05, 0xA1301)
    exact = oracle.align_biwfa(p, t)[2]
    items.append((p, t, BI | LIMIT, 0, 0, 0, 0, exact))        # the limit is the score: kept
    over = len(items)
    items.append((p, t, BI | LIMIT, 0, 0, 0, 0, exact - 1))    # one below: WFM_ST_MAX_SCORE
    ss = gpu.upload(items)
    try:
        failed, _ = gpu.align_resident_rle(ss)
        assert failed == 1 and ss.results[over].status == capi.WFM_ST_MAX_SCORE
        got = gpu.check_optimal(ss, ss.results)
    finally:
        ss.free()
    for i, g in enumerate(got):
        if i == over:
            assert ss.results[i].status != 0 and g.flags == NOT_CHECKED and g.cells == 0
        else:
            assert ss.results[i].status == 0
            assert g.flags == 0 and g.dp_score == ss.results[i].score, (i, g.flags, g.dp_score, ss.results[i].score)
            assert g.cells > 0


def test_negatives(gpu, oracle, fuzz):
    items, scores = fuzz[DEFAULT]
    pick = [i for i, s in enumerate(scores) if s > 0][:40]
    assert len(pick) == 40 and any(items[i][2] == EF for i in pick)
    sub = [items[i] for i in pick]
    opt = [scores[i] for i in pick]
    for delta in (1, 5000):
        got = _check(gpu, sub, [s + delta for s in opt])
        assert [(g.flags, g.dp_score) for g in got] == [(CHEAPER, s) for s in opt], delta
    got = _check(gpu, sub, [s - 1 for s in opt])
    assert all(g.flags == UNREACHED and (g.dp_score == -1 or g.dp_score >= s) for g, s in zip(got, opt))
    # identical sequences: the optimum is 0, a claim of -1 is no score at all
    same = synth.random_dna(0xE0, 500)
    got = _check(gpu, [(same, same, BI, 0, 0, 0, 0), sub[0]], [-1, opt[0]])
    assert (got[0].flags, got[0].cells) == (NOT_CHECKED, 0) and got[1].flags == 0


def test_a_valid_suboptimal_alignment_passes_check_runs_and_fails_here(gpu):
    """one substitution spelled as an insertion and a deletion: the runs fit their bases and are priced right (2 x (8 + 2) = 20), the optimum is 5"""
    left, right = synth.random_dna(0x5B0, 300), synth.random_dna(0x5B1, 250)
    p, t = left + b"A" + right, left + b"C" + right
    runs = [(300, 0), (1, 2), (1, 3), (250, 0)]  # M I D M
    words = np.array([(n << 2) | op for n, op in runs], dtype=np.uint32)
    ss = gpu.upload([(p, t, UNI, 0, 0, 0, 0)])
    try:
        flagged, ck = gpu.check_runs(ss, [(0, 20, 0, 552, 4)], words)
        assert flagged == 0 and ck[0].flags == 0 and ck[0].score == 20
        got = gpu.check_optimal(ss, [(0, 20)])
    finally:
        ss.free()
    assert (got[0].flags, got[0].dp_score) == (CHEAPER, 5)


def _wide(seed, plen, kf):
    """a pattern of plen bases and a text that is the pattern with kf bases inserted in its middle and two substitutions: very unequal
    lengths, so every diagonal in [0, kf] is in the band at any claim, and the optimum is about one long insertion"""
    p = synth.random_dna(seed, plen)
    t = bytearray(p[:plen // 2] + synth.random_dna(seed + 2, kf) + p[plen // 2:])
    for at in (plen // 4, len(t) - plen // 4):
        t[at] = {65: 67, 67: 71, 71: 84, 84: 65}[t[at]]
    return p, bytes(t)


def _width(it, claim):
    lo, hi, _ = capi.host_opt_band(DEFAULT, len(it[0]), len(it[1]), (0, 0, 0, 0), claim)
    return hi - lo + 1


def test_widths_around_every_form_change(gpu, oracle):
    """bands one below, at and one above WFM_OPT_BAND_C1, WFM_OPT_BAND_C4 and WFM_OPT_REG_MAX, made with plen 200 and tlen = 200 + kf: once
    with kf + 1 = the width, where the exact score is the claim, and once with kf + 3 = the width and the claim raised until the band has
    grown by a diagonal on either side"""
    items, targets = [], []
    for q, Wc in enumerate((capi.OPT_BAND_C1, capi.OPT_BAND_C4, capi.OPT_REG_MAX)):
        for W in (Wc - 1, Wc, Wc + 1):
            for grow in (0, 2):
                items.append(_wide(0xD1A6 + 16 * q + grow, 200, W - 1 - grow) + (BI, 0, 0, 0, 0))
                targets.append(W)
    scores = _oracle_scores(oracle, items, DEFAULT)
    claims = []
    for it, s, W in zip(items, scores, targets):
        c = s
        while _width(it, c) < W:
            c += 1
        claims.append(c)
    assert sum(1 for c, s in zip(claims, scores) if c == s) == 9 and sum(1 for c, s in zip(claims, scores) if c > s) == 9
    got = _check(gpu, items, claims)
    for g, s, c, W in zip(got, scores, claims, targets):
        assert g.band_hi - g.band_lo + 1 == W, (W, g.band_lo, g.band_hi)
        assert (g.flags, g.dp_score) == ((CHEAPER if c > s else 0), s), (W, c, g.flags, g.dp_score, s)


def test_wide_bands_from_memory_and_ends_free(gpu, oracle):
    """bands of several tiles of WFM_OPT_REG_MAX diagonals, rows held in memory: a free beginning puts every diagonal of a 300 x 9000 matrix in
    the band, a free end likewise; and the end-to-end form of the same pair, whose band is [0, kf] and a little more"""
    p = synth.random_dna(0x3E30, 300)
    t = synth.random_dna(0x3E31, 5200) + synth.mutate(p, 0.05, 0x3E32) + synth.random_dna(0x3E33, 3500)
    items = [(p, t, EF, 300, 0, len(t), 0), (p, t, EF, 0, 300, 0, len(t)), (p, t, EF, 0, 0, len(t), len(t)), (p, t, EF, 17, 5, 6000, 40), (p, t, BI, 0, 0, 0, 0),
             (t, p, EF, len(t), len(t), 0, 0), (t, p, UNI, 0, 0, 0, 0)]
    scores = _oracle_scores(oracle, items, DEFAULT)
    got = _check(gpu, items, scores)
    for g, s in zip(got, scores):
        assert g.band_hi - g.band_lo + 1 > 2 * capi.OPT_REG_MAX
        assert (g.flags, g.dp_score) == (0, s)
    assert [g.flags for g in _check(gpu, items[:3], [s + 7 for s in scores[:3]])] == [CHEAPER] * 3


def test_unrelated_square_and_long_thin(gpu, oracle):
    a, b = synth.random_dna(0x1600, 1600), synth.random_dna(0x1601, 1600)
    long_p = synth.random_dna(0x60000, 60000)
    long_t = bytearray(long_p)
    for k, at in enumerate(range(2500, 60000, 5000)):  # a dozen edits: substitutions, and two short indels
        if k % 5 == 1:
            del long_t[at:at + 3]
        elif k % 5 == 3:
            long_t[at:at] = b"GATTACA"
        else:
            long_t[at] = {65: 67, 67: 71, 71: 84, 84: 65}[long_t[at]]
    long_t = bytes(long_t)
    rc, _, thin, _ = oracle.align_biwfa(long_p, long_t)
    assert rc == 0 and thin > 0
    square = oracle.dp_score(a, b)
    got = _check(gpu, [(a, b, BI, 0, 0, 0, 0), (long_p, long_t, BI, 0, 0, 0, 0)], [square, thin])
    assert (got[0].flags, got[0].dp_score) == (0, square)
    assert got[0].band_hi - got[0].band_lo + 1 > 3000 and got[0].cells > 2500000
    assert (got[1].flags, got[1].dp_score) == (0, thin)
    assert got[1].band_hi - got[1].band_lo + 1 < capi.OPT_BAND_C1
    got = _check(gpu, [(long_p, long_t, BI, 0, 0, 0, 0)], [thin - 1])
    assert got[0].flags == UNREACHED


def test_cell_cap(gpu, fuzz):
    items, scores = fuzz[DEFAULT]
    sub, opt = items[:30], scores[:30]
    free = _check(gpu, sub, opt)
    cells = [g.cells for g in free]
    k = max(range(30), key=lambda i: cells[i])   # the one problem the cap is set around
    assert cells[k] > 1 and sum(1 for c in cells if c == cells[k]) == 1
    below = _check(gpu, sub, opt, max_cells=cells[k] - 1)
    at = _check(gpu, sub, opt, max_cells=cells[k])
    for i in range(30):
        if i == k:
            assert (below[i].flags, below[i].cells, below[i].dp_score) == (SKIPPED, 0, -1)
        else:
            assert (below[i].flags, below[i].cells, below[i].dp_score) == (0, cells[i], opt[i])
        assert (at[i].flags, at[i].cells, at[i].dp_score) == (0, cells[i], opt[i])


def test_bytes_compare_as_bytes(gpu):
    """N against N costs nothing; a soft-masked base differs from its upper-case form and costs a mismatch"""
    s = synth.random_dna(0xB17E, 400)
    with_n = s[:100] + b"NNNNNNNN" + s[108:]
    lower = s[:200] + s[200:201].lower() + s[201:]
    got = _check(gpu, [(with_n, with_n, BI, 0, 0, 0, 0), (s, lower, BI, 0, 0, 0, 0), (s, lower, BI, 0, 0, 0, 0), (with_n, s, UNI, 0, 0, 0, 0)], [0, 5, 0, 40])
    assert sum(1 for a, b in zip(with_n, s) if a != b) == 8
    assert (got[0].flags, got[0].dp_score) == (0, 0)
    assert (got[1].flags, got[1].dp_score) == (0, 5)
    assert got[2].flags == UNREACHED
    assert (got[3].flags, got[3].dp_score) == (0, 40)   # (N differs from every base: eight mismatches, cheaper than any pair of gaps)
