"""WFM_MODE_ENDSFREE over general free lengths, through every form of the base kernels and every entry point, against the CPU oracle.

The callers of the product send two tuples -- (plen, 0, tlen, 0) and (0, plen, 0, tlen) -- and every other test of the suite does the same;
the ABI takes four independent lengths and the device implements them (row 0 spans [-pbf, tbf]: base_rows of wfa_base.h; the end tests of
wfa_generic_inc.h and wfa_tile2.hip read pef / tef; base_columns of wfa_plan.h bands a job around the end corner only when pef == tef == 0;
the upload clamps every length to its sequence).  tests/endsfree_cases.py is the family: partial lengths, one free end alone, begin and end
free at once, empty sides.  Every comparison is exact: status, score, op bytes, run counts, flags.  The score is compared three ways -- the
oracle's (which tests/test_oracle_wfa.py holds against the O(nm) DP), the score-only run's, and the op string priced on its own
(endsfree_price) -- because a full ends-free result used to carry the price of its runs, free end gaps included."""
import contextlib
import itertools
import os
import types

import pytest

import endsfree_cases as E
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

EF, SO = capi.WFM_MODE_ENDSFREE, capi.WFM_MODE_SCORE_ONLY
RING, TILES, BYTE = capi.WFM_PF_RING_KERNEL, capi.WFM_PF_BASE_TILES, capi.WFM_PF_BYTE_KERNEL
BIG_PEN = (6, 10, 3, 124, 1)  # o2 + e2 = 125: the 128-row rings
FORMS = (("ring", {"WFM_BASE_V2": "0"}), ("registers", {}), ("tiles", {"WFM_BASE_TILES": "2"}))


def _expect(oracle, cases, pen=None):
    out = []
    for c in cases:
        rc, ops, sc, _ = oracle.align_endsfree(c.p, c.free[0], c.free[1], c.t, c.free[2], c.free[3], pen=pen)
        assert rc == 0, (c.name, c.free)
        out.append((ops, sc))
    return out


@pytest.fixture(scope="module")
def family(oracle):
    """The family with the oracle's (ops, score) under the default penalties and under BIG_PEN: computed once, never changed."""
    cases = E.build_cases()
    return types.SimpleNamespace(cases=cases, exp={None: _expect(oracle, cases), BIG_PEN: _expect(oracle, cases, BIG_PEN)},
                                 nontrivial=[i for i, c in enumerate(cases) if c.p and c.t])


def _items(cases, flags=0):
    return [(c.p, c.t, EF | flags) + tuple(c.free) for c in cases]


def _n_runs(ops):
    return sum(1 for _ in itertools.groupby(ops))


def _check_full(cases, res, exp, pen=None):
    assert len(res) == len(cases) == len(exp)
    for i, (c, r, (ops, sc)) in enumerate(zip(cases, res, exp)):
        where = (i, c.name, c.free)
        assert r.status == 0, where
        assert r.ops == ops, where
        assert r.n_runs == _n_runs(ops), where
        assert r.score == sc, where + (r.score, sc)
        assert E.endsfree_price(r.ops, c.free, pen) == r.score, where


def _check_scores(cases, res, exp):
    for i, (c, r, (_, sc)) in enumerate(zip(cases, res, exp)):
        where = (i, c.name, c.free)
        assert r.status == 0, where
        assert r.score == sc, where + (r.score, sc)
        assert r.ops == b"" and r.n_runs == 0, where  # (ops is the arena's ops_len bytes)


@contextlib.contextmanager
def _switches(env):
    """the base kernels' switches are read per call: set for the block, whatever the caller's environment holds put back behind it"""
    names = ("WFM_BASE_V2", "WFM_BASE_TILES")
    before = {k: os.environ.pop(k) for k in names if k in os.environ}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(before)


def _through_forms(gpu, items, pen=None):
    runs, flags = {}, {}
    for name, env in FORMS:
        with _switches(env):
            runs[name] = gpu.align(items, pen)
            flags[name] = [int(f) for f in gpu.problem_flags(len(items))]
    return runs, flags


def _same_results(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x.status, x.score, x.n_runs) == (y.status, y.score, y.n_runs), i
        assert x.ops == y.ops, i


def test_family_under_the_default_switches(gpu, family):
    with _switches({}):
        res = gpu.align(_items(family.cases))
    _check_full(family.cases, res, family.exp[None])


def test_family_score_only_and_mixed(gpu, family):
    """The same batch with WFM_MODE_SCORE_ONLY: the same scores and nothing else; and one call with full and score-only problems in turn."""
    with _switches({}):
        only = gpu.align(_items(family.cases, SO))
        mixed = gpu.align([it if i % 2 == 0 else _items([c], SO)[0] for i, (c, it) in enumerate(zip(family.cases, _items(family.cases)))])
    _check_scores(family.cases, only, family.exp[None])
    _check_full(family.cases[0::2], mixed[0::2], family.exp[None][0::2])
    _check_scores(family.cases[1::2], mixed[1::2], family.exp[None][1::2])


def test_family_through_ring_register_and_tile_forms(gpu, family):
    """WFM_BASE_V2=0 (r32::wfa_base_kernel's ring), nothing set (wfa_base2_kernel's registers), WFM_BASE_TILES=2 (wfa_base2t_kernel's tiles for
    rows beyond 128 diagonals): the three share base_rows and base_walk, and each of them ran -- by the problems' flags -- on a third at
    least of the jobs that have a cell to compute."""
    runs, flags = _through_forms(gpu, _items(family.cases))
    nt = family.nontrivial
    assert len(nt) * 10 >= len(family.cases) * 9
    on_ring = [i for i in nt if flags["ring"][i] & RING]
    on_registers = [i for i in nt if not flags["registers"][i] & (RING | TILES)]
    on_tiles = [i for i in nt if flags["tiles"][i] & TILES]
    assert len(on_ring) * 3 >= len(nt) and len(on_registers) * 3 >= len(nt) and len(on_tiles) * 3 >= len(nt), (len(nt), len(on_ring), len(on_registers), len(on_tiles))
    assert not any(f & TILES for f in flags["ring"]) and not any(f & RING for f in flags["registers"] + flags["tiles"])
    assert set(on_tiles) <= set(on_ring)
    for name in ("ring", "registers", "tiles"):
        _check_full(family.cases, runs[name], family.exp[None])
    _same_results(runs["ring"], runs["registers"])
    _same_results(runs["tiles"], runs["registers"])


def test_family_on_128_row_rings(gpu, family):
    """Penalties (6, 10, 3, 124, 1): r128::wfa_base_kernel for every job, against the oracle under those penalties; full and score-only."""
    with _switches({}):
        res = gpu.align(_items(family.cases), BIG_PEN)
        fl = [int(f) for f in gpu.problem_flags(len(family.cases))]
        only = gpu.align(_items(family.cases, SO), BIG_PEN)
    _check_full(family.cases, res, family.exp[BIG_PEN], BIG_PEN)
    _check_scores(family.cases, only, family.exp[BIG_PEN])
    assert all(fl[i] & RING for i in family.nontrivial) and not any(f & TILES for f in fl)


def test_byte_kernel_pairs(gpu, oracle):
    """An N and a soft-masked stretch send an ends-free job to the byte form of the ring kernel (WFM_PF_BYTE_KERNEL, WFM_PF_RING_KERNEL)."""
    cases = []
    for L, rate, junk in ((130, 0.05, (9, 3, 24, 1)), (400, 0.2, (0, 41, 3, 70)), (900, 0.05, (24, 0, 0, 9))):
        b, d, a, c = junk
        core = synth.random_dna(0xB17E + L, L)
        mut = bytearray(synth.mutate(core, rate, 0xB17F + L))
        mut[len(mut) // 2] = ord("N")
        p = synth.random_dna(0xB180 + L, b) + core[:L // 4] + core[L // 4:L // 4 + 40].lower() + core[L // 4 + 40:] + synth.random_dna(0xB181 + L, d)
        t = synth.random_dna(0xB182 + L, a) + bytes(mut) + synth.random_dna(0xB183 + L, c)
        for f in ((b, d, a, c), (b + 2, max(0, d - 2), max(0, a - 3), c + 1), (len(p), 0, len(t), 0), (0, len(p), 0, len(t)), (3, 4, 5, 6), (0, 0, 0, 0)):
            cases.append(E.Case("N%d" % L, p, t, E.clamp(f, len(p), len(t))))
    exp = _expect(oracle, cases)
    with _switches({}):
        res = gpu.align(_items(cases))
        fl = [int(f) for f in gpu.problem_flags(len(cases))]
        only = gpu.align(_items(cases, SO))
    _check_full(cases, res, exp)
    _check_scores(cases, only, exp)
    assert all(f & BYTE and f & RING for f in fl), fl


def _prefix_cases():
    """base_columns' corner band (a job whose alignment must end in the far corner keeps the diagonals within its score budget of
    tl - pl; first budget 256): a 600-base unrelated prefix on one side in front of a core of 300 / 400 bases.
    A: pef == tef == 0, begin-free lengths short of and beyond the prefix, row 0 = [-pbf, tbf] partly outside tl - pl +- 256;
    B: the same with row 0 inside it (a 200-base prefix; and the 600-base prefix at 20 %: its second budget's band holds row 0);
    C: the prefix as a free END (pef / tef > 0): no corner to band around, the end is reached 600 diagonals from tl - pl."""
    out = []
    core = synth.random_dna(0xC0A, 300)
    near = synth.mutate(core, 0.03, 0xC0B)
    far = synth.random_dna(0xC0C, 400)
    far_m = synth.mutate(far, 0.2, 0xC0D)
    pre600, pre200 = synth.random_dna(0xC0E, 600), synth.random_dna(0xC0F, 200)
    smax = 256

    def row0_inside(p, t, f):
        k_end = len(t) - len(p)
        return k_end - smax <= -f[0] and f[2] <= k_end + smax

    for f in ((0, 0, 620, 0), (0, 0, 590, 0), (50, 0, 600, 0), (0, 0, 899, 0), (7, 0, 605, 0)):  # A, the prefix on the text
        c = E.Case("A_text", core, pre600 + near, f)
        assert not row0_inside(c.p, c.t, f)
        out.append(c)
    for f in ((620, 0, 0, 0), (590, 0, 0, 0), (600, 0, 50, 0), (605, 0, 7, 0)):  # A, the prefix on the pattern
        c = E.Case("A_pattern", pre600 + core, near, f)
        assert not row0_inside(c.p, c.t, f)
        out.append(c)
    for f in ((0, 0, 220, 0), (0, 0, 190, 0), (30, 0, 200, 0)):  # B
        c = E.Case("B_text", core, pre200 + near, f)
        assert row0_inside(c.p, c.t, f)
        out.append(c)
    for f in ((220, 0, 0, 0), (190, 0, 40, 0)):
        c = E.Case("B_pattern", pre200 + core, near, f)
        assert row0_inside(c.p, c.t, f)
        out.append(c)
    for f in ((0, 0, 620, 0), (0, 0, 590, 0)):  # B by its second budget
        out.append(E.Case("B_second_budget", far, pre600 + far_m, f))
    for f in ((0, 620, 0, 0), (0, 590, 0, 0), (0, 600, 0, 3), (5, 900, 0, 0)):  # C
        out.append(E.Case("C_pattern", core + pre600, near, f))
    for f in ((0, 0, 0, 620), (0, 0, 0, 590), (0, 3, 0, 600)):
        out.append(E.Case("C_text", core, near + pre600, f))
    return out


def test_corner_band_edges(gpu, oracle):
    cases = _prefix_cases()
    exp = _expect(oracle, cases)
    runs, flags = _through_forms(gpu, _items(cases))
    for name, _ in FORMS:
        _check_full(cases, runs[name], exp)
    # the premises: A and the first B fit their first budget, the last B needs its second; C's end lies far from the corner's diagonal
    for c, (ops, sc), f in zip(cases, exp, flags["registers"]):
        if c.name == "B_second_budget":
            assert sc > 256 and f & capi.WFM_PF_BASE_RETRY, (c.free, sc, f)
        elif c.name[0] in "AB":
            assert sc <= 256 and not f & capi.WFM_PF_BASE_RETRY, (c.name, c.free, sc, f)
        else:
            assert ops.endswith(b"D" * 590) or ops.endswith(b"I" * 590), (c.name, c.free)
    with _switches({}):
        _check_scores(cases, gpu.align(_items(cases, SO)), exp)


def test_third_attempt_with_partial_free_lengths(gpu, oracle):
    """3 kb at 10 %: the score passes the first budget (256) and the second (1020).  On tiles the second attempt takes the eightfold budget
    at once (WFM_PF_BASE_RETRY); with WFM_BASE_TILES=0 there is a third attempt (WFM_PF_BASE_RETRY2).  Free lengths short of and beyond
    the junk on either end of the text."""
    p = synth.random_dna(0x3A77, 3000)
    t = synth.random_dna(0x3A78, 40) + synth.mutate(p, 0.10, 0x3A79) + synth.random_dna(0x3A7A, 30)
    cases = [E.Case("3kb", p, t, f) for f in ((0, 0, 50, 25), (0, 0, 35, 30), (4, 0, 40, 0))]
    exp = _expect(oracle, cases)
    assert all(sc > 1020 for _, sc in exp), [sc for _, sc in exp]
    with _switches({}):
        res = gpu.align(_items(cases))
        fl = [int(f) for f in gpu.problem_flags(len(cases))]
        only = gpu.align(_items(cases, SO))
    _check_full(cases, res, exp)
    _check_scores(cases, only, exp)
    assert all(f & capi.WFM_PF_BASE_RETRY for f in fl), fl
    with _switches({"WFM_BASE_TILES": "0"}):
        res0 = gpu.align(_items(cases))
        fl0 = [int(f) for f in gpu.problem_flags(len(cases))]
    _check_full(cases, res0, exp)
    assert all(f & capi.WFM_PF_BASE_RETRY and f & capi.WFM_PF_BASE_RETRY2 and not f & TILES for f in fl0), fl0


def test_score_zero_without_a_match(gpu, oracle):
    """Unrelated sequences: everything free; the pattern skipped before the text (pbf = plen, tef = tlen alone); and the mirror."""
    cases = []
    for i, (pl, tl) in enumerate(((300, 280), (1, 1), (70, 1500), (1500, 64))):
        p, t = synth.random_dna(0x2E60 + i, pl), synth.random_dna(0x2E70 + i, tl)
        for f in ((pl, pl, tl, tl), (pl, 0, 0, tl), (0, pl, tl, 0)):
            cases.append(E.Case("unrelated", p, t, f))
    exp = _expect(oracle, cases)
    assert all(sc == 0 for _, sc in exp)
    runs, _ = _through_forms(gpu, _items(cases))
    for name, _ in FORMS:
        _check_full(cases, runs[name], exp)
    with _switches({}):
        _check_scores(cases, gpu.align(_items(cases, SO)), exp)
        _check_full(cases, gpu.align(_items(cases), BIG_PEN), _expect(oracle, cases, BIG_PEN), BIG_PEN)


def test_free_lengths_are_clamped(gpu, oracle, family):
    """Lengths above the sequence's and below zero give exactly the clamped tuple's result (the oracle is asked with the clamped values)."""
    big, neg = 2 ** 31 - 1, -2 ** 31
    picked = [c for c in family.cases if c.name in ("core60_5%", "core400_20%", "core5_0%") and c.free == (0, 0, 0, 0)]
    picked += [c for c in family.cases if c.name in ("empty_x_10", "12_x_empty") and c.free == (0, 0, 0, 0)]
    assert len(picked) == 5
    raw, cases = [], []
    for c in picked:
        pl, tl = len(c.p), len(c.t)
        for f in ((pl + 50, -3, tl + 7, -1), (-5, pl + 1, -2, 2 * tl + 1), (big, big, big, big), (neg, neg, neg, neg), (3, big, neg, 4), (neg, 2, 5, big)):
            raw.append((c.p, c.t, EF) + f)
            cases.append(E.Case(c.name, c.p, c.t, E.clamp(f, pl, tl)))
    exp = _expect(oracle, cases)
    with _switches({}):
        got = gpu.align(raw)
        want = gpu.align(_items(cases))
        only = gpu.align([it[:2] + (EF | SO,) + it[3:] for it in raw])
    _same_results(got, want)
    _check_full(cases, got, exp)
    _check_scores(cases, only, exp)


def test_the_other_entry_points(gpu, family):
    """A dozen of the family through wfm_align_batch_rle, wfm_align_resident and wfm_align_refs_rle (the patterns as windows of one stored
    sequence, the texts and the empty patterns as host bytes)."""
    n = len(family.cases)
    picked = sorted(set(range(5, n, n // 10)) | {i for i, c in enumerate(family.cases) if c.free in ((0, 0, 4, 3), (5, 2, 0, 0))})
    assert 12 <= len(picked) <= 14
    cases = [family.cases[i] for i in picked]
    exp = [family.exp[None][i] for i in picked]
    assert sum(E.endsfree_price(ops, (0, 0, 0, 0)) != sc for ops, sc in exp) >= 6  # (free gaps in use)
    items = _items(cases)
    with _switches({}):
        rle = gpu.align_rle(items)
        ss = gpu.upload(items)
        try:
            resident = gpu.align_resident(ss)
        finally:
            ss.free()
        store = gpu.seqstore()
        try:
            blob, offs = b"", []
            for c in cases:
                blob += b"ACGT" * 3
                offs.append(len(blob))
                blob += c.p
            sid = store.add(blob + b"ACGT")
            refs = []
            for c, o in zip(cases, offs):
                free = dict(pattern_begin_free=c.free[0], pattern_end_free=c.free[1], text_begin_free=c.free[2], text_end_free=c.free[3])
                if c.p:
                    refs.append(dict(pattern_seq=sid, pattern_off=o, plen=len(c.p), text=c.t, mode=EF, **free))
                else:
                    refs.append(dict(pattern=c.p, text=c.t, mode=EF, **free))
            by_ref = gpu.align_refs(store, refs)
        finally:
            store.free()
    _check_full(cases, resident, exp)
    _check_full(cases, by_ref, exp)
    for i, (c, (r, ops_len), (ops, sc)) in enumerate(zip(cases, rle, exp)):
        assert r.status == 0 and r.score == sc, (i, c.name, c.free, r.score, sc)
        assert b"".join(op * ln for ln, op in r.ops) == ops and r.n_runs == len(r.ops) == _n_runs(ops) and ops_len == len(ops), (i, c.name, c.free)
