"""GPU tests of --genotypes: wfm_sites_* through capi.Sites on hand-built lists, every table held cell for cell against the brute force of
tests/sites_model.py; then the align driver on the synthetic pangenome of tests/test_left_align_gpu.py and the command line."""
import os
import random
import re
import subprocess
import types

import numpy as np
import pytest

from tests import sites_model as M
from tests import test_left_align_gpu as LT  # its synthetic pangenome and line helpers (nothing of it is collected from here)
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
SNV, INS, DEL = M.SNV, M.INS, M.DEL
SLICE, TASK, BLOCK = capi.WFM_SITES_SLICE, capi.WFM_SITES_TASK, capi.WFM_PAV_SCAN_BLOCK
P = M.parse
RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


# ---- 1. the ABI against the model ----
def _v(pos, g, ref, alt):
    return (pos, M.kind_of(ref, alt), g, ref, alt)


def _add_ref(obj, problems):
    probs, words = [], []
    for base, runs, g in problems:
        probs.append((base, len(words), len(runs), g))
        words += M.words(runs)
    return obj.add_ref(probs, words)


def _raw(obj):
    """the table as it came: bytes of the three outputs"""
    sites, alleles, gt = obj.table()
    return sites.tobytes(), alleles, gt.tobytes()


def _decode(n_groups, sites, alleles, gt):
    """[(pos, ref, alt)] and their rows as strings, in the device's order; the fields are checked on the way"""
    out, rows = [], []
    assert sites.dtype.itemsize == 32 and gt.shape == (len(sites), n_groups)
    at = 0
    for i, s in enumerate(sites):
        assert int(s["off"]) == at  # the representatives' bytes lie in site order, without holes
        ref = alleles[at:at + int(s["ref_len"])]
        alt = alleles[at + int(s["ref_len"]):at + int(s["ref_len"]) + int(s["alt_len"])]
        at += len(ref) + len(alt)
        assert int(s["kind"]) == M.kind_of(ref, alt)
        out.append((int(s["pos"]), ref, alt))
        rows.append(gt[i].tobytes().decode())
        assert rows[-1].count("1") == int(s["n_carrier_groups"]) >= 1
    assert at == len(alleles)
    assert [p for p, _, _ in out] == sorted(p for p, _, _ in out)  # ascending pos
    return out, rows


def _assert_model(obj, variants, problems, n_bases, n_groups):
    """the object's table equals the model's for (variants, problems), cell for cell; returns {(pos, ref, alt): row}"""
    got_sites, got_rows = _decode(n_groups, *obj.table())
    want_sites, want_rows, want_n = M.table(variants, problems, n_bases, n_groups)
    assert len(set(got_sites)) == len(got_sites)  # no site twice
    got = dict(zip(got_sites, got_rows))
    assert sorted(got) == want_sites
    assert [got[s] for s in want_sites] == want_rows
    assert obj.counts()[1] == len(want_sites) and obj.counts()[3] == 0
    return got


def _fresh(gpu, variants, problems, n_bases, n_groups):
    obj = gpu.sites(n_bases, n_groups)
    try:
        obj.add_variants(variants)
        assert not _add_ref(obj, problems).any()
        assert obj.counts()[0] == len(variants)
        return _assert_model(obj, variants, problems, n_bases, n_groups)
    finally:
        obj.close()


def test_one_snv_two_carriers_one_reference(gpu):
    got = _fresh(gpu, [_v(10, 0, b"A", b"G"), _v(10, 1, b"A", b"G")],
                 [(5, P("5=1X5="), 0), (8, P("2=1X9="), 1), (0, P("30="), 2)], 40, 3)
    assert got == {(10, b"A", b"G"): "110"}


def test_an_x_that_spells_another_alt(gpu):
    got = _fresh(gpu, [_v(10, 0, b"A", b"G"), _v(10, 1, b"A", b"T")], [(5, P("5=1X5="), 0), (5, P("5=1X5="), 1)], 40, 2)
    assert got == {(10, b"A", b"G"): "1.", (10, b"A", b"T"): ".1"}


def test_under_a_deletion_and_uncovered(gpu):
    # group 1 deletes [8, 14): the SNV at 10 lies under its D; group 2 has no record there at all
    got = _fresh(gpu, [_v(10, 0, b"A", b"G"), _v(7, 1, b"CAAAAAA", b"C")], [(5, P("5=1X5="), 0), (2, P("6=6D6="), 1), (30, P("5="), 2)], 40, 3)
    assert got[(10, b"A", b"G")] == "1.."
    assert got[(7, b"CAAAAAA", b"C")] == ".1."  # group 0 has an X inside the span


def test_a_deletion_span_over_two_abutting_records(gpu):
    """the REF span [10, 16) of a DEL is covered for group 1 only by [4, 13) of one record and [13, 20) of another; one base short is '.'"""
    v = [_v(10, 0, b"ACGTAC", b"A")]
    refs0 = [(4, P("7=5D8="), 0)]
    got = _fresh(gpu, v, refs0 + [(4, P("9="), 1), (13, P("7="), 1)], 40, 2)
    assert got == {(10, b"ACGTAC", b"A"): "10"}
    got = _fresh(gpu, v, refs0 + [(4, P("9="), 1), (14, P("6="), 1)], 40, 2)  # base 13 is missing
    assert got == {(10, b"ACGTAC", b"A"): "1."}
    got = _fresh(gpu, v, refs0 + [(4, P("9="), 1), (13, P("2="), 1)], 40, 2)  # the span's last base, 15, is missing
    assert got == {(10, b"ACGTAC", b"A"): "1."}
    got = _fresh(gpu, v, refs0 + [(4, P("9="), 1), (13, P("7="), 2)], 40, 3)  # the second half is another group's
    assert got == {(10, b"ACGTAC", b"A"): "1.."}


def test_overlapping_records_of_one_group_one_carrying(gpu):
    got = _fresh(gpu, [_v(10, 0, b"A", b"G")], [(5, P("5=1X5="), 0), (0, P("30="), 0)], 40, 1)
    assert got == {(10, b"A", b"G"): "1"}


def test_two_insertions_at_one_anchor(gpu):
    """each group is '0' on the other's line (= on the anchor) and '1' on its own; the third has an X on the anchor"""
    got = _fresh(gpu, [_v(10, 0, b"A", b"ACC"), _v(10, 1, b"A", b"AT"), _v(10, 2, b"A", b"C")],
                 [(5, P("6=2I5="), 0), (5, P("6=1I5="), 1), (5, P("5=1X5="), 2)], 40, 3)
    assert got == {(10, b"A", b"ACC"): "10.", (10, b"A", b"AT"): "01.", (10, b"A", b"C"): "001"}


def test_soft_masked_alleles_are_one_site_in_upper_case(gpu):
    got = _fresh(gpu, [_v(10, 0, b"a", b"g"), _v(10, 1, b"A", b"G"), _v(20, 0, b"c", b"cTt"), _v(20, 1, b"C", b"Ctt")],
                 [(5, P("5=1X5="), 0), (5, P("5=1X5="), 1)], 40, 2)
    assert got == {(10, b"A", b"G"): "11", (20, b"C", b"CTT"): "11"}


def test_ins_and_del_sharing_an_anchor(gpu):
    got = _fresh(gpu, [_v(10, 0, b"A", b"ACC"), _v(10, 1, b"ACG", b"A")], [(5, P("6=2I9="), 0), (5, P("6=2D7="), 1)], 40, 2)
    assert got == {(10, b"A", b"ACC"): "10", (10, b"ACG", b"A"): "01"}  # an I takes no target base: group 0's = bases cover [10, 13)


BASES = b"ACGT"


def _distinct_sites(n, n_groups, seed):
    """n distinct SNV sites (three ALTs per position), each carried by one to three groups, in shuffled order"""
    rng = random.Random(seed)
    out = []
    for k in range(n):
        pos, a = k // 3, k % 3
        ref = BASES[pos % 4:pos % 4 + 1]
        alt = BASES[(pos + 1 + a) % 4:(pos + 1 + a) % 4 + 1]
        for g in rng.sample(range(n_groups), min(n_groups, rng.randint(1, 3))):
            out.append(_v(pos, g, ref, alt))
    rng.shuffle(out)
    return out


@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK - 1, 4 * BLOCK, 4 * BLOCK + 1])
def test_site_counts_on_the_scan_block(gpu, n):
    n_bases = n // 3 + 2
    refs = [(0, P("%d=" % (n_bases // 2)), 0), (n_bases // 3, P("%d=" % (n_bases // 2)), 1)]
    got = _fresh(gpu, _distinct_sites(n, 4, n), refs, n_bases, 4)
    assert len(got) == n


def test_one_site_carried_by_1500_groups(gpu):
    """its records cross a scan block; neighbours before and behind it"""
    v = [_v(3, g, b"A", b"C") for g in range(0, 1600, 2)] + [_v(7, g, b"G", b"T") for g in range(1500)] + [_v(9, g, b"T", b"TA") for g in range(1, 1600, 3)]
    random.Random(5).shuffle(v)
    got = _fresh(gpu, v, [(0, P("12="), g) for g in range(0, 1600, 7)], 12, 1600)
    assert got[(7, b"G", b"T")].count("1") == 1500


@pytest.mark.parametrize("n_groups", [1, 8, 300])
def test_group_counts(gpu, n_groups):
    rng = random.Random(n_groups)
    v = [_v(rng.randrange(50), rng.randrange(n_groups), b"A", rng.choice([b"C", b"G", b"AT"])) for _ in range(400)]
    refs = [(rng.randrange(40), P("%d=1X%d=" % (rng.randint(1, 5), rng.randint(1, 5))), rng.randrange(n_groups)) for _ in range(60)]
    _fresh(gpu, v, refs, 60, n_groups)


def test_all_variants_at_one_pos_and_the_edges_of_the_target(gpu):
    rng = random.Random(3)
    alts = [bytes(rng.choice(BASES) for _ in range(rng.randint(1, 6))) for _ in range(300)]
    v = [_v(17, rng.randrange(8), b"A", b"A" + a) for a in alts] + [_v(17, rng.randrange(8), b"A", b"C") for _ in range(20)]
    _fresh(gpu, v, [(10, P("10="), 0), (17, P("1="), 1), (18, P("5="), 2)], 30, 8)
    # pos 0, and REF spans that end at n_bases exactly
    got = _fresh(gpu, [_v(0, 0, b"A", b"C"), _v(29, 1, b"G", b"T"), _v(26, 0, b"ACGT", b"A")], [(0, P("30="), 2), (0, P("1="), 1), (26, P("3="), 1)], 30, 3)
    assert got == {(0, b"A", b"C"): "100", (29, b"G", b"T"): ".10", (26, b"ACGT", b"A"): "1.0"}


def _ins(length, seed):
    rng = random.Random(seed)
    return b"A" + bytes(rng.choice(BASES) for _ in range(length))


@pytest.mark.parametrize("total", [SLICE - 1, SLICE, SLICE + 1, TASK - 1, TASK, TASK + 1, 70001])
def test_long_alleles(gpu, total):
    """REF + ALT of `total` bytes (an insertion of total - 2): identical in two groups it is one site with two carriers; differing in the
    last byte only, or in the first inserted byte only, it is two sites"""
    a = _ins(total - 2, total)
    last = a[:-1] + (b"C" if a[-1:] != b"C" else b"G")
    first = a[:1] + (b"C" if a[1:2] != b"C" else b"G") + a[2:]
    refs = [(0, P("20="), 0), (0, P("20="), 1), (0, P("20="), 2)]
    got = _fresh(gpu, [_v(5, 0, b"A", a), _v(5, 1, b"A", a.lower())], refs, 20, 3)
    assert got == {(5, b"A", a): "110"}
    got = _fresh(gpu, [_v(5, 0, b"A", a), _v(5, 1, b"A", last), _v(5, 2, b"A", a)], refs, 20, 3)
    assert got == {(5, b"A", a): "101", (5, b"A", last): "010"}
    got = _fresh(gpu, [_v(5, 0, b"A", first), _v(5, 1, b"A", a), _v(6, 2, b"A", a)], refs, 20, 3)
    assert got == {(5, b"A", first): "100", (5, b"A", a): "010", (6, b"A", a): "001"}


def test_a_long_deletion_and_a_long_insertion_among_short_ones(gpu):
    rng = random.Random(11)
    ref = bytes(rng.choice(BASES) for _ in range(3 * TASK + 5))
    v = [_v(100, 0, ref, ref[:1]), _v(100, 1, ref.lower(), ref[:1]), _v(100, 2, ref[:-1], ref[:1]), _v(100, 2, ref[:1], ref), _v(100, 0, ref[:1], ref)]
    v += _distinct_sites(200, 3, 2)
    rng.shuffle(v)
    n_bases = 100 + len(ref) + 10
    _fresh(gpu, v, [(0, P("%d=" % n_bases), 1), (50, P("%d=3D9=" % (len(ref) + 40)), 2)], n_bases, 3)


# ---- 2. collisions ----
def test_a_collision_fails_the_call_and_the_object_stays_good(gpu, monkeypatch):
    obj = gpu.sites(40, 2)
    try:
        v = [_v(10, 0, b"A", b"G"), _v(10, 1, b"A", b"T")]
        obj.add_variants(v)
        refs = [(5, P("5=1X5="), 0), (5, P("5=1X5="), 1)]
        _add_ref(obj, refs)
        monkeypatch.setenv("WFM_SITES_HASH_BITS", "0")
        with pytest.raises(capi.WfmError, match=r"\(%d\).*collision" % capi.WFM_E_INTERNAL):
            obj.table()
        assert obj.counts()[3] == 1 and obj.counts()[1] == 0
        monkeypatch.delenv("WFM_SITES_HASH_BITS")
        assert _assert_model(obj, v, refs, 40, 2) == {(10, b"A", b"G"): "1.", (10, b"A", b"T"): ".1"}
        assert gpu.align([(b"ACGT", b"ACGT")])[0].status == 0
    finally:
        obj.close()


# ---- 3. a set function ----
def _random_case(seed=7, n_bases=5000, n_groups=8, n_var=4000, n_ref=300):
    rng = random.Random(seed)
    target = bytes(rng.choice(BASES) for _ in range(n_bases))
    variants = []
    for _ in range(n_var):
        pos, g, kind = rng.randrange(n_bases - 40), rng.randrange(n_groups), rng.choice([SNV, SNV, SNV, INS, DEL])
        pos = pos // 3 * 3 if rng.random() < 0.7 else pos  # so that groups meet on sites
        ref = target[pos:pos + 1]
        if kind == SNV:
            alt = rng.choice([b for b in (b"A", b"C", b"G", b"T") if b != ref][:2])
            if rng.random() < 0.1:
                ref, alt = ref.lower(), alt.lower()
            variants.append((pos, SNV, g, ref, alt))
        elif kind == INS:
            variants.append((pos, INS, g, ref, ref + rng.choice([b"A", b"AC", b"ACG", b"T" * 7, b"G" * 90])))
        else:
            variants.append((pos, DEL, g, target[pos:pos + rng.choice([2, 3, 5, 30])], ref))
    problems = []
    for _ in range(n_ref):
        base = rng.randrange(n_bases - 400)
        runs, left = [], rng.randint(20, 390)
        while left > 0:
            n = min(left, rng.randint(1, 40))
            op = rng.choice("====XDI") if runs and runs[-1][1] == "=" else "="
            runs.append((n, op))
            left -= n if op != "I" else 0
        problems.append((base, runs, rng.randrange(n_groups)))
    return types.SimpleNamespace(n_bases=n_bases, n_groups=n_groups, variants=variants, problems=problems)


@pytest.fixture(scope="module")
def rcase(gpu):
    """the random case and the bytes of its table from ONE call of each add: made once, never changed"""
    c = _random_case()
    obj = gpu.sites(c.n_bases, c.n_groups)
    try:
        obj.add_variants(c.variants)
        assert not _add_ref(obj, c.problems).any()
        _assert_model(obj, c.variants, c.problems, c.n_bases, c.n_groups)
        c.raw = _raw(obj)
        assert _raw(obj) == c.raw  # the table taken twice
        assert obj.counts()[0] == len(c.variants) and obj.counts()[3] == 0
        c.n_sites = obj.counts()[1]
        c.gt = np.frombuffer(c.raw[2], dtype=np.uint8).reshape(c.n_sites, c.n_groups)
        c.sites = np.frombuffer(c.raw[0], dtype=capi.SITE_DTYPE)
    finally:
        obj.close()
    return c


def _in_three(gpu, c, order):
    obj = gpu.sites(c.n_bases, c.n_groups)
    thirds_v = [c.variants[k::3] for k in range(3)]
    thirds_p = [c.problems[k::3] for k in range(3)]
    for k in order:
        obj.add_variants(thirds_v[k][::-1])
        _add_ref(obj, thirds_p[k])
    return obj


def test_three_calls_in_permuted_order(gpu, rcase):
    for order in [(2, 0, 1), (1, 2, 0)]:
        obj = _in_three(gpu, rcase, order)
        try:
            assert _raw(obj) == rcase.raw
        finally:
            obj.close()


def test_a_union_after_every_add(gpu, rcase, monkeypatch):
    monkeypatch.setenv("WFM_SITES_MB", "0.000001")
    obj = _in_three(gpu, rcase, (0, 1, 2))
    try:
        assert obj.counts()[2] > 0  # the = union was taken by the adds
        assert _raw(obj) == rcase.raw
    finally:
        obj.close()


def test_export_of_two_objects_imported_into_a_third(gpu, rcase):
    c = rcase
    a, b, t = gpu.sites(c.n_bases, c.n_groups), gpu.sites(c.n_bases, c.n_groups), gpu.sites(c.n_bases, c.n_groups)
    try:
        half = len(c.variants) // 2
        a.add_variants(c.variants[:half]); _add_ref(a, c.problems[::2])
        b.add_variants(c.variants[half:]); _add_ref(b, c.problems[1::2])
        for obj in (b, a):
            v, alleles, segs = obj.export()
            assert v.dtype.itemsize == 32 and alleles == alleles.upper()
            t.import_(v, alleles, segs)
        assert t.counts()[0] == len(c.variants)
        assert _raw(t) == c.raw
    finally:
        for obj in (a, b, t):
            obj.close()


def test_rows_in_several_chunks(gpu, rcase, monkeypatch):
    c = rcase
    monkeypatch.setenv("WFM_SITES_OUT_MB", "%.6f" % (c.n_sites * c.n_groups / 5 / 1048576.0))
    obj = _in_three(gpu, c, (0, 1, 2))
    try:
        assert _raw(obj) == c.raw
        monkeypatch.setenv("WFM_SITES_OUT_MB", "0")  # one row a chunk
        assert _raw(obj) == c.raw
    finally:
        obj.close()


def test_pav_is_what_it_was_and_contains_the_reference_cells(gpu, rcase):
    """a pav object fed the same problems returns the =/X union of tests/pav_model.py, as before; every '0' cell's span is covered in it"""
    from tests import pav_model as PM
    c = rcase
    pav = gpu.pav(c.n_bases, c.n_groups)
    try:
        probs, words = [], []
        for base, runs, g in c.problems:
            probs.append((base, len(words), len(runs), g))
            words += M.words(runs)
        assert not pav.add(probs, words).any()
        assert pav.counts()[0] == PM.segments_of(c.problems)
        mask = PM.mask_of(c.problems, c.n_bases, c.n_groups)
        e = pav.export()
        assert list(zip(e["start"].tolist(), e["length"].tolist(), e["group"].tolist())) == PM.union_of(mask)
        iv = [(int(s["pos"]), int(s["pos"]) + int(s["ref_len"])) for s in c.sites]
        cells = pav.matrix(iv)
        assert cells.tolist() == PM.matrix_of(mask, iv)
        zero = c.gt == ord("0")
        assert zero.any() and (cells[zero] == np.repeat(c.sites["ref_len"][:, None], c.n_groups, axis=1)[zero]).all()
    finally:
        pav.close()


# ---- 4. refusals ----
def test_refusals_add_nothing_and_leave_the_handle_usable(gpu):
    obj = gpu.sites(100, 3)
    try:
        assert obj.table()[0].size == 0 and obj.counts() == (0, 0, 0, 0)  # an empty object
        v, problems = [_v(10, 0, b"A", b"G")], [(5, P("5=1X5="), 0)]
        obj.add_variants(v)
        _add_ref(obj, problems)
        good = (50, SNV, 1, b"C", b"T")
        bad = [
            ((50, 3, 1, b"C", b"T"), "kind"),
            ((50, SNV, 1, b"C", b"TT"), "lengths"),
            ((50, SNV, 1, b"CC", b"T"), "lengths"),
            ((50, INS, 1, b"C", b"T"), "lengths"),
            ((50, INS, 1, b"CC", b"CTT"), "lengths"),
            ((50, DEL, 1, b"C", b"T"), "lengths"),
            ((50, DEL, 1, b"CTT", b"CT"), "lengths"),
            ((50, SNV, 1, b"", b"T"), "lengths"),
            ((100, SNV, 1, b"C", b"T"), "beyond"),
            ((98, DEL, 1, b"CTT", b"C"), "beyond"),
            ((50, SNV, 3, b"C", b"T"), "group"),
        ]
        for rec, word in bad:
            with pytest.raises(capi.WfmError, match=r"\(%d\).*%s" % (capi.WFM_E_ARG, word)):
                obj.add_variants([good, rec])  # the good one before it is not added either
            assert obj.counts()[0] == 1
        # an allele range outside the bytes
        arr, alleles = capi.Sites.pack([good])
        arr["off"] = 1
        with pytest.raises(capi.WfmError, match=r"\(%d\).*allele bytes" % capi.WFM_E_ARG):
            obj.add_variants(arr, alleles)
        arr["off"] = 2 ** 63
        with pytest.raises(capi.WfmError, match=r"\(%d\).*allele bytes" % capi.WFM_E_ARG):
            obj.add_variants(arr, alleles)
        # flagged = problems add nothing: an empty run, a span that leaves the target, a group that is not below n_groups
        flags = _add_ref(obj, [(5, [(3, "="), (0, "="), (2, "=")], 1), (95, P("10="), 1), (5, P("10="), 3)])
        assert flags.tolist() == [capi.WFM_PAV_SPANS] * 3
        assert _assert_model(obj, v, problems, 100, 3) == {(10, b"A", b"G"): "1.."}
        assert gpu.align([(b"ACGT", b"ACGT")])[0].status == 0
    finally:
        obj.close()
    for n_bases, n_groups in [(1 << 40, 1), (10, 1 << 24)]:
        with pytest.raises(capi.WfmError, match=r"wfm_sites_create.*2\^40 bases and 2\^24 groups"):
            gpu.sites(n_bases, n_groups)
    assert gpu.align([(b"ACGT", b"ACGT")])[0].status == 0


# ---- 5. the align driver ----
def _align(handles, case, out, gt, vcf=None, left=False, **params):
    capi.set_genotypes(gt)
    capi.set_variants(vcf)
    capi.set_left_align(left)
    try:
        if len(handles) == 1:
            capi.align_paf(handles[0], case.fa, case.paf, out, params=params or None)
        else:
            capi.align_paf_multi(handles, case.fa, case.paf, out, params=params or None)
        return (open(out, "rb").read(), (open(gt).read().splitlines() if gt else None), capi.genotypes_counts(),
                (open(vcf).read().splitlines() if vcf else None), capi.variants_counts())
    finally:
        capi.set_genotypes(None)
        capi.set_variants(None)
        capi.set_left_align(False)


@pytest.fixture(scope="module")
def case(gpu, tmp_path_factory):
    """the pangenome, its mapping rows, the aligned PAF of a run without the switch, the VCF of a run with --variants alone, and the PAF and
    the two files of one with both: made once, never changed"""
    d = str(tmp_path_factory.mktemp("genotypes"))
    fa, paf, seqs = LT._make_case(d)
    c = types.SimpleNamespace(dir=d, fa=fa, paf=paf, seqs=seqs, names=list(seqs), lengths=[len(s) for s in seqs.values()])
    c.cols = M.columns(c.names)
    assert c.cols == ["hap0#1", "hap1#1", "hap2#1", "hap3#1", "hap9#1"]
    c.text, none, counts, _, _ = _align([gpu], c, os.path.join(d, "plain.paf"), None)
    assert none is None and counts == (0, 0, 0, 0)  # nothing new runs without the switch
    c.lines = c.text.decode().splitlines()
    assert len(c.lines) >= 20
    _, _, _, c.vcf_alone, c.vcf_counts_alone = _align([gpu], c, os.path.join(d, "v.paf"), None, vcf=os.path.join(d, "v.vcf"))
    c.with_text, c.gt, c.counts, c.vcf, c.vcf_counts = _align([gpu], c, os.path.join(d, "with.paf"), os.path.join(d, "with.gt.vcf"), vcf=os.path.join(d, "with.vcf"))
    c.version = c.gt[1].split(" ", 1)[1]
    return c


def _want(case, lines):
    variants, problems, masked = M.inputs_of_paf(lines, lambda f: LT._bases(case.seqs, f), LT._split, case.names, case.lengths, case.cols)
    return M.file_of(case.version, case.names, case.lengths, case.cols, variants, problems), len(variants)


def _body(lines):
    return [l for l in lines if not l.startswith("#")]


def test_driver_leaves_the_paf_and_the_variants_file_alone(gpu, case):
    assert case.with_text == case.text
    assert case.vcf == case.vcf_alone and case.vcf_counts == case.vcf_counts_alone and case.vcf_counts[1] > 100
    # the switch off again: the bytes of the run without it, no counts
    again, none, counts, _, _ = _align([gpu], case, os.path.join(case.dir, "off.paf"), None)
    assert again == case.text and none is None and counts == (0, 0, 0, 0)


def test_driver_file_is_the_model_of_its_own_paf(gpu, case):
    want, n_variants = _want(case, case.lines)
    assert case.gt == want
    assert re.fullmatch(r"##source=wfmash-hip \S+", case.gt[1])
    n_sites = len(_body(case.gt))
    assert case.counts == (len(case.lines), n_sites, n_variants - n_sites, 0)
    assert 100 < n_sites <= n_variants == case.vcf_counts[1]
    cells = "".join("".join(l.split("\t")[9:]) for l in _body(case.gt))
    assert cells.count("0") > 0 and cells.count("1") >= n_sites and cells.count(".") > 0
    # sorted by (sequence in index order, POS, REF, ALT)
    keys = [(case.names.index(f[0]), int(f[1]), f[3].encode(), f[4].encode()) for f in (l.split("\t") for l in _body(case.gt))]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_driver_ones_against_the_fastas(gpu, case):
    """every '1' cell has a line of the --variants file of the same run behind it -- same CHROM, POS, REF, ALT, a query of the cell's group --
    whose REF is the target at POS and whose ALT is that query at [QSTART, QEND); and every such line is a '1'"""
    carried = {}
    for l in _body(case.vcf):
        chrom, pos, _, ref, alt, _, _, info = l.split("\t")
        kv = dict(x.split("=") for x in info.split(";"))
        a, b = int(kv["QSTART"]), int(kv["QEND"])
        assert case.seqs[chrom][int(pos) - 1:int(pos) - 1 + len(ref)].upper() == ref.encode()
        q = case.seqs[kv["QNAME"]][a:b]
        if kv["QSTRAND"] == "-":
            q = q[::-1].translate(RC)
        snv = len(ref) == 1 and len(alt) == 1
        assert q.upper() == (alt if snv else alt[1:]).encode()
        carried.setdefault((chrom, pos, ref, alt), set()).add(case.cols.index(M.group_key(kv["QNAME"])))
    ones = {}
    for l in _body(case.gt):
        f = l.split("\t")
        ones[(f[0], f[1], f[3], f[4])] = {g for g, c in enumerate(f[9:]) if c == "1"}
    assert ones == carried


def test_driver_resident_threads_and_two_handles(gpu, case):
    for tag, params in (("r", {"resident_sequences": 1}), ("t8", {"threads": 8}), ("t1", {"threads": 1})):
        text, gt, counts, _, _ = _align([gpu], case, os.path.join(case.dir, tag + ".paf"), os.path.join(case.dir, tag + ".gt.vcf"), **params)
        assert text == case.text and gt == case.gt and counts == case.counts, tag  # (without --variants beside it, too)
    h2 = capi.Handle(0)
    try:
        text, gt, counts, _, _ = _align([gpu, h2], case, os.path.join(case.dir, "m.paf"), os.path.join(case.dir, "m.gt.vcf"))
    finally:
        h2.close()
    assert text == case.text and gt == case.gt and counts == case.counts


def test_driver_two_gpus(gpu, case):
    if capi.load().wfm_device_count() < 2:
        pytest.skip("one GPU on this node: the two-GPU file cannot be made")
    h2 = capi.Handle(1)
    try:
        text, gt, counts, _, _ = _align([gpu, h2], case, os.path.join(case.dir, "g2.paf"), os.path.join(case.dir, "g2.gt.vcf"))
    finally:
        h2.close()
    assert text == case.text and gt == case.gt and counts == case.counts


def test_driver_with_left_align(gpu, case):
    text, gt, counts, _, _ = _align([gpu], case, os.path.join(case.dir, "la.paf"), os.path.join(case.dir, "la.gt.vcf"), left=True)
    assert text != case.text  # the pangenome plants gaps in repeats
    want, n_variants = _want(case, text.decode().splitlines())
    assert gt == want != case.gt  # the normalised runs' variants
    assert counts == (len(case.lines), len(_body(gt)), n_variants - len(_body(gt)), 0)


def test_driver_filtered_records_add_nothing(gpu, case):
    text, gt, counts, _, _ = _align([gpu], case, os.path.join(case.dir, "f.paf"), os.path.join(case.dir, "f.gt.vcf"), min_alignment_length=5000)
    lines = text.decode().splitlines()
    assert 0 < len(lines) < len(case.lines) and counts[0] == len(lines) and counts[3] == 0
    assert gt == _want(case, lines)[0] != case.gt


# ---- 6. the command line ----
def _cli(args, cwd=None):
    # (a fresh child process, ended by `timeout` if it hangs)
    return subprocess.run(["timeout", "-k", "10", "120", CLI] + args, capture_output=True, text=True, cwd=cwd)


def test_cli_writes_the_same_file_beside_the_other_switches(case):
    d = case.dir
    out, gt, vcf = os.path.join(d, "cli.paf"), os.path.join(d, "cli.gt.vcf"), os.path.join(d, "cli.vcf")
    r = _cli(["--genotypes", gt, "--variants", vcf, "--pav-window", "3000", "--pav-out", os.path.join(d, "cli.pav"), "--chain", os.path.join(d, "cli.chain"),
              "--gpus", "1", "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(out, "rb").read() == case.text and open(gt).read().splitlines() == case.gt and open(vcf).read().splitlines() == case.vcf
    assert "[wfmash::genotypes] %d records added, %d sites written, %d variants merged away, %d records left alone" % case.counts in r.stderr
    assert os.path.getsize(os.path.join(d, "cli.pav")) > 0 and os.path.getsize(os.path.join(d, "cli.chain")) > 0
    # alone, too
    r = _cli(["--genotypes", gt, "-i", case.paf, "--out", out, case.fa])
    assert r.returncode == 0, r.stderr[-500:]
    assert open(out, "rb").read() == case.text and open(gt).read().splitlines() == case.gt
