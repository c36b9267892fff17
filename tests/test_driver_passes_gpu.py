"""All eight across-record outputs of the align driver in ONE run (--variants, --coverage, --lift, --chain, --pav, --genotypes, --chain-net,
--transitive) over two handles of a device and several batches, on the synthetic pangenome of tests/test_left_align_gpu.py: every file,
the PAF and every switch's counts are, byte for byte, those of a single-handle run with that switch alone.  A pass that took another
pass's object, batch number, tables or counts would show here and nowhere else: no other test turns on more than three switches.

The six --*-paf modes feed the same passes and stages from the PAF that run wrote: their files are that run's byte for byte, in one batch
and in batches of 7 lines (WFM_PAF_BATCH_RECORDS), their counts are the run's where the two count the same thing, and they leave every
process-wide switch count alone while the switches are on."""
import os

import pytest

from tests import test_left_align_gpu as LT  # its synthetic pangenome (nothing of it is collected from here)
from wfmash_amd import capi

pytestmark = pytest.mark.gpu

# switch -> (set it for a run that writes `out` and reads `bed`, clear it, its counts)
SWITCHES = {
    "variants": (lambda out, bed: capi.set_variants(out), lambda: capi.set_variants(None), capi.variants_counts),
    "coverage": (lambda out, bed: capi.set_coverage(out), lambda: capi.set_coverage(None), capi.coverage_counts),
    "lift": (lambda out, bed: capi.set_lift(bed, out), lambda: capi.set_lift(None, None), capi.lift_counts),
    "chain": (lambda out, bed: capi.set_chain(out), lambda: capi.set_chain(None), capi.chain_counts),
    "pav": (lambda out, bed: capi.set_pav(bed, 0, out), lambda: capi.set_pav(None, 0, None), capi.pav_counts),
    "genotypes": (lambda out, bed: capi.set_genotypes(out), lambda: capi.set_genotypes(None), capi.genotypes_counts),
    "chain_net": (lambda out, bed: capi.set_chain_net(out), lambda: capi.set_chain_net(None), capi.chain_net_counts),
    "transitive": (lambda out, bed: capi.set_transitive(bed, out, 2), lambda: capi.set_transitive(None, None), capi.transitive_counts),
}


ALL_COUNTS = [capi.verify_counts, capi.left_align_counts, capi.cs_counts, capi.variants_counts, capi.coverage_counts, capi.lift_counts, capi.chain_counts,
              capi.maf_counts, capi.chain_net_counts, capi.transitive_counts, capi.pav_counts, capi.genotypes_counts, capi.verify_optimal_counts]

# mode -> the call over (handle, fa, aligned PAF, bed, out) that returns its out[4]; the switch whose file it makes
OFFLINE = {
    "coverage": lambda h, fa, paf, bed, out: capi.coverage_paf(h, fa, paf, out),
    "lift": lambda h, fa, paf, bed, out: capi.lift_paf(h, fa, paf, bed, out),
    "chain": lambda h, fa, paf, bed, out: capi.chain_paf(h, fa, paf, out),
    "chain_net": lambda h, fa, paf, bed, out: capi.chain_paf(h, fa, paf, None, net_path=out),
    "pav": lambda h, fa, paf, bed, out: capi.pav_paf(h, fa, None, paf, bed, 0, out),
    "transitive": lambda h, fa, paf, bed, out: capi.transitive_paf(h, fa, paf, bed, out, depth=2),
}


def _offline(h, fa, paf, bed, d, tag):
    """the six modes over one aligned PAF: ({mode: file bytes}, {mode: out[4]})"""
    files, outs = {}, {}
    for n, call in OFFLINE.items():
        out = os.path.join(d, tag + "." + n)
        outs[n] = tuple(call(h, fa, paf, bed, out))
        files[n] = open(out, "rb").read()
    return files, outs


def _run(handles, fa, paf, bed, d, tag, names, then=None):
    """one align run with the switches `names` on: (PAF bytes, {switch: file bytes}, {switch: counts}, batches).  then(aligned PAF): called
    while the switches are still on; no switch's counts may move meanwhile"""
    out = os.path.join(d, tag + ".paf")
    files = {n: os.path.join(d, tag + "." + n) for n in names}
    for n in names:
        SWITCHES[n][0](files[n], bed)
    try:
        if len(handles) == 1:
            summ = capi.align_paf(handles[0], fa, paf, out)
        else:
            summ = capi.align_paf_multi(handles, fa, paf, out)
        counts = {n: tuple(SWITCHES[n][2]()) for n in names}
        if then is not None:
            before = [tuple(c()) for c in ALL_COUNTS]
            then(out)
            assert [tuple(c()) for c in ALL_COUNTS] == before
    finally:
        for n in names:
            SWITCHES[n][1]()
    return open(out, "rb").read(), {n: open(files[n], "rb").read() for n in names}, counts, int(summ.batches)


def test_all_eight_switches_on_one_run_over_two_handles(gpu, tmp_path, monkeypatch):
    d = str(tmp_path)
    fa, paf, seqs = LT._make_case(d)
    names = list(seqs)
    bed = os.path.join(d, "iv.bed")
    with open(bed, "w") as f:  # intervals on three sequences, one that abuts a sequence's end, two lines to skip
        f.write("# intervals\n")
        for k, name in enumerate(names[:3]):
            for j in range(4):
                f.write("%s\t%d\t%d\tiv%d_%d\n" % (name, 1500 + 9000 * j + 100 * k, 4500 + 9000 * j + 100 * k, k, j))
        f.write("%s\t%d\t%d\tend\n" % (names[0], len(seqs[names[0]]) - 700, len(seqs[names[0]])))
        f.write("nobody\t0\t10\n%s\t5\n" % names[1])
    h2 = capi.Handle(0)
    try:
        offline = {}
        text, files, counts, batches = _run([gpu, h2], fa, paf, bed, d, "all", list(SWITCHES),
                                            then=lambda aligned: offline.update(zip(("files", "outs"), _offline(gpu, fa, aligned, bed, d, "offline"))))
    finally:
        h2.close()
    assert batches >= 4 and text.count(b"\n") >= 20
    # the --*-paf modes over the PAF of that run: its files; its counts, where both count the same thing
    assert any(counts["coverage"][:3]) and all(len(files[n]) > 0 and offline["files"][n] == files[n] for n in OFFLINE), [n for n in OFFLINE if offline["files"][n] != files[n]]
    cov = offline["outs"]["coverage"]  # (lines added, lines skipped, covered bases, sum of depth) against (records added, covered bases, sum of depth, intervals)
    assert (cov[0], cov[2], cov[3]) == counts["coverage"][:3] and cov[1] == 0
    for n in ("lift", "chain", "chain_net", "pav", "transitive"):
        assert offline["outs"][n] == counts[n], n
    # ... and in batches of 7 lines: orders, chain ids and the batches' lists carry over the batch boundary
    n_lines = text.count(b"\n")
    assert n_lines > 2 * 7  # (three batches at least)
    monkeypatch.setenv("WFM_PAF_BATCH_RECORDS", "7")
    small_files, small_outs = _offline(gpu, fa, os.path.join(d, "all.paf"), bed, d, "offline7")
    monkeypatch.delenv("WFM_PAF_BATCH_RECORDS")
    assert small_files == offline["files"] and small_outs == offline["outs"]
    for n in SWITCHES:
        one_text, one_files, one_counts, _ = _run([gpu], fa, paf, bed, d, "only_" + n, [n])
        assert one_text == text, n
        assert len(one_files[n]) > 0 and one_files[n] == files[n], n
        assert any(one_counts[n]) and one_counts[n] == counts[n], n
