"""All eight across-record outputs of the align driver in ONE run (--variants, --coverage, --lift, --chain, --pav, --genotypes, --chain-net,
--transitive) over two handles of a device and several batches, on the synthetic pangenome of tests/test_left_align_gpu.py: every file,
the PAF and every switch's counts are, byte for byte, those of a single-handle run with that switch alone.  A pass that took another
pass's object, batch number, tables or counts would show here and nowhere else: no other test turns on more than three switches."""
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


def _run(handles, fa, paf, bed, d, tag, names):
    """one align run with the switches `names` on: (PAF bytes, {switch: file bytes}, {switch: counts}, batches)"""
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
    finally:
        for n in names:
            SWITCHES[n][1]()
    return open(out, "rb").read(), {n: open(files[n], "rb").read() for n in names}, counts, int(summ.batches)


def test_all_eight_switches_on_one_run_over_two_handles(gpu, tmp_path):
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
        text, files, counts, batches = _run([gpu, h2], fa, paf, bed, d, "all", list(SWITCHES))
    finally:
        h2.close()
    assert batches >= 4 and text.count(b"\n") >= 20
    for n in SWITCHES:
        one_text, one_files, one_counts, _ = _run([gpu], fa, paf, bed, d, "only_" + n, [n])
        assert one_text == text, n
        assert len(one_files[n]) > 0 and one_files[n] == files[n], n
        assert any(one_counts[n]) and one_counts[n] == counts[n], n
