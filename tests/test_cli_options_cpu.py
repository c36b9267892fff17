"""CPU tests of the command line options that complete the reference's parser (parse_args.hpp:61-138): --hg-filter,
-B/--tmp-base, -Z/--keep-temp, --quiet, --ani-sketch-size and --streaming-minhash; and of the restatement of
sketchSequenceStreaming (tests/streaming_sketch_ref.py) the GPU tests of --streaming-minhash compare against."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pymap
from tests import filter_cases as FC
from tests import streaming_sketch_ref as SR
from wfmash_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("value,message", [
    ("2,1", "hypergeometric filter requires 3 comma-separated values: numerator,ani-diff,confidence"),
    ("2,1,95,4", "hypergeometric filter requires 3 comma-separated values: numerator,ani-diff,confidence"),
    ("0.5,0,99.9", "hg-filter numerator must be >= 1.0"),
    ("2,x,95", "--hg-filter expects numbers"),
    ("two,1,95", "--hg-filter expects numbers"),
], ids=["two_values", "four_values", "numerator_below_1", "ani_diff_not_a_number", "numerator_not_a_number"])
def test_hg_filter_refused(tmp_path, value, message):
    r = _cli(["-m", "--hg-filter", value, "target.fa"], tmp_path)
    assert r.returncode == 1 and message in r.stderr


def test_ani_sketch_size_needs_an_integer(tmp_path):
    r = _cli(["-m", "--ani-sketch-size", "many", "target.fa"], tmp_path)
    assert r.returncode == 1 and "--ani-sketch-size expects an integer" in r.stderr


def test_tmp_base_checked_before_any_device(tmp_path):
    """map + align with a missing -B directory: refused before a device is opened, and no hand-off file anywhere"""
    fa = FC.write_fai(str(tmp_path))
    r = _cli(["-B", "/nonexistent/dir", fa], tmp_path)
    assert r.returncode == 1
    assert "(-B) /nonexistent/dir does not exist or is not writable" in r.stderr
    assert "device" not in r.stderr
    ro = tmp_path / "file_not_dir"
    ro.write_text("")
    r = _cli(["-B", str(ro), fa], tmp_path)
    assert r.returncode == 1 and "is not writable" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("wfmash-")]


def test_help_lists_the_options(tmp_path):
    r = _cli(["--help"], tmp_path)
    assert r.returncode == 0
    for opt in ["--hg-filter", "--ani-sketch-size", "--streaming-minhash", "-B DIR", "-Z", "--quiet"]:
        assert opt in r.stderr


def test_options_accepted_without_effect_on_external_seeds(tmp_path):
    """-K -m runs on the host only; --streaming-minhash has no effect with -K (as in the reference), the hypergeometric
    parameters are read only by L2, --quiet and --ani-sketch-size by nothing: the output is the same byte for byte."""
    fa = FC.write_fai(str(tmp_path))
    seeds = str(tmp_path / "seeds.paf")
    length = dict(FC.NAMES)
    lines = []
    for i in range(30):
        q0, t0 = i * 1000, 5000 + i * 1000
        lines.append("\t".join(["A#1#c1", str(length["A#1#c1"]), str(q0), str(q0 + 1000), "+", "B#1#c1", str(length["B#1#c1"]),
                                str(t0), str(t0 + 1000), "0", "1000", "255", "id:f:0.97"]))
    lines.append("\t".join(["B#1#c2", "50000", "100", "2100", "-", "C#1#c1", str(length["C#1#c1"]), "7000", "9000", "0", "2000", "255"]))
    with open(seeds, "w") as f:
        f.write("".join(l + "\n" for l in lines))
    plain, extra = str(tmp_path / "plain.paf"), str(tmp_path / "extra.paf")
    r0 = _cli(["-m", "-p", "90", "-K", seeds, "--out", plain, fa], tmp_path)
    assert r0.returncode == 0, r0.stderr
    r1 = _cli(["-m", "-p", "90", "-K", seeds, "--quiet", "--ani-sketch-size", "500", "--streaming-minhash", "--hg-filter", "2,1,95",
               "--out", extra, fa], tmp_path)
    assert r1.returncode == 0, r1.stderr
    got = open(extra).read()
    assert got == open(plain).read() and len(got.splitlines()) >= 2


# ---- the restatement of sketchSequenceStreaming against the brute-force statement

needs_ref = pytest.mark.skipif(not pymap.have_ref(), reason="oracle/_ref/libref_map.so not built (needs the reference tree)")


def _with_ns(seq):
    b = bytearray(seq)
    b[5] = ord("N")           # among the first k bases: the head counter covers k-mers 0..5 only
    b[700] = ord("n")
    b[1500:1503] = b"NNR"     # R is not ACGT: an N after upper-casing
    return bytes(b)


def _lowercase(seq):
    return seq[:400] + seq[400:1600].lower() + seq[1600:]


def _tandem(seed):
    unit = synth.random_dna(seed + 1, 37)
    return synth.random_dna(seed, 500) + unit * 60 + synth.random_dna(seed + 2, 500)


def _palindromes(seed):
    return synth.random_dna(seed, 600) + b"ACGT" * 12 + synth.random_dna(seed + 1, 300) + b"GGATCC" * 3 + synth.random_dna(seed + 2, 600)


CASES = {
    "n_head_and_body": lambda: _with_ns(synth.random_dna(11, 3000)),
    "lowercase": lambda: _lowercase(synth.random_dna(12, 3000)),
    "tandem_repeat": lambda: _tandem(13),
    "palindromes_even_k": lambda: _palindromes(14),
    "short_s_larger": lambda: synth.random_dna(15, 140),
}


@needs_ref
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("k,s", [(15, 1), (15, 200), (16, 37), (16, 4096), (19, 500)])
def test_restatement_equals_brute_force(case, k, s):
    seq = CASES[case]()
    got = SR.streaming_sketch(seq, k, 1000, s, seq_id=3)
    exp = SR.brute_force(seq, k, 1000, s, seq_id=3)
    assert got.tobytes() == exp.tobytes()
    assert 0 < len(got) <= s
    assert (np.diff(got["wpos"]) >= 0).all() and (got["wpos_end"] == got["wpos"] + 1000).all() and (got["seqId"] == 3).all()


@needs_ref
def test_restatement_corner_cases_occur():
    """the cases above reach what they are for: duplicate sketch entries, palindromes, the head rule, s beyond the k-mers"""
    rep = SR.streaming_sketch(_tandem(13), 15, 1000, 200)
    assert len(np.unique(rep["hash"])) < len(rep)                    # one hash several times in the sketch: identical records
    pal = _palindromes(14)
    assert any(pymap.get_hash(pal[i:i + 16], "ref") == pymap.get_hash(pal[i:i + 16][::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")), "ref")
               for i in range(600, 650))
    full = SR.streaming_sketch(_palindromes(14), 16, 1000, 100000)
    assert len(full) < len(pal) - 15                                   # the palindromes are not in it
    short = SR.streaming_sketch(CASES["short_s_larger"](), 15, 1000, 500)
    assert len(short) == 140 - 15 + 1 and short["wpos_end"].max() > 140  # every k-mer; wpos_end runs past the end
    head = SR.streaming_sketch(_with_ns(synth.random_dna(11, 3000)), 15, 1000, 100000)
    assert head["wpos"].min() == 6                                     # k-mers 6..14 hold no N and are kept
