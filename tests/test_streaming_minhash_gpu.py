"""GPU tests of --streaming-minhash (the target sketch from one bottom-s MinHash per sequence, wfm_streaming_minmers, and the
index / PAF built from it) against the restatement of sketchSequenceStreaming (tests/streaming_sketch_ref.py), and of the
other options completing the reference's parser on the GPU path: --hg-filter, -B/--tmp-base and -Z/--keep-temp."""
import os
import subprocess

import numpy as np
import pytest

from oracle import map_index as MI
from oracle import map_index_file as IF
from oracle import map_pipeline as MP
from oracle import pyfilter, pymap
from oracle import wflign_host as W
from tests import streaming_sketch_ref as SR
from test_cli_options_cpu import CASES
from test_map_paf_gpu import _pangenome, _write_fasta
from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wfmash_amd", "wfmash-hip")
W_LEN = 1000


@pytest.fixture(scope="module", autouse=True)
def _needs_ref():
    if not (pymap.have_ref() and pyfilter.have_ref()):
        pytest.skip("oracle/_ref is not built (it is compiled from the reference tree by `make -C oracle ref`): no restatement to compare with")


def _unit_with_small_hash(k, frac, n=37):
    """a tandem unit one of whose canonical k-mer hashes lies in the lowest `frac` of the range: repeated, it puts one hash
    into the sketch many times"""
    lim = int(frac * 2 ** 64)
    for seed in range(5000):
        u = synth.random_dna(900 + seed, n)
        t = u * 3
        for i in range(n):
            km = t[i:i + k]
            f, b = pymap.get_hash(km, "ref"), pymap.get_hash(W.revcomp(km), "ref")
            if f != b and min(f, b) < lim:
                return u
    raise AssertionError("no unit found")


def _cut_inside_a_run(recs):
    """the sketch size at which the cut falls between two entries of one hash (the entries of a larger sketch `recs`)"""
    h = np.sort(recs["hash"])
    dup = np.nonzero(h[1:] == h[:-1])[0]
    assert len(dup), "no duplicate hash in the sketch"
    return int(dup[0]) + 1


def _crosses(small, big):
    """the last hash of the sketch `small` has more entries in the larger sketch `big`: its run crosses the cut"""
    last = small["hash"].max()
    return int((big["hash"] == last).sum()) > int((small["hash"] == last).sum())


@pytest.mark.parametrize("k", [15, 16, 19])
@pytest.mark.parametrize("s", [1, 37, 200, 4096])
def test_short_sequences_two_pass(gpu, k, s):
    """sequences too short for the fused form, several in one call with seq ids of their own: N inside the first k bases and
    further on, lower case, a tandem repeat, palindromes, and fewer k-mers than s"""
    seqs = [CASES[c]() for c in CASES]
    ids = [7, 0, 12, 3, 99]
    got = capi.streaming_minmers(gpu, seqs, k, W_LEN, s, seq_ids=ids)
    exp = SR.streaming_sketch_multi(seqs, k, W_LEN, s, ids)
    assert len(got) == len(exp) > 0
    assert got.tobytes() == exp.tobytes()


def test_short_sequence_cut_inside_a_run(gpu):
    seq = CASES["tandem_repeat"]()
    big = SR.streaming_sketch(seq, 15, W_LEN, 4000)
    s = _cut_inside_a_run(big)
    got = capi.streaming_minmers(gpu, [seq], 15, W_LEN, s)
    exp = SR.streaming_sketch(seq, 15, W_LEN, s)
    assert _crosses(exp, big)
    assert got.tobytes() == exp.tobytes()
    # and a sketch that holds several entries of that hash
    got = capi.streaming_minmers(gpu, [seq], 15, W_LEN, s + 3)
    exp = SR.streaming_sketch(seq, 15, W_LEN, s + 3)
    assert len(np.unique(exp["hash"])) < len(exp) and got.tobytes() == exp.tobytes()


@pytest.fixture(scope="module")
def long_seq():
    """more than 2^20 k-mers: N among the first k bases and runs further on, a lower-case stretch, and a tandem repeat whose
    unit holds a hash in the bottom of the range"""
    L = (1 << 20) + 40000
    b = bytearray(synth.random_dna(2024, L))
    b[3] = ord("N")
    b[500000:500040] = b"N" * 40
    b[800000:800003] = b"nRy"
    b[300000:360000] = bytes(b[300000:360000]).lower()
    unit = _unit_with_small_hash(15, 0.0005)
    b[700000:700000 + len(unit) * 50] = unit * 50
    return bytes(b)


@pytest.mark.parametrize("k,s", [(15, "cut"), (16, 4096), (19, 1), (18, 500)], ids=["k15_cut_in_run", "k16_s4096", "k19_s1", "k18_two_pass"])
def test_long_sequence(gpu, long_seq, k, s):
    """(15, 16, 19: the fused form; 18 has none, the two-pass form selects under the same threshold)"""
    nk = len(long_seq) - k + 1
    big = None
    if s == "cut":
        big = SR.streaming_sketch(long_seq, k, W_LEN, 16000)
        s = _cut_inside_a_run(big)
    assert nk > 1 << 20 and 64 * s < nk
    exp = SR.streaming_sketch(long_seq, k, W_LEN, s, seq_id=5)
    got = capi.streaming_minmers(gpu, [long_seq], k, W_LEN, s, seq_ids=[5])
    assert len(got) == s and got.tobytes() == exp.tobytes()
    if big is not None:
        assert _crosses(exp, big)
        # a sketch that holds every entry of that hash
        s2 = int(np.searchsorted(np.sort(big["hash"]), exp["hash"].max(), side="right"))
        exp2 = SR.streaming_sketch(long_seq, k, W_LEN, s2, seq_id=5)
        got2 = capi.streaming_minmers(gpu, [long_seq], k, W_LEN, s2, seq_ids=[5])
        assert len(np.unique(exp2["hash"])) < len(exp2) and got2.tobytes() == exp2.tobytes()
        # with a short sequence after it in the same call
        short = CASES["n_head_and_body"]()
        got2 = capi.streaming_minmers(gpu, [long_seq, short], k, W_LEN, s, seq_ids=[5, 2])
        assert got2.tobytes() == np.concatenate([exp, SR.streaming_sketch(short, k, W_LEN, s, seq_id=2)]).tobytes()


def _streaming_pangenome(seed=61, L=4000):
    """sequences a few windows long (a target sketch of s hashes per sequence maps only where the sequences are short), one of
    which holds a duplicate hash in its sketch"""
    base = synth.random_dna(seed, L)
    seqs = []
    for g, gname in enumerate(["HG01", "HG02", "HG03"]):
        for hap in (1, 2):
            s = synth.mutate(base, 0.005 + 0.01 * g, seed * 100 + g * 10 + hap)
            if g == 1 and hap == 2:
                s = W.revcomp(s)
            if g == 2 and hap == 1:
                s = s[:L // 4] + s[L // 4:L // 2].lower() + s[L // 2:]
            seqs.append((f"{gname}#{hap}#chr1", s))
    rep = synth.random_dna(seed + 5, 1500) + _unit_with_small_hash(15, 0.0005) * 40 + synth.random_dna(seed + 6, 1500)
    seqs.append(("rep#1#chr3", rep))
    seqs.append(("rep#2#chr3", synth.mutate(rep, 0.01, 77)))
    seqs.append(("tiny#1#x", synth.random_dna(seed + 9, 700)))     # shorter than a window: not indexed
    seqs.append(("other#1#chr2", synth.random_dna(seed + 7, 2500)))
    return seqs


def _restated(seqs, s):
    return lambda sq, sid: SR.streaming_sketch(sq, 15, W_LEN, s, sid)


def test_index_from_streaming_records(gpu, tmp_path):
    seqs = _streaming_pangenome()
    fa = str(tmp_path / "pan.fa")
    _write_fasta(fa, seqs)
    idx = str(tmp_path / "pan.idx")
    P = capi.map_default_params(percentage_identity=0.85, auto_pct_identity=0, index_file=idx, write_index=1, streaming_minhash=1)
    summ = capi.map_paf(gpu, fa, str(tmp_path / "none.paf"), params=P)
    S = summ.sketch_size
    assert S == MP.sketch_size(0.85, W_LEN, 15) == 49
    recs = [SR.streaming_sketch(sq, 15, W_LEN, S, sid) for sid, (_, sq) in enumerate(seqs) if len(sq) >= W_LEN]
    rep = recs[6]
    assert len(np.unique(rep["hash"])) < len(rep)  # two identical records: two OPEN / CLOSE pairs
    mm = [(int(x["hash"]), int(x["wpos"]), int(x["wpos_end"]), int(x["seqId"]), int(x["strand"])) for r in recs for x in r]
    assert summ.index_windows == len(mm)
    lookup, index, _ = MI.build_index(mm)
    (sub,) = IF.parse(idx)
    kept = sub["minmers"]
    assert [(int(x["hash"]), int(x["wpos"]), int(x["wpos_end"]), int(x["seqId"]), int(x["strand"])) for x in kept] == index
    assert sorted(sub["keys"]) == sorted(lookup)
    for key, lst in zip(sub["keys"], sub["lists"]):
        assert [(int(p["pos"]), int(p["hash"]), int(p["seqId"]), int(p["side"])) for p in lst] == [tuple(p) for p in lookup[key]]
    dup = int(rep["hash"][np.nonzero(np.diff(np.sort(rep["hash"])) == 0)[0][0]])
    assert len(lookup[dup]) >= 4


def test_cli_streaming_paf(gpu, tmp_path):
    """-m --streaming-minhash writes the PAF of the stage oracles over the restated target records, and so does -W then -I"""
    seqs = _streaming_pangenome()
    fa = str(tmp_path / "pan.fa")
    _write_fasta(fa, seqs)
    pct = 0.85
    args = ["-m", "-p", "85", "-S", "0"]  # (-S 0: chains of a few windows are enough, no scaffold filter)
    P = capi.map_default_params(percentage_identity=pct, auto_pct_identity=0, scaffold_min_length=0)
    S = MP.sketch_size(pct, W_LEN, 15)
    maps, _, _ = MP.map_queries(seqs, pct, add_minmers=_restated(seqs, S))
    exp = "".join(pyfilter.ref_filter("subset", maps[q], fa, seqs[q][0], P) for q in range(len(seqs)))
    assert len(exp.splitlines()) > 20
    out, direct = str(tmp_path / "s.paf"), str(tmp_path / "d.paf")
    subprocess.check_call([CLI] + args + ["--streaming-minhash", "--out", out, fa], cwd=str(tmp_path), timeout=300)
    assert open(out).read() == exp
    subprocess.check_call([CLI] + args + ["--out", direct, fa], cwd=str(tmp_path), timeout=300)
    assert open(direct).read() != exp  # the flag changes the index
    idx, from_file = str(tmp_path / "s.idx"), str(tmp_path / "f.paf")
    subprocess.check_call([CLI, "-W", idx, "--streaming-minhash", "-p", "85", fa], cwd=str(tmp_path), timeout=300)
    subprocess.check_call([CLI] + args + ["-I", idx, "--streaming-minhash", "--out", from_file, fa], cwd=str(tmp_path), timeout=300)
    assert open(from_file).read() == exp


def test_hg_filter(gpu, tmp_path):
    seqs = _pangenome(41)
    fa = str(tmp_path / "pan.fa")
    _write_fasta(fa, seqs)

    def run(tag, *extra):
        out = str(tmp_path / f"{tag}.paf")
        subprocess.check_call([CLI, "-m", "-p", "85", "--out", out, *extra, fa], cwd=str(tmp_path), timeout=300)
        return open(out).read()

    default = run("default")
    assert len(default.splitlines()) > 10
    assert run("explicit_default", "--hg-filter", "1.0,0.0,99.9") == default
    hg = run("hg", "--hg-filter", "2,1,95")
    api = str(tmp_path / "api.paf")
    capi.map_paf(gpu, fa, api, params=capi.map_default_params(percentage_identity=0.85, auto_pct_identity=0, hg_numerator=2,
                                                               ani_diff=0.01, ani_diff_conf=0.95))
    assert hg == open(api).read()
    assert hg != default


def test_tmp_base_and_keep_temp(gpu, tmp_path):
    seqs = _pangenome(47, L=24000)
    fa = str(tmp_path / "pan.fa")
    _write_fasta(fa, seqs)
    base = [CLI, "-p", "85", "-t", "4"]
    m, one = str(tmp_path / "m.paf"), str(tmp_path / "one.paf")
    subprocess.check_call(base + ["-m", "--out", m, fa], cwd=str(tmp_path), timeout=300)
    subprocess.check_call(base + ["--out", one, fa], cwd=str(tmp_path), timeout=300)
    work, keep, gone = tmp_path / "work", tmp_path / "keep", tmp_path / "gone"
    for d in (work, keep, gone):
        d.mkdir()
    two = str(tmp_path / "two.paf")
    r = subprocess.run(base + ["-B", str(keep), "-Z", "--out", two, fa], cwd=str(work), timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kept = os.listdir(keep)
    assert len(kept) == 1 and kept[0].startswith("wfmash-") and os.listdir(work) == []
    assert str(keep / kept[0]) in r.stderr
    assert open(keep / kept[0]).read() == open(m).read()
    assert open(two).read() == open(one).read()
    three = str(tmp_path / "three.paf")
    subprocess.check_call(base + ["-B", str(gone), "--out", three, fa], cwd=str(work), timeout=300)
    assert os.listdir(gone) == [] and os.listdir(work) == []
    assert open(three).read() == open(one).read()
