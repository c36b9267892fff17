"""CPU tests of the device sequence store's boundary: the ctypes structures match the header, the new entry points are
exported, the align driver's sub-window translation (problems by reference) is right on both strands, and the command line
lists its switch.  No GPU here."""
import ctypes as C
import os
import random
import re
import subprocess

from wfmash_amd import capi, synth
from oracle import wflign_host as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes():
    assert C.sizeof(capi.ProblemRef) == 80
    # resident_sequences took the place of the padding word: the layout is what it was
    assert C.sizeof(capi.AlignParams) == 88
    assert capi.AlignParams.resident_sequences.offset == 84 and capi.AlignParams.threads.offset == 80
    # records_resident and lazy_fetches are appended: nothing before them moves
    assert capi.AlignSummary.ms_tags.offset == 120
    assert capi.AlignSummary.records_resident.offset == 128 and capi.AlignSummary.lazy_fetches.offset == 136
    assert C.sizeof(capi.AlignSummary) == 144


def test_default_is_off():
    L = capi._host()
    prm = capi.AlignParams()
    prm.resident_sequences = 7
    L.wfmh_align_default_params(C.byref(prm))
    assert prm.resident_sequences == 0


def test_new_entry_points_are_declared_and_exported():
    L = capi.load()
    text = open(os.path.join(ROOT, "include", "wfmash_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("wfm_seqstore_create", "wfm_seqstore_free", "wfm_seqstore_add", "wfm_seqstore_info",
                 "wfm_upload_sequence_refs", "wfm_align_refs_rle", "wfm_download_sequences"):
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    m = re.search(r"#define\s+WFM_SEQ_GATHER_CHUNK\s+(\d+)", text)
    assert m and int(m.group(1)) == capi.SEQ_GATHER_CHUNK
    assert "wfmh_test_subwindow" in capi.HOST_EXPORTS and hasattr(L, "wfmh_test_subwindow")


def test_subwindow_translation_on_both_strands():
    """[a, b) of the strand-adjusted window [ws, we) of a stored sequence is a forward window of that sequence: the same bases
    as slicing the window a Python string holds -- reverse-complemented for a '-' side."""
    rng = random.Random(5)
    seq = W.upper_valid_dna(synth.random_dna(77, 3000))
    for _ in range(300):
        ws = rng.randrange(0, 2900)
        we = rng.randrange(ws, 3001)
        n = we - ws
        a = rng.randrange(0, n + 1)
        b = rng.randrange(a, n + 1)
        for rev in (False, True):
            window = W.revcomp(seq[ws:we]) if rev else seq[ws:we]
            s, e = capi.host_subwindow(ws, we, rev, a, b)
            assert e - s == b - a and ws <= s and e <= we
            got = W.revcomp(seq[s:e]) if rev else seq[s:e]
            assert got == window[a:b], (ws, we, a, b, rev)
    # the form the issue states: [a, b) of the '-' window [qs, qe) is [qe - b, qe - a)
    assert capi.host_subwindow(100, 500, True, 30, 70) == (500 - 70, 500 - 30)
    assert capi.host_subwindow(100, 500, False, 30, 70) == (130, 170)
    # head and tail patches: the first / last bases of the window
    assert capi.host_subwindow(100, 500, True, 0, 128) == (372, 500)
    assert capi.host_subwindow(100, 500, True, 400 - 128, 400) == (100, 228)


def test_cli_help_lists_the_switch():
    cli = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")
    r = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--resident-seqs" in r.stderr + r.stdout
