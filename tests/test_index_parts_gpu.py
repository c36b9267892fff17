"""The target index built from parts: wfm_sketch_part leaves the records of some sequences on the device that made them,
wfm_index_build_parts runs the index stage on the union of such parts in a given order (a segmented gather lays the
sequences' records end to end), and wfmh_map_multi deals every target subset over its handles that way.  Several handles on
device 0 stand in for several GPUs.

Run as a program (`python tests/test_index_parts_gpu.py MODE OUT ...`) this file is the child process of the tests that need
an environment switch set before the library reads it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from wfmash_amd import capi, synth  # noqa: E402

pytestmark = pytest.mark.gpu

K, W, S, THREADS = 15, 256, 12, 4
# 255: under w (the driver skips it); 20 000 Ns: no record, in the middle of the order; 300 000: many gather tiles
LENGTHS = [255, 256, 3017, 40_000, 20_000, 300_000, 5_000, 120_000]
N_RUN = 4  # index of the run of Ns
INFO_FIELDS = ("n_windows", "n_kept", "n_unique", "n_points", "threshold", "filtered", "adjusted")


def _sequences():
    return [b"N" * n if i == N_RUN else synth.random_dna(0x1D00 + i, n) for i, n in enumerate(LENGTHS)]


def _deal(name):
    """-> (sequence indices of every part, order): order[i] = (part, place in the part) of sequence i."""
    n = len(LENGTHS)
    if name == "one":
        members = [list(range(n))]
    elif name == "round_robin":
        members = [[i for i in range(n) if i % 3 == p] for p in range(3)]
    else:
        # four parts, the third empty; sequence i goes to part (0, 1, 3)[i % 3], so that neighbours in the order never share a
        # part, and a part holds its sequences in descending order, so that no part is in order
        assert name == "interleaved"
        members = [[i for i in reversed(range(n)) if (0, 1, 3)[i % 3] == p] for p in range(4)]
    where = {i: (p, j) for p, m in enumerate(members) for j, i in enumerate(m)}
    order = [where[i] for i in range(n)]
    if name != "one":
        assert all(order[i][0] != order[i + 1][0] for i in range(n - 1))
    return members, order


def _index_arrays(ix):
    inf = ix.info()
    uh, po, pts, mm = ix.download()
    return {"info": np.array([int(getattr(inf, f)) for f in INFO_FIELDS], dtype=np.int64), "uhash": uh, "poff": po,
            "points": pts.view(np.uint8), "minmers": mm.view(np.uint8)}


def _build_from_parts(handles, deal_name, seqs):
    """sketches the parts of the deal on handles[p % len(handles)], builds on handles[0]; -> (index arrays, number of records)"""
    members, order = _deal(deal_name)
    parts = []
    try:
        for p, m in enumerate(members):
            parts.append(handles[p % len(handles)].sketch_part([seqs[i] for i in m], K, W, S, seq_ids=m, threads=THREADS))
        ix, n = handles[0].index_build_parts(parts, order)
        try:
            return _index_arrays(ix), n
        finally:
            ix.free()
    finally:
        for p in parts:
            p.free()


def _assert_same_index(got, want):
    assert dict(zip(INFO_FIELDS, got["info"].tolist())) == dict(zip(INFO_FIELDS, want["info"].tolist()))
    for name in ("uhash", "poff", "points", "minmers"):
        assert np.array_equal(got[name], want[name]), name


def _child(mode, out, env, *args):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, out, *args], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def whole(gpu):
    """the reference of every test below, computed once: the records per sequence and the index of the whole list"""
    seqs = _sequences()
    recs = gpu.add_minmers_multi(seqs, K, W, S, threads=THREADS)
    ix, n = gpu.index_build_sequences(seqs, K, W, S, threads=THREADS)
    try:
        arrays = _index_arrays(ix)
    finally:
        ix.free()
    assert n == sum(len(r) for r in recs) and arrays["info"][0] == n
    return {"seqs": seqs, "recs": recs, "index": arrays, "n": n}


def test_the_sizes_reach_the_gather_kernels_cases(whole):
    """from the counts: the longest sequence spans more than three tiles, a sequence lies inside one tile, a row without records
    lies between two with records"""
    counts = np.array([len(r) for r in whole["recs"]], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(counts)])
    tile = capi.GATHER_TILE
    assert counts[0] == 0 and counts[N_RUN] == 0  # under w; nothing but N
    assert counts.max() > 3 * tile
    big = int(counts.argmax())
    assert (offs[big + 1] - 1) // tile - offs[big] // tile >= 3
    assert any(counts[i] > 0 and offs[i] // tile == (offs[i + 1] - 1) // tile and offs[i] % tile != 0 for i in range(len(counts)))
    assert counts[:N_RUN].sum() > 0 and counts[N_RUN + 1:].sum() > 0
    assert offs[-1] > tile and offs[-1] % tile != 0  # more than one workgroup, the last tile not full


def test_a_part_holds_the_records_of_add_minmers_multi(gpu, whole):
    some = [7, 0, N_RUN, 2, 5]
    part = gpu.sketch_part([whole["seqs"][i] for i in some], K, W, S, seq_ids=some, threads=THREADS)
    try:
        total, counts = part.info()
        assert counts.tolist() == [len(whole["recs"][i]) for i in some] and total == counts.sum()
        got = part.download()
        for g, i in zip(got, some):
            assert np.array_equal(g.view(np.uint8), whole["recs"][i].view(np.uint8)), i  # (sequence i has id i in both)
    finally:
        part.free()
    # a sequence shorter than k: no record, and a part of nothing is a part
    part = gpu.sketch_part([b"ACGTACGTAC", whole["seqs"][1]], K, W, S, threads=THREADS)
    try:
        total, counts = part.info()
        assert counts.tolist() == [0, len(whole["recs"][1])] and total == counts.sum()
    finally:
        part.free()
    empty = gpu.sketch_part([], K, W, S, threads=THREADS)
    try:
        assert empty.info()[0] == 0 and len(empty.info()[1]) == 0 and empty.download() == []
        ix, n = gpu.index_build_parts([empty], [])
        assert ix is None and n == 0
    finally:
        empty.free()


@pytest.mark.parametrize("deal", ["one", "round_robin", "interleaved"])
def test_parts_equal_the_whole(gpu, whole, deal):
    got, n = _build_from_parts([gpu], deal, whole["seqs"])
    assert n == whole["n"]
    _assert_same_index(got, whole["index"])


def test_a_sequence_is_named_once_and_exists(gpu, whole):
    part = gpu.sketch_part(whole["seqs"][1:3], K, W, S, threads=THREADS)
    try:
        for order in ([(0, 0), (0, 0)], [(0, 2)], [(1, 0)], [(0, -1)]):
            with pytest.raises(capi.WfmError):
                gpu.index_build_parts([part], order)
    finally:
        part.free()


def test_device_winnowed_records(whole, tmp_path):
    """WFM_WINNOW_DEV_MIN=100000 (child process): the records of the 300 000 and the 120 000 base sequence come from the
    device winnower and reach the part device to device"""
    out = str(tmp_path / "dev.npz")
    _, log = _child("parts", out, {"WFM_WINNOW_DEV_MIN": "100000", "WFM_DEBUG": "1"}, "round_robin")
    # (the two sequences are in two parts: each sketch call reports one sequence winnowed on the device, none handed back)
    assert log.count("winnowing on the device: 1 sequences") == 2 and log.count("; 0 handed back to the host") == 2, log[-2000:]
    _assert_same_index(np.load(out), whole["index"])


def test_parts_on_different_handles(gpu, whole):
    """Three parts sketched on three handles, the index built on the first; the second handle is gone by then.  All handles
    are on device 0: this covers who owns a part and how long it lives, NOT the copy between two devices (no test box has
    two) -- test_staged_parts runs that copy's code with source and destination on one device."""
    hs = [gpu, capi.Handle(0), capi.Handle(0)]
    members, order = _deal("round_robin")
    parts = []
    try:
        for h, m in zip(hs, members):
            parts.append(h.sketch_part([whole["seqs"][i] for i in m], K, W, S, seq_ids=m, threads=THREADS))
        hs[1].close()
        ix, n = gpu.index_build_parts(parts, order)
        try:
            assert n == whole["n"]
            _assert_same_index(_index_arrays(ix), whole["index"])
        finally:
            ix.free()
    finally:
        for p in parts:
            p.free()
        hs[2].close()


@pytest.mark.parametrize("deal", ["round_robin", "interleaved"])
def test_staged_parts(whole, tmp_path, deal):
    """WFM_INDEX_STAGE_ALL=1 (child process): every part goes through the pinned staging buffers as a part of another device
    would, in chunks of 4096 records -- the longest part is several chunks, the slots are used again.  Source and destination
    are the same device here."""
    out = str(tmp_path / "staged.npz")
    _child("parts", out, {"WFM_INDEX_STAGE_ALL": "1", "WFM_INDEX_STAGE_CHUNK": "4096"}, deal)
    _assert_same_index(np.load(out), whole["index"])


# ---------------------------------------------------------------- the driver ----

def _pangenome(path):
    """six sequences of 60 - 200 kb in two PanSN groups, all cut from one backbone"""
    base = synth.random_dna(0x9A17, 200_000)
    lens = [200_000, 150_000, 100_000, 80_000, 120_000, 60_000]
    names = ["A#1#c1", "A#1#c2", "A#1#c3", "B#1#c1", "B#1#c2", "B#1#c3"]
    recs = [(nm, synth.mutate(base[:n], 0.02, 0x9A00 + i)) for i, (nm, n) in enumerate(zip(names, lens))]
    synth.write_fasta(path, recs)
    return [len(s) for _, s in recs]


SUBSET_BASES = 500_000  # two subsets: four sequences, then two (fewer than the three handles)


def _map_params(**over):
    return capi.map_default_params(threads=8, index_by_size=SUBSET_BASES, **over)


@pytest.fixture(scope="module")
def pangenome(gpu, tmp_path_factory):
    d = tmp_path_factory.mktemp("index_parts")
    fa = str(d / "pan.fa")
    lens = _pangenome(fa)
    assert sum(lens[:3]) < SUBSET_BASES <= sum(lens[:4]) and sum(lens[4:]) < SUBSET_BASES
    paf = str(d / "one.paf")
    s1 = capi.map_paf(gpu, fa, paf, params=_map_params())
    assert s1.subsets == 2 and s1.written > 0 and s1.index_parts == 1
    assert s1.ms_index_sketch == 0 and s1.ms_index_merge == 0
    return {"dir": d, "fa": fa, "paf": open(paf, "rb").read(), "summary": s1}


def test_driver_three_handles_give_the_bytes_of_one(gpu, pangenome):
    hs = [gpu, capi.Handle(0), capi.Handle(0)]
    try:
        out = str(pangenome["dir"] / "three.paf")
        s3 = capi.map_paf_multi(hs, pangenome["fa"], out, params=_map_params())
        assert open(out, "rb").read() == pangenome["paf"]
        assert s3.index_parts == 3
        assert s3.index_windows == pangenome["summary"].index_windows and s3.written == pangenome["summary"].written
        assert 0 < s3.ms_index_sketch <= s3.ms_index and 0 < s3.ms_index_merge <= s3.ms_index
        # -W: the index files
        i1, i3 = str(pangenome["dir"] / "one.idx"), str(pangenome["dir"] / "three.idx")
        w1 = capi.map_paf(gpu, pangenome["fa"], str(pangenome["dir"] / "none1.paf"), params=_map_params(index_file=i1, write_index=1))
        w3 = capi.map_paf_multi(hs, pangenome["fa"], str(pangenome["dir"] / "none3.paf"), params=_map_params(index_file=i3, write_index=1))
        assert os.path.getsize(i1) > 0 and open(i1, "rb").read() == open(i3, "rb").read()
        assert w1.index_parts == 1 and w3.index_parts == 3
        # -I: nothing is sketched
        r3 = capi.map_paf_multi(hs, pangenome["fa"], out, params=_map_params(index_file=i3, write_index=0))
        assert r3.index_parts == 0 and open(out, "rb").read() == pangenome["paf"]
        # --streaming-minhash: the records are made on the host, handles[0] builds alone
        m1, m3 = str(pangenome["dir"] / "mh1.paf"), str(pangenome["dir"] / "mh3.paf")
        capi.map_paf(gpu, pangenome["fa"], m1, params=_map_params(streaming_minhash=1))
        sm = capi.map_paf_multi(hs, pangenome["fa"], m3, params=_map_params(streaming_minhash=1))
        assert sm.index_parts == 1 and open(m1, "rb").read() == open(m3, "rb").read()
    finally:
        for h in hs[1:]:
            h.close()


def test_driver_switch_forces_the_single_handle_build(pangenome):
    """WFM_INDEX_SHARDED=0 (child process): three handles, the index built on the first alone"""
    out = str(pangenome["dir"] / "unsharded.paf")
    got = json.loads(_child("driver", out, {"WFM_INDEX_SHARDED": "0"}, pangenome["fa"])[0].strip().splitlines()[-1])
    assert got["index_parts"] == 1 and got["ms_index_sketch"] == 0
    assert open(out, "rb").read() == pangenome["paf"]


def _main(argv):
    mode, out = argv[0], argv[1]
    if mode == "parts":
        h = capi.Handle(0)
        got, _ = _build_from_parts([h], argv[2], _sequences())
        np.savez(out, **got)
        h.close()
    elif mode == "driver":
        hs = [capi.Handle(0) for _ in range(3)]
        s = capi.map_paf_multi(hs, argv[2], out, params=_map_params())
        print(json.dumps({"index_parts": s.index_parts, "ms_index_sketch": s.ms_index_sketch}))
        for h in hs:
            h.close()
    else:
        raise SystemExit("unknown mode " + mode)


if __name__ == "__main__":
    _main(sys.argv[1:])
