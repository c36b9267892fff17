"""The record passes of one handle share one scratch block and one output block (wfmash_amd/csrc/wfa_passes.hip): every pass carves its own
layout out of them, and the blocks grow with the largest call.  Here the passes run interleaved on ONE handle over batches of different
sizes -- small, large, the small one again -- and every result must be what a fresh handle gives for that batch alone."""
import numpy as np
import pytest

from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu


def _batch(seed, n, length):
    items = []
    for i in range(n):
        t = synth.random_dna(seed + i, length + 7 * i)
        items.append((t, synth.mutate(t, 0.06, (seed << 8) + i, p_sub=0.6, p_ins=0.2)))
    return items


def _fields(recs):
    return [tuple(getattr(r, f[0]) for f in r._fields_ if f[0] != "pad_") for r in recs]


def _all_passes(h, items):
    """check, left-align, cs (both forms), variants and check_optimal of one batch on handle h, as plain values"""
    ss = h.upload(items)
    try:
        failed, runs = h.align_resident_rle(ss)
        assert failed == 0
        n = ss.n
        res = [(r.status, r.score, r.ops_off, r.ops_len, r.n_runs) for r in ss.results[:n]]
        flagged, checks = h.check_runs(ss, ss.results, runs)
        assert flagged == 0
        la_res, la_runs, la_stats = h.left_align(ss, ss.results, runs)
        short, short_per = h.cs_strings(ss, ss.results, runs, capi.WFM_CS_SHORT)
        long_, long_per = h.cs_strings(ss, la_res, la_runs, capi.WFM_CS_LONG)
        recs, alleles, calls = h.call_variants(ss, ss.results, runs)
        opt = h.check_optimal(ss, ss.results)
        assert all(s for s in short) and all(o.flags == 0 for o in opt)
        return (res, runs.tobytes(), _fields(checks), [(r.ops_off, r.n_runs) for r in la_res[:n]], la_runs.tobytes(), _fields(la_stats),
                short, _fields(short_per), long_, _fields(long_per), recs.tobytes(), alleles, _fields(calls), _fields(opt))
    finally:
        ss.free()


def test_interleaved_passes_on_one_handle(gpu):
    small, large = _batch(0x5a00, 3, 300), _batch(0x5b00, 40, 2000)
    want = {}
    for name, items in (("small", small), ("large", large)):
        h = capi.Handle(0)
        try:
            want[name] = _all_passes(h, items)
        finally:
            h.close()
    assert len(want["large"][4]) > len(want["small"][4]) > 0 and len(want["large"][10]) > 0  # runs were left-aligned, variants called
    for name, items in (("small", small), ("large", large), ("small", small)):
        got = _all_passes(gpu, items)
        for k, (g, w) in enumerate(zip(got, want[name])):
            assert g == w, (name, k)
