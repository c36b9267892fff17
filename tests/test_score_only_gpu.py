"""WFM_MODE_SCORE_ONLY and WFM_MODE_SCORE_LIMIT (include/wfmash_hip.h) against the CPU oracle: the score alone on every path that can
produce one, mixed with full alignments, the limit as a verdict on both sides of the boundary, and the work that is NOT done.
The oracle is oracle/pyoracle.py (align_* return the score; dp_score / dp_score_endsfree are the independent O(nm) check); the pairs are
synth.random_dna(1000 + n, n) against its mutation with seed 1001 + n, the smallest that reach each path."""
import os
import subprocess
import types

import pytest

from wfmash_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BI, EF, UNI = capi.WFM_MODE_END2END_BIWFA, capi.WFM_MODE_ENDSFREE, capi.WFM_MODE_END2END_UNI
SO, LIM = capi.WFM_MODE_SCORE_ONLY, capi.WFM_MODE_SCORE_LIMIT
MAX_SCORE = capi.WFM_ST_MAX_SCORE


def _pair(n, rate):
    t = synth.random_dna(1000 + n, n)
    return t, synth.mutate(t, rate, 1001 + n)


def _n_pair():
    p, t = _pair(3000, 0.05)
    return p[:1495] + b"N" * 10 + p[1505:], t


@pytest.fixture(scope="module")
def ref(oracle):
    """The pairs of this file by name, with the oracle's op string and score (computed once, never changed)."""
    pairs = {"60": _pair(60, 0.10), "100": _pair(100, 0.10), "101": _pair(101, 0.10), "700": _pair(700, 0.06), "2600": _pair(2600, 0.12),
             "6000": _pair(6000, 0.05), "20000": _pair(20000, 0.05), "N": _n_pair()}
    same = synth.random_dna(500, 500)
    pairs["same"] = (same, same)
    pairs["empty"] = (b"", same)
    pairs["unrelated"] = (synth.random_dna(1, 4000), synth.random_dna(2, 4000))
    r = types.SimpleNamespace(pairs=pairs, ops={}, score={})
    for name, (p, t) in pairs.items():
        rc, ops, sc, _ = oracle.align_biwfa(p, t)
        assert rc == 0
        r.ops[name], r.score[name] = ops, sc
        if max(len(p), len(t)) <= 6100:
            assert oracle.dp_score(p, t) == sc, name
    # the figures the issue names for these pairs
    assert (r.score["700"], r.score["2600"], r.score["6000"], r.score["20000"]) == (282, 1930, 1913, 6921)
    assert (r.score["same"], r.score["empty"], r.score["unrelated"]) == (0, 524, 8040)
    return r


ALL = ["60", "100", "101", "700", "2600", "6000", "20000", "N", "same", "empty", "unrelated"]


def _check_scores(res, names, ref):
    for name, r in zip(names, res):
        assert r.status == 0, (name, r.status)
        assert r.score == ref.score[name], (name, r.score, ref.score[name])
        assert r.ops == b"" and r.n_runs == 0, name


def test_scores_on_every_path(gpu, ref):
    """Every pair score-only through the four entry forms: base jobs at the fallback boundary (60, 100 | 101), the tile phase from one block
    (700) to seventy (20000), the byte kernels (N), a root that ends at score 0, an all-gap job, unrelated sequences."""
    items = [ref.pairs[n] + (BI | SO,) for n in ALL]
    _check_scores(gpu.align(items), ALL, ref)
    rle = gpu.align_rle(items)
    _check_scores([r for r, _ in rle], ALL, ref)
    assert all(ops_len == 0 for _, ops_len in rle)
    ss = gpu.upload(items)
    try:
        assert ss.arena_bytes == 0
        _check_scores(gpu.align_resident(ss), ALL, ref)
        assert all(ss.results[i].ops_len == 0 for i in range(ss.n))
    finally:
        ss.free()
    # by reference: the patterns as windows of one stored sequence (a spacer between them), the texts as host bytes
    store = gpu.seqstore()
    try:
        blob, offs = b"", []
        for n in ALL:
            blob += b"ACGT" * 3
            offs.append(len(blob))
            blob += ref.pairs[n][0]
        sid = store.add(blob + b"ACGT")
        refs = [dict(pattern_seq=sid, pattern_off=o, plen=len(ref.pairs[n][0]), text=ref.pairs[n][1], mode=BI | SO) for n, o in zip(ALL, offs)]
        _check_scores(gpu.align_refs(store, refs), ALL, ref)
    finally:
        store.free()
    assert gpu.scores([ref.pairs[n] for n in ALL]) == [(0, ref.score[n]) for n in ALL]


@pytest.mark.parametrize("pen", [(6, 10, 3, 124, 1), (19, 39, 3, 81, 1), (1, 0, 1, 0, 1), (4, 0, 2, 0, 2)], ids=lambda p: "-".join(map(str, p)))
def test_scores_for_other_penalties(gpu, oracle, pen):
    """128-row rings, the LDS tile kernel, edit distance and gap-linear penalties: score-only against the O(nm) DP."""
    pairs = [_pair(80, 0.10), _pair(700, 0.06), _pair(2600, 0.12)]
    got = gpu.scores(pairs, pen=pen)
    assert got == [(0, oracle.dp_score(p, t, pen=pen)) for p, t in pairs]


def test_scores_in_the_other_modes(gpu, oracle, ref):
    p, t = ref.pairs["700"]
    r = gpu.align([(p, t, UNI | SO)])[0]
    assert (r.status, r.score, r.ops, r.n_runs) == (0, 282, b"", 0)
    p = synth.random_dna(8300, 900)
    t = synth.random_dna(8301, 40) + synth.mutate(p, 0.1, 8302)
    free = (len(p), 0, len(t), 0)
    for pen in (None, (5, 8, 2, 60, 1)):
        want = oracle.align_endsfree(p, free[0], free[1], t, free[2], free[3], pen=pen)[2]
        assert want == oracle.dp_score_endsfree(p, t, *free, pen=pen)
        if pen is None:
            assert want == 567
        r = gpu.align([(p, t, EF | SO) + free], pen=pen)[0]
        assert (r.status, r.score, r.ops, r.n_runs) == (0, want, b"", 0), pen


def test_mixed_batch(gpu, ref):
    """Score-only and full problems side by side: the full ones give the oracle's op strings byte for byte, the others its scores, and the
    arena holds the full problems' strings alone."""
    names = ALL + ALL[::-1]
    items = [ref.pairs[n] + ((BI | SO) if i % 2 else BI,) for i, n in enumerate(names)]
    ss = gpu.upload(items)
    try:
        assert ss.arena_bytes == sum(len(p) + len(t) + 1 for i, (p, t, _) in enumerate(items) if i % 2 == 0)
        res = gpu.align_resident(ss)
        used = max(ss.results[i].ops_off + ss.results[i].ops_len for i in range(ss.n))
    finally:
        ss.free()
    for i, (n, r) in enumerate(zip(names, res)):
        assert r.status == 0 and r.score == ref.score[n], (i, n)
        assert r.ops == (b"" if i % 2 else ref.ops[n]), (i, n)
    assert sum(len(ref.ops[n]) for i, n in enumerate(names) if i % 2 == 0) <= used <= ss.arena_bytes  # (the parts of a batch begin at offsets of their own)
    rle = gpu.align_rle(items)
    for i, (n, (r, ops_len)) in enumerate(zip(names, rle)):
        assert r.status == 0 and r.score == ref.score[n], (i, n)
        if i % 2:
            assert r.ops == b"" and r.n_runs == 0 and ops_len == 0
        else:
            assert b"".join(op * ln for ln, op in r.ops) == ref.ops[n]


def test_the_work_really_stops(gpu, ref):
    """Eight 6000-base pairs, full and then score-only on the same handle: no base job, fewer breakpoint jobs, fewer cells."""
    p, t = ref.pairs["6000"]
    full = gpu.align([(p, t, BI)] * 8)
    a = gpu.stats()
    a = (a.cells, a.ms_kernels, a.bp_jobs, a.base_jobs, a.base_launches)
    only = gpu.align([(p, t, BI | SO)] * 8)
    b = gpu.stats()
    b = (b.cells, b.ms_kernels, b.bp_jobs, b.base_jobs, b.base_launches)
    print(f"eight 6000-base pairs: full cells {a[0]} ms_kernels {a[1]:.3f} bp_jobs {a[2]} base_jobs {a[3]}; "
          f"score-only cells {b[0]} ms_kernels {b[1]:.3f} bp_jobs {b[2]} base_jobs {b[3]}")
    assert all(r.status == 0 and r.ops == ref.ops["6000"] for r in full)
    assert all(r.status == 0 and r.score == 1913 and r.ops == b"" for r in only)
    assert b[4] == 0 and b[3] == 0
    assert b[2] < a[2] and b[0] < a[0]


LIMITED = ["60", "101", "700", "2600", "6000", "N"]


def _limit_items(ref, names, flags):
    items, want = [], []
    for n in names:
        s = ref.score[n]
        for lim in (s, s - 1, s + 1000):
            items.append(ref.pairs[n] + (BI | LIM | flags, 0, 0, 0, 0, lim))
            want.append((n, lim >= s))
    return items, want


def _check_limits(res, want, ref, flags):
    for (n, ok), r in zip(want, res):
        if ok:
            assert r.status == 0 and r.score == ref.score[n], (n, r.status, r.score)
            assert r.ops == (b"" if flags & SO else ref.ops[n]), n
        else:
            assert r.status == MAX_SCORE and r.score == -1 and r.ops is None and r.n_runs == 0, (n, r.status, r.score)


@pytest.mark.parametrize("flags", [0, SO], ids=["full", "score_only"])
def test_limit_on_both_sides_of_the_boundary(gpu, ref, flags):
    items, want = _limit_items(ref, LIMITED, flags)
    ss = gpu.upload(items)
    try:
        failed = gpu.align_resident(ss, collect=False)
        res = gpu._collect(ss)
        assert all(ss.results[i].ops_len == 0 for i, (_, ok) in enumerate(want) if not ok)
    finally:
        ss.free()
    _check_limits(res, want, ref, flags)
    assert failed == sum(not ok for _, ok in want)


@pytest.mark.parametrize("flags", [0, SO], ids=["full", "score_only"])
def test_limit_when_guessed_bands_fail(ref, monkeypatch, flags):
    """Eighteen divergent roots under a budget their full rings do not fit, with bands of 200 scores a direction: the bands run out long before
    the limits do, the roots run again without them (WFM_PF_ROOT_AGAIN) -- under the limit still -- and the verdicts are the same."""
    monkeypatch.setenv("WFM_MEM_BUDGET_MB", "64")
    monkeypatch.setenv("WFM_BAND_ROOT", "200")
    monkeypatch.setenv("WFM_OVERLAP", "0")
    h = capi.Handle(0)
    try:
        items, want = _limit_items(ref, ["2600", "6000"] * 3, flags)
        res = h.align(items)
        fl = h.problem_flags(len(items))
    finally:
        h.close()
    assert len(items) >= 16
    _check_limits(res, want, ref, flags)
    assert any(int(f) & capi.WFM_PF_ROOT_AGAIN for f in fl), list(fl)


@pytest.mark.parametrize("flags", [0, SO], ids=["full", "score_only"])
def test_limit_on_the_step_kernel_alone(gpu, ref, monkeypatch, flags):
    """Without the tile phase the step kernel itself stops at the limit (a switch read per call)."""
    monkeypatch.setenv("WFM_TILE", "0")
    items, want = _limit_items(ref, ["101", "700", "2600"], flags)
    _check_limits(gpu.align(items), want, ref, flags)


def test_the_limit_bounds_the_work(gpu, ref):
    """A limit far below the score: WFM_ST_MAX_SCORE after at most a quarter of the cells of the unlimited score-only run (with limit 300 no
    direction passes score 300 plus one block of 100, where the unlimited run takes each to half the score under a far wider cut)."""
    for name, lim in (("20000", 300), ("unrelated", 500)):
        p, t = ref.pairs[name]
        assert gpu.scores([(p, t)]) == [(0, ref.score[name])]
        free = gpu.stats().cells
        assert gpu.scores([(p, t)], limit=lim) == [(MAX_SCORE, -1)]
        held = gpu.stats().cells
        print(f"{name}: cells without a limit {free}, with limit {lim} {held}: ratio {held / free:.5f}")
        assert held * 4 <= free, (name, held, free)


def test_argument_errors(gpu, ref):
    p, t = ref.pairs["700"]
    for bad in ((p, t, 3), (p, t, 0x400), (p, t, EF | LIM, 0, 0, 0, 0, 100), (p, t, BI | LIM, 0, 0, 0, 0, 0)):
        with pytest.raises(capi.WfmError):
            gpu.align([(p, t), bad])
        with pytest.raises(capi.WfmError):
            gpu.upload([bad])
        with pytest.raises(capi.WfmError):
            gpu.align_refs(None, [dict(pattern=p, text=t, mode=bad[2], score_hint=bad[7] if len(bad) > 7 else 0)])
        r = gpu.align([(p, t)])[0]
        assert r.status == 0 and r.ops == ref.ops["700"]


def test_shim_scope_and_max_steps(tmp_path, oracle, ref):
    from test_score_only_cpu import build_shim_user
    exe = build_shim_user(tmp_path)
    p, t = ref.pairs["700"]
    out = subprocess.check_output([exe, p.decode(), t.decode()]).decode().split()
    # score and length with scope Score; the status under a limit of 281, and of 282; the edit distance
    assert out == ["-282", "0", "-100", "0", str(-oracle.dp_score(p, t, pen=(1, 0, 1, 0, 1)))], out
