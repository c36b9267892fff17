"""What the map driver decides without a device (wfmash_amd/host/map_plan.hpp through wfmh_test_map_plan; no GPU): the targets'
subsets, a query's fragments, which queries share a batch, the room for a batch's mappings, the split of a batch's mappings by
query and the fill of a query's vector from the device's permutation.  Every expected value is worked out here, in Python."""
import numpy as np
import pytest

from wfmash_amd import capi

W = 1000
BATCH_BASES = 256 << 20
COPY_BASES = 64 << 20


def layout(length, w=W, base=0, first_frag=0):
    out = capi.host_map_plan(0, [length, w, base, first_frag], 2 + length // w)
    return int(out[0]), [int(x) for x in out[1:1 + int(out[0])]]


def subsets(batch, lengths):
    out = capi.host_map_plan(1, [batch] + list(lengths), 1 + len(lengths))
    return [int(x) for x in out[1:1 + int(out[0])]]


def plan(batch_bases, qi, lengths):
    out = capi.host_map_plan(2, [batch_bases, qi] + list(lengths), 4 + len(lengths))
    nxt, in_place, n_bases, nm = (int(x) for x in out[:4])
    return nxt, bool(in_place), n_bases, [int(x) for x in out[4:4 + nm]]


def sizes(n_handles, query_bp, nfrag, subset_size):
    return [int(x) for x in capi.host_map_plan(3, [n_handles, query_bp, nfrag, subset_size], 7)]


def split(spans, mfrag):
    return [int(x) for x in capi.host_map_plan(4, [len(spans)] + [v for s in spans for v in s] + list(mfrag), len(spans) + 1)]


def results(first_frag, w, m0, nq, mfrag, perm, qstart, threads=1):
    """-> (the mapping each result was, its queryStartPos, orig)"""
    n = len(mfrag)
    values = [first_frag, w, m0, nq, threads, perm is not None, n] + list(mfrag) + list(perm if perm is not None else [0] * n) + list(qstart)
    out = capi.host_map_plan(5, values, 1 + 3 * nq)
    no = int(out[0])
    return [int(x) for x in out[1:1 + nq]], [int(x) for x in out[1 + nq:1 + 2 * nq]], [int(x) for x in out[1 + 2 * nq:1 + 2 * nq + no]]


def expected_layout(length, w, base):
    whole = length // w
    offs = [base + i * w for i in range(whole)]
    if whole >= 1 and length % w:
        offs.append(base + length - w)
    return offs


@pytest.mark.parametrize("length", [0, W - 1, W, W + 1, 2 * W, 2 * W + 1, 3 * W - 1])
def test_layout_fragments_edges(length):
    n, offs = layout(length)
    exp = {0: [], W - 1: [], W: [0], W + 1: [0, 1], 2 * W: [0, W], 2 * W + 1: [0, W, W + 1], 3 * W - 1: [0, W, 2 * W - 1]}[length]
    assert (n, offs) == (len(exp), exp)
    if length >= W and length % W:
        assert offs[-1] == length - W  # anchored at the end
    # inside a batch: the offsets move with the sequence's place, the count does not
    assert layout(length, W, 12345, 7) == (len(exp), [12345 + o for o in exp])


def test_target_subsets():
    assert subsets(100, []) == []
    assert subsets(100, [250]) == [1]                       # a sequence alone reaches the batch
    assert subsets(100, [250, 10, 20]) == [1, 2]            # ... and the last subset is short
    assert subsets(100, [40, 60, 99, 1, 30]) == [2, 2, 1]   # exactly the batch closes a subset (>=)
    assert subsets(100, [40, 59, 1, 5]) == [3, 1]
    assert subsets(5_000_000, [3_000_000_000, 1]) == [1, 1]  # sums beyond 2^31


def test_plan_batch_cases():
    # one sequence longer than batch_bases: alone and in place
    assert plan(1000, 0, [5000, 10, 10]) == (1, True, 5000, [0])
    # several short ones reach it: copied
    assert plan(1000, 0, [400, 400, 400, 400]) == (3, False, 1200, [0, 1, 2])
    # the second would pass kCopyBases: it begins its own batch, whatever batch_bases allows
    big = COPY_BASES - 10
    assert plan(BATCH_BASES, 0, [big, 11, 5]) == (1, True, big, [0])
    assert plan(BATCH_BASES, 0, [big, 10, 5]) == (2, False, COPY_BASES, [0, 1])  # exactly kCopyBases is still copied
    assert plan(BATCH_BASES, 1, [big, 11, 5]) == (3, False, 16, [1, 2])
    # empties and missing ones between real ones are consumed, never members
    assert plan(1000, 0, [0, 300, 0, -1, 300, 0, 500, 0, 7]) == (7, False, 1100, [1, 4, 6])
    assert plan(1000, 7, [0, 300, 0, -1, 300, 0, 500, 0, 7]) == (9, True, 7, [8])
    # nothing left but empties: no batch, everything consumed
    assert plan(1000, 0, [0, 0]) == (2, False, 0, [])
    assert plan(1000, 2, [5, 5]) == (2, False, 0, [])


def expected_plan(batch_bases, qi, lengths):
    members, n_bases = [], 0
    while qi < len(lengths) and (n_bases < batch_bases or not members):
        if lengths[qi] <= 0:
            qi += 1
            continue
        if members and n_bases + lengths[qi] > COPY_BASES:
            break
        members.append(qi)
        n_bases += lengths[qi]
        qi += 1
    return qi, len(members) == 1, n_bases, members


def test_sizes():
    bb, cap, hint, k_batch, k_copy, k_early, k_spare = sizes(1, 10**12, 1000, 3)
    assert (k_batch, k_copy, k_early, k_spare) == (BATCH_BASES, COPY_BASES, 1 << 16, 1 << 17)
    assert bb == BATCH_BASES                                   # one handle: the constant, whatever the queries hold
    assert sizes(1, 5, 1, 1)[0] == BATCH_BASES
    assert sizes(2, 3, 1, 1)[0] == 1                           # two handles, tiny input: the floor
    assert sizes(2, 4000, 1, 1)[0] == 1000                     # query_bp / (2 * handles)
    assert sizes(8, 10**12, 1, 1)[0] == BATCH_BASES            # never above the constant
    assert (cap, hint) == (1000 * 16 + 65536, 3000)            # at least 16 per fragment; one per target sequence
    assert sizes(1, 0, 1000, 40)[1:3] == [1000 * 80 + 65536, 16000]
    assert sizes(1, 0, 1000, 500)[1:3] == [1000 * 256 + 65536, 16000]
    assert sizes(1, 0, 0, 0)[1:3] == [65536, 0]


def test_split_by_query():
    # three queries of 3, 2 and 4 fragments; the middle one has no mappings
    assert split([(0, 3), (3, 2), (5, 4)], [0, 0, 2, 5, 5, 8]) == [0, 3, 3, 6]
    assert split([(0, 3), (3, 2), (5, 4)], []) == [0, 0, 0, 0]
    assert split([(0, 3), (3, 2), (5, 4)], [4]) == [0, 0, 1, 1]
    assert split([(0, 0), (0, 2)], [0, 1]) == [0, 0, 2]       # a query shorter than the window has no fragments
    assert split([], []) == [0]


def test_query_results_orders():
    rng = np.random.default_rng(5)
    first_frag, m0, nq, n = 10, 4, 9, 16
    mfrag = sorted(int(x) for x in rng.integers(10, 14, n))
    qstart = [int(x) for x in rng.integers(0, 50, n)]
    exp_q = lambda ms: [qstart[m] + (mfrag[m] - first_frag) * W for m in ms]
    frag_order = list(range(m0, m0 + nq))
    # no permutation: fragment order
    assert results(first_frag, W, m0, nq, mfrag, None, qstart) == (frag_order, exp_q(frag_order), [])
    # the identity
    ident = list(range(n))
    assert results(first_frag, W, m0, nq, mfrag, ident, qstart) == (frag_order, exp_q(frag_order), list(range(nq)))
    # a real permutation: every query's range permuted within itself
    perm = np.arange(n)
    for lo, hi in ((0, m0), (m0, m0 + nq), (m0 + nq, n)):
        perm[lo:hi] = rng.permutation(np.arange(lo, hi))
    assert perm[0] != 0xFFFFFFFF and not np.array_equal(perm[m0:m0 + nq], frag_order)
    taken = [int(x) for x in perm[m0:m0 + nq]]
    assert results(first_frag, W, m0, nq, mfrag, perm.tolist(), qstart) == (taken, exp_q(taken), [int(x) for x in perm[m0:m0 + nq] - m0])
    assert results(first_frag, W, m0, nq, mfrag, perm.tolist(), qstart, threads=4) == (taken, exp_q(taken), [t - m0 for t in taken])
    # one entry points outside the query, before it or after it: fragment order, no orig
    for where, to in ((m0 + 2, m0 - 1), (m0 + nq - 1, m0 + nq), (m0, 0)):
        bad = perm.copy()
        bad[where] = to
        assert results(first_frag, W, m0, nq, mfrag, bad.tolist(), qstart) == (frag_order, exp_q(frag_order), [])
    # a single mapping takes no order; nor does a batch whose permutation begins with ~0
    assert results(first_frag, W, m0, 1, mfrag, perm.tolist(), qstart) == ([m0], exp_q([m0]), [])
    refused = perm.copy()
    refused[0] = 0xFFFFFFFF
    assert results(first_frag, W, m0, nq, mfrag, refused.tolist(), qstart) == (frag_order, exp_q(frag_order), [])
    assert results(first_frag, W, m0, 0, mfrag, perm.tolist(), qstart) == ([], [], [])


def test_query_results_long_query_on_several_threads():
    """at 2^17 mappings the fill is split over the threads it is given: the same vector whatever the split"""
    n = (1 << 17) + 3
    rng = np.random.default_rng(9)
    mfrag = np.sort(rng.integers(0, 5000, n))
    qstart = rng.integers(0, 900, n)
    perm = rng.permutation(n)
    exp = (perm.tolist(), (qstart[perm] + mfrag[perm] * W).tolist(), perm.tolist())
    for threads in (1, 3, 32):
        assert results(0, W, 0, n, mfrag.tolist(), perm.tolist(), qstart.tolist(), threads) == exp


def test_random_length_lists():
    """over a few thousand random lists: fragments cover [0, len) and none passes the end; batches partition the queries, in order"""
    rng = np.random.default_rng(2026)
    for it in range(3000):
        w = int(rng.choice([16, 100, 1000]))
        n = int(rng.integers(0, 12))
        lengths = [int(x) for x in np.where(rng.random(n) < 0.2, 0, rng.integers(1, 12 * w, n))]
        if it % 50 == 0 and n:
            lengths[int(rng.integers(0, n))] = COPY_BASES - int(rng.integers(0, 3 * w))
        batch_bases = int(rng.choice([1, 3 * w, 20 * w, BATCH_BASES]))
        qi, seen = 0, []
        while True:
            got = plan(batch_bases, qi, lengths)
            assert got == expected_plan(batch_bases, qi, lengths)
            nxt, in_place, n_bases, members = got
            if not members:
                assert nxt == len(lengths)
                break
            assert nxt > qi and n_bases == sum(lengths[m] for m in members) and in_place == (len(members) == 1)
            assert len(members) == 1 or n_bases <= COPY_BASES
            seen += members
            qi = nxt
        assert seen == [i for i, l in enumerate(lengths) if l > 0]  # each real query once, in order
        for length in lengths[:3]:
            if length >= COPY_BASES - 3000:
                continue
            nf, offs = layout(length, w, 0, 0)
            assert offs == expected_layout(length, w, 0) and nf == len(offs)
            assert all(0 <= o and o + w <= length for o in offs)
            covered = np.zeros(length, dtype=bool)
            for o in offs:
                covered[o:o + w] = True
            assert covered.all() if length >= w else nf == 0
