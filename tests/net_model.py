"""The net across records (include/wfmash_hip.h, wfm_net_*) restated by brute force: one array cell per target base, painted record by
record from the worst to the best, then read off base by base.  No prefix, no search, no tree: nothing here is shared with wfa_net.hip.

A record is a dict {order, score, blocks: [(t, q, size), ...]}.  A run word is (length << 2) | op with op 0 '=', 1 'X', 2 'I', 3 'D'
(the pattern is the target: D advances the target alone, I the query alone)."""
OP_M, OP_X, OP_I, OP_D = 0, 1, 2, 3
SCORE_EQ = 0xffffffff


def run_words(spec):
    """[(op, length), ...] as run words"""
    return [(n << 2) | op for op, n in spec]


def blocks_of_runs(base, runs):
    """(the blocks [(t, q, size)] of the maximal stretches of =/X runs, the = columns); base: the global target position of the first run"""
    blocks, eq = [], 0
    t, q = base, 0
    open_at = None
    for w in runs:
        n, op = w >> 2, w & 3
        if op in (OP_M, OP_X):
            if open_at is None:
                open_at = (t, q)
            if op == OP_M:
                eq += n
            t += n
            q += n
        else:
            if open_at is not None:
                blocks.append((open_at[0], open_at[1], t - open_at[0]))
                open_at = None
            if op == OP_I:
                q += n
            else:
                t += n
    if open_at is not None:
        blocks.append((open_at[0], open_at[1], t - open_at[0]))
    return blocks, eq


def refused(base, runs, n_bases):
    """what wfm_net_add flags WFM_NET_SPANS: an empty run, no runs, a pattern or text span beyond 32 bits or outside [0, n_bases]"""
    if not runs or any((w >> 2) == 0 for w in runs):
        return True
    span = sum(w >> 2 for w in runs if (w & 3) != OP_I)
    tspan = sum(w >> 2 for w in runs if (w & 3) != OP_D)
    return base > n_bases or base + span > n_bases or span > 0xffffffff or tspan > 0xffffffff


def record(order, score, base, runs):
    """the record a problem {base, runs, score, order} adds"""
    blocks, eq = blocks_of_runs(base, runs)
    return {"order": order, "score": eq if score == SCORE_EQ else score, "blocks": blocks}


def net(records, lo=0, hi=None):
    """(pieces [(order, t, q, size)] sorted by (order, t), per [(order, score, first, count, bases_won, bases_aligned)] sorted by order).
    The cells are those of [lo, hi): every block must lie inside (hi: the largest block end)."""
    ends = [t + n for r in records for (t, _, n) in r["blocks"]]
    if hi is None:
        hi = max(ends) if ends else lo
    assert all(lo <= t and t + n <= hi for r in records for (t, _, n) in r["blocks"])
    owner = [None] * (hi - lo)
    # the worst record first: whoever paints last is the best record over the base
    for r in sorted(records, key=lambda r: (r["score"], -r["order"])):
        for k, (t, _, n) in enumerate(r["blocks"]):
            for b in range(t, t + n):
                owner[b - lo] = (r["order"], k)
    by_order = {r["order"]: r for r in records}
    assert len(by_order) == len(records), "orders are unique"
    pieces = []
    start = None
    for b in range(lo, hi + 1):
        cur = owner[b - lo] if b < hi else None
        if start is not None and cur != owner[start - lo]:
            order, k = owner[start - lo]
            bt, bq, _ = by_order[order]["blocks"][k]
            pieces.append((order, start, bq + (start - bt), b - start))
            start = None
        if start is None and cur is not None:
            start = b
    pieces.sort(key=lambda p: (p[0], p[1]))
    per = []
    for order in sorted(by_order):
        mine = [i for i, p in enumerate(pieces) if p[0] == order]
        first = mine[0] if mine else sum(1 for p in pieces if p[0] < order)
        per.append((order, by_order[order]["score"], first, len(mine), sum(pieces[i][3] for i in mine),
                    sum(n for (_, _, n) in by_order[order]["blocks"])))
    return pieces, per


def chain_text(records, n_bases=None):
    """the --chain-net file's bytes.  A record is a dict with qname, qsize, qs, qe, strand, tname, tsize, ts, te as its PAF line has them
    (forward coordinates, half-open), runs, the line's cg:Z: as [(length, op)] with op one of "=XID", and t_offset, where its target
    sequence begins in the concatenation.  The records compete with their = columns, in the order given: ids count from 1 in that
    order, and a record that won nothing (or was refused) has no chain."""
    recs, heads = [], {}
    for order, r in enumerate(records):
        words = [(n << 2) | "=XID".index(op) for n, op in r["runs"]]
        base = r["t_offset"] + r["ts"]
        if refused(base, words, n_bases if n_bases is not None else base + (1 << 40)):
            continue
        recs.append(record(order, SCORE_EQ, base, words))
        heads[order] = r
    pieces, per = net(recs, lo=min([t for r in recs for (t, _, _) in r["blocks"]], default=0))
    out, cid = [], 0
    for order, score, first, count, _, _ in per:
        if count == 0:
            continue
        cid += 1
        r = heads[order]
        mine = pieces[first:first + count]
        q0 = r["qsize"] - r["qe"] if r["strand"] == "-" else r["qs"]  # where the runs begin on the record's strand
        (_, t_first, q_first, _), (_, t_last, q_last, n_last) = mine[0], mine[-1]
        out.append("chain %d %s %d + %d %d %s %d %s %d %d %d\n" % (score, r["tname"], r["tsize"], t_first - r["t_offset"], t_last + n_last - r["t_offset"],
                                                                 r["qname"], r["qsize"], r["strand"], q0 + q_first, q0 + q_last + n_last, cid))
        for k, (_, t, q, n) in enumerate(mine):
            if k + 1 < len(mine):
                out.append("%d\t%d\t%d\n" % (n, mine[k + 1][1] - (t + n), mine[k + 1][2] - (q + n)))
            else:
                out.append("%d\n" % n)
        out.append("\n")
    return "".join(out).encode()
