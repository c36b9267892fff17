"""The semantics of --chain (include/wfmash_hip.h: wfm_chain_runs; include/wfmash_host.h: wfmh_set_chain) restated in plain Python by
brute force: the yardstick of tests/test_chain_cpu.py and tests/test_chain_gpu.py.

The pattern is the target, the text the query as aligned.  A run list is expanded to one (p, t, op) per column (lift_model.columns) and
the blocks are read off the columns one by one.  Nothing here takes a prefix or searches one: the model shares no logic with the kernels.

A block is a maximal stretch of = and X columns; the gap behind it is (the D columns, the I columns) up to the next block.  The columns
before the first block are the lead, those behind the last one the trail."""
import re

from tests import lift_model as lm

SWAP, REVERSE = 1, 2
CHAIN_SPANS = 2


def plain(runs):
    """(blocks [[size, eq]], gaps [(dt, dq)] one fewer, lead (dt, dq), trail (dt, dq), eq, x) of a run list, column by column"""
    cols, _, _ = lm.columns(runs)
    blocks, gaps, pend, prev = [], [], [0, 0], None
    for _, _, op in cols:
        if op in "=X":
            if prev is None or prev not in "=X":
                gaps.append(tuple(pend))
                pend = [0, 0]
                blocks.append([0, 0])
            blocks[-1][0] += 1
            blocks[-1][1] += op == "="
        else:
            pend[0 if op == "D" else 1] += 1
        prev = op
    if not blocks:
        return [], [], tuple(pend), (0, 0), 0, 0
    eq = sum(b[1] for b in blocks)
    return blocks, gaps[1:], gaps[0], tuple(pend), eq, sum(b[0] for b in blocks) - eq


def flagged(shape, flags):
    """the plain shape of a problem under WFM_CHAIN_REVERSE and WFM_CHAIN_SWAP"""
    blocks, gaps, lead, trail, eq, x = shape
    if flags & REVERSE:
        blocks, gaps, lead, trail = blocks[::-1], gaps[::-1], trail, lead
    if flags & SWAP:
        gaps, lead, trail = [(q, t) for t, q in gaps], lead[::-1], trail[::-1]
    return blocks, gaps, lead, trail, eq, x


def refused(runs):
    """what the device refuses before it writes anything: no runs, an empty run, a pattern or text span beyond 32 bits"""
    return (not runs or any(n == 0 for n, _ in runs) or sum(n for n, op in runs if op != "I") > 0xffffffff
            or sum(n for n, op in runs if op != "D") > 0xffffffff)


def chain_problems(problems):
    """what wfm_chain_runs returns: ([(size, dt, dq, eq)], [(flags, n_runs, first, count, lead_dt, lead_dq, trail_dt, trail_dq, eq, x)]).
    problems = [([(length, op)], flags)]"""
    out, per = [], []
    for runs, flags in problems:
        if refused(runs):
            per.append((CHAIN_SPANS, len(runs), len(out), 0, 0, 0, 0, 0, 0, 0))
            continue
        blocks, gaps, lead, trail, eq, x = flagged(plain(runs), flags)
        per.append((0, len(runs), len(out), len(blocks)) + tuple(lead) + tuple(trail) + (eq, x))
        for k, (size, beq) in enumerate(blocks):
            dt, dq = gaps[k] if k + 1 < len(blocks) else (0, 0)
            out.append((size, dt, dq, beq))
    return out, per


def chain_text(records, swap=False):
    """the chain file's bytes.  A record is a dict with qname, qsize, qs, qe, strand, tname, tsize, ts, te as its PAF line has them (forward
    coordinates, half-open) and runs, the line's cg:Z: ([(length, op)]).  Ids count from 1 in the order given; a record without an aligned
    column has no chain."""
    out, cid = [], 0
    for r in records:
        blocks, gaps, lead, trail, eq, _ = plain(r["runs"])
        if not blocks:
            continue
        cid += 1
        rev = r["strand"] == "-"
        # the two sides as the plain chain has them: the target forward, the query on its strand
        ts, te = r["ts"] + lead[0], r["te"] - trail[0]
        qs, qe = (r["qsize"] - r["qe"], r["qsize"] - r["qs"]) if rev else (r["qs"], r["qe"])
        qs, qe = qs + lead[1], qe - trail[1]
        a = (r["tname"], r["tsize"], "+", ts, te)
        b = (r["qname"], r["qsize"], r["strand"], qs, qe)
        if swap:  # chainSwap: the sides change places; the first side must stay +, so a - chain is read from its other end
            a, b, gaps = b, a, [(q, t) for t, q in gaps]
            if rev:
                a = (a[0], a[1], "+", a[1] - a[4], a[1] - a[3])
                b = (b[0], b[1], "-", b[1] - b[4], b[1] - b[3])
                blocks, gaps = blocks[::-1], gaps[::-1]
        out.append("chain %d %s %d %s %d %d %s %d %s %d %d %d\n" % ((eq,) + a + b + (cid,)))
        for k, (size, _) in enumerate(blocks):
            out.append("%d\t%d\t%d\n" % ((size,) + gaps[k]) if k + 1 < len(blocks) else "%d\n" % size)
        out.append("\n")
    return "".join(out).encode()


def parse_chains(text):
    """[(header fields as a dict, [(size, dt, dq)])] of a chain file; the last block of a chain has dt = dq = 0"""
    if isinstance(text, bytes):
        text = text.decode()
    chains = []
    for para in text.split("\n\n"):
        lines = [ln for ln in para.split("\n") if ln]
        if not lines:
            continue
        f = lines[0].split(" ")
        assert f[0] == "chain" and len(f) == 13, lines[0]
        head = dict(score=int(f[1]), tname=f[2], tsize=int(f[3]), tstrand=f[4], tstart=int(f[5]), tend=int(f[6]), qname=f[7], qsize=int(f[8]),
                    qstrand=f[9], qstart=int(f[10]), qend=int(f[11]), id=int(f[12]))
        blocks = []
        for ln in lines[1:]:
            v = [int(s) for s in ln.split("\t")]
            assert len(v) in (1, 3), ln
            blocks.append(tuple(v) if len(v) == 3 else (v[0], 0, 0))
        assert all(re.fullmatch(r"\d+\t\d+\t\d+", ln) for ln in lines[1:-1]) and re.fullmatch(r"\d+", lines[-1]), para
        chains.append((head, blocks))
    return chains


def lift_pos(text, name, pos):
    """liftOver of one forward position of the chain file's first side: [(qname, qstrand, forward position on the second side)], one per
    chain whose block holds it"""
    hits = []
    for head, blocks in parse_chains(text):
        if head["tname"] != name:
            continue
        t, q = head["tstart"], head["qstart"]
        for size, dt, dq in blocks:
            if t <= pos < t + size:
                at = q + (pos - t)
                hits.append((head["qname"], head["qstrand"], head["qsize"] - 1 - at if head["qstrand"] == "-" else at))
            t, q = t + size + dt, q + size + dq
    return hits
