"""The left-alignment rule of wfm_left_align_runs (include/wfmash_hip.h) in plain Python, and what the tests hold it against.

Runs are (length, op) with op one of 'M', 'X', 'I', 'D' (a CIGAR's '=' reads as 'M'); P is the pattern (target), T the text (query,
strand-adjusted), both bytes.  Nothing here is shared with the library: left_align() is the sequential rule as the header states it,
movable() looks at a finished CIGAR gap by gap and knows nothing of left_align()'s loop."""
import random
import re

OPS = "MXID"


def parse(cigar):
    """'12=3D4X' or '12M3D4X' -> [(12, 'M'), (3, 'D'), (4, 'X')]"""
    return [(int(n), "M" if op == "=" else op) for n, op in re.findall(r"(\d+)([=MXID])", cigar)]


def spell(runs, match="="):
    return "".join(f"{n}{match if op == 'M' else op}" for n, op in runs)


def to_words(runs):
    """runs -> the library's 32-bit runs, (length << 2) | op"""
    return [(n << 2) | OPS.index(op) for n, op in runs]


def from_words(words):
    return [(int(w) >> 2, OPS[int(w) & 3]) for w in words]


def left_align(P, T, runs):
    """The rule, run by run, each interior gap reading the output built so far.  Returns (new runs, [d of every interior gap])."""
    out, shifts = [], []
    p = t = 0
    n = len(runs)
    for r, (L, op) in enumerate(runs):
        if op in "ID" and 0 < r < n - 1:
            S, g = (P, p) if op == "D" else (T, t)
            rot = 0
            while g - rot - 1 >= 0 and S[g - rot - 1] == S[g + L - rot - 1]:
                rot += 1
            room = 0
            if out and out[-1][1] == "M":
                room = out[-1][0]
                if len(out) == 1 or out[-2][1] == op:
                    room -= 1
            d = min(rot, room)
            shifts.append(d)
            if d:
                e = out[-1][0] - d
                if e:
                    out[-1] = (e, "M")
                else:
                    out.pop()
                out.append((L, op))
                out.append((d, "M"))  # joins the M run behind it below, or stays a run of its own
            else:
                out.append((L, op))
        elif op == "M" and out and out[-1][1] == "M":
            out[-1] = (out[-1][0] + L, "M")
        else:
            out.append((L, op))
        if op != "I":
            p += L
        if op != "D":
            t += L
    return out, shifts


def check(P, T, runs):
    """None if runs are a valid CIGAR of P x T (no empty run, no two neighbours with one op, M over equal bytes, X over different
    ones, spanning both exactly), else what is wrong."""
    p = t = 0
    for r, (L, op) in enumerate(runs):
        if L <= 0:
            return f"run {r}: length {L}"
        if r and runs[r - 1][1] == op:
            return f"run {r}: same op as the run before"
        if op in "MX":
            if p + L > len(P) or t + L > len(T):
                return f"run {r}: leaves the sequences"
            for k in range(L):
                if (P[p + k] == T[t + k]) != (op == "M"):
                    return f"run {r} ({op}): pattern {p + k}, text {t + k}"
        if op != "I":
            p += L
        if op != "D":
            t += L
    if p != len(P) or t != len(T):
        return f"spans {p} x {t}, sequences {len(P)} x {len(T)}"
    return None


def counts(runs):
    """(matches, mismatches, ins_runs, ins_bases, del_runs, del_bases, x_runs): wfm_check_t's counts and the number of X runs"""
    c = [0] * 7
    for L, op in runs:
        if op == "M":
            c[0] += L
        elif op == "X":
            c[1] += L
            c[6] += 1
        elif op == "I":
            c[2] += 1
            c[3] += L
        else:
            c[4] += 1
            c[5] += L
    return tuple(c)


def price(runs, pen):
    x, o1, e1, o2, e2 = pen
    s = 0
    for L, op in runs:
        if op == "X":
            s += x * L
        elif op in "ID":
            s += min(o1 + e1 * L, o2 + e2 * L)
    return s


def movable(P, T, runs):
    """Indices of the interior gaps of a finished CIGAR that could still go one base to the left: the base before the gap equals the
    gap's last base, the run before it is an M run, and taking one base from that run neither empties the CIGAR's first run nor lets
    the gap meet a gap of its own op."""
    starts, p, t = [], 0, 0
    for L, op in runs:
        starts.append((p, t))
        p += L if op != "I" else 0
        t += L if op != "D" else 0
    found = []
    for r in range(1, len(runs) - 1):
        L, op = runs[r]
        if op not in "ID":
            continue
        S, g = (P, starts[r][0]) if op == "D" else (T, starts[r][1])
        if g < 1 or S[g - 1] != S[g + L - 1]:
            continue  # the bases do not rotate
        before_len, before_op = runs[r - 1]
        if before_op != "M":
            continue  # behind an X run or another gap
        if before_len == 1 and (r - 1 == 0 or runs[r - 2][1] == op):
            continue  # would become the first run, or merge with a gap of its op
        found.append(r)
    return found


# ---- cases by construction: sequences from homopolymers, short tandem units and random stretches, a CIGAR planted with them ----
def repeat_rich(rng, n):
    """n bases: homopolymers, tandem repeats of units of 2 - 6 bases, random stretches"""
    out = bytearray()
    while len(out) < n:
        kind = rng.random()
        if kind < 0.3:
            out += bytes([rng.choice(b"ACGT")]) * rng.randint(2, 40)
        elif kind < 0.65:
            unit = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(2, 6)))
            out += unit * rng.randint(2, 15)
        else:
            out += bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 30)))
    return bytes(out[:n])


def mutated_pair(rng, n, rate):
    """(P, T, ops): P repeat-rich, T = P with substitutions and indels at `rate` per base, ops the op per base that says so"""
    P = repeat_rich(rng, n)
    T = bytearray()
    ops = []
    i = 0
    while i < len(P):
        u = rng.random()
        if u < rate / 3:
            T.append(rng.choice([c for c in b"ACGT" if c != P[i]]))
            ops.append("X")
            i += 1
        elif u < 2 * rate / 3:
            L = min(rng.choice([1, 1, 2, 3, 5, 8, 13]), len(P) - i)
            ops += ["D"] * L
            i += L
        elif u < rate:
            L = rng.choice([1, 1, 2, 3, 5, 8, 13])
            # an insertion that copies what precedes it (a repeat grows) or is random
            ins = bytes(T[-L:]) if len(T) >= L and rng.random() < 0.7 else bytes(rng.choice(b"ACGT") for _ in range(L))
            T += ins
            ops += ["I"] * len(ins)
        else:
            T.append(P[i])
            ops.append("M")
            i += 1
    return P, bytes(T), ops


def planted_case(rng, n, rate):
    """(P, T, runs): a mutated pair and the CIGAR that says so with every gap at its RIGHTMOST placement (what the aligners give):
    planted base by base, then every gap pushed right while its bases rotate."""
    P, T, ops = mutated_pair(rng, n, rate)
    return P, T, push_right(P, T, compress(ops))


def compress(ops):
    runs = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1] = (runs[-1][0] + 1, op)
        else:
            runs.append((1, op))
    return runs


def push_right(P, T, runs):
    """every interior gap moved right base by base while the base behind it equals its first base, an M run follows and an M run
    precedes -- the placement an aligner that extends matches first ends up with.  Gaps of one op are kept apart by one M base."""
    runs = list(runs)
    changed = True
    while changed:
        changed = False
        p = t = r = 0
        while r < len(runs):
            L, op = runs[r]
            if op in "ID" and 0 < r < len(runs) - 2 and runs[r + 1][1] == "M" and runs[r - 1][1] == "M":
                S, g = (P, p) if op == "D" else (T, t)
                nl = runs[r + 1][0]
                keep = 1 if runs[r + 2][1] == op else 0
                k = 0
                while k < nl - keep and S[g + k] == S[g + L + k]:
                    k += 1
                if k:
                    runs[r - 1] = (runs[r - 1][0] + k, "M")
                    runs[r + 1] = (nl - k, "M")
                    if nl == k:
                        del runs[r + 1]
                    p += k
                    t += k
                    changed = True
            if op != "I":
                p += L
            if op != "D":
                t += L
            r += 1
    return runs


def seeded_cases(count, seed=0x1EF7, lo=60, hi=400):
    rng = random.Random(seed)
    return [planted_case(rng, rng.randint(lo, hi), rng.choice([0.02, 0.08, 0.2])) for _ in range(count)]
