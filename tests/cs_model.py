"""minimap2's cs difference string as wfm_cs_strings spells it (include/wfmash_hip.h states the grammar), in plain Python, and its inverse.

Runs are (length, op) with op one of 'M', 'X', 'I', 'D' as in tests/left_align_model.py; P is the pattern (target), T the text (query,
strand-adjusted), both bytes.  Nothing here is shared with the library.  The string is spelled from the runs, never from a comparison."""
import re

SHORT, LONG = 0, 1


def lc(b):
    """'A'..'Z' -> 'a'..'z', every other byte as it is"""
    return bytes(c + 32 if 65 <= c <= 90 else c for c in b)


def cs_of(P, T, runs, form):
    out, p, t = [], 0, 0
    for n, op in runs:
        if op == "M":
            out.append(b"=" + P[p:p + n] if form == LONG else b":%d" % n)
            p += n
            t += n
        elif op == "X":
            out.append(b"".join(b"*" + lc(P[p + j:p + j + 1]) + lc(T[t + j:t + j + 1]) for j in range(n)))
            p += n
            t += n
        elif op == "I":
            out.append(b"+" + lc(T[t:t + n]))
            t += n
        else:
            out.append(b"-" + lc(P[p:p + n]))
            p += n
    return b"".join(out)


_TOKEN = re.compile(rb":(\d+)|=([^:=*+\-]+)|\*([^:=*+\-])([^:=*+\-])|\+([^:=*+\-]+)|-([^:=*+\-]+)")


def decode(cs, P=None):
    """The long form (no P): (P', T') from the string alone, both lower-cased wherever the string lower-cases (X, I, D) and as written
    in the = runs.  The short form (P given): T' from P, taking the bases of the : runs from P and the others, lower-cased, from the
    string.  Raises ValueError on anything the grammar does not spell."""
    pat, txt, at, p = [], [], 0, 0
    while at < len(cs):
        m = _TOKEN.match(cs, at)
        if not m:
            raise ValueError("bad cs at byte %d: %r" % (at, cs[at:at + 20]))
        at = m.end()
        n, eq, xa, xb, ins, dele = m.groups()
        if n is not None:
            if P is None:
                raise ValueError("a short cs string needs the pattern")
            n = int(n)
            if n <= 0 or p + n > len(P):
                raise ValueError("a : run of %d bases at pattern index %d of %d" % (n, p, len(P)))
            txt.append(P[p:p + n])
            pat.append(P[p:p + n])
            p += n
        elif eq is not None:
            pat.append(eq)
            txt.append(eq)
            p += len(eq)
        elif xa is not None:
            pat.append(xa)
            txt.append(xb)
            p += 1
        elif ins is not None:
            txt.append(ins)
        else:
            pat.append(dele)
            p += len(dele)
    if P is not None:
        if p != len(P):
            raise ValueError("the string covers %d of %d pattern bases" % (p, len(P)))
        return b"".join(txt)
    return b"".join(pat), b"".join(txt)


def same_bases(a, b):
    """equal but for the case decode() cannot give back"""
    return lc(a) == lc(b)
