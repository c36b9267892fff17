"""TEST INFRASTRUCTURE ONLY -- restatement of CommonFunc::sketchSequenceStreaming (src/map/include/commonFunc.hpp:338-430),
the target sketch of `--streaming-minhash`, composed of the reference's own pieces as oracle/pymap.py exposes them from
oracle/_ref/libref_map.so: makeUpperCaseAndValidDNA, reverseComplement, getHash and StreamingMinHash.  Only the glue is
restated here: the ambiguous-k-mer counter, the first position of every canonical hash, and the records made of the sketch.

`brute_force` states the same result without any of the reference's pieces but getHash, for the CPU tests of the restatement."""
import ctypes as C

import numpy as np

from oracle import pymap

MINMER = pymap.MINMER
FWD = 1


def _records(sketch, first, w, seq_id):
    recs = sorted(((int(h), first[int(h)], first[int(h)] + w, seq_id, FWD, 0) for h in sketch), key=lambda r: r[1])
    return np.array(recs, dtype=MINMER) if recs else np.zeros(0, dtype=MINMER)


def streaming_sketch(seq: bytes, k: int, w: int, s: int, seq_id: int = 0):
    """The records sketchSequenceStreaming appends for one sequence, ordered by wpos (MINMER array)."""
    L = pymap._load("ref")
    n = len(seq)
    if n < k:
        return np.zeros(0, dtype=MINMER)
    buf = C.create_string_buffer(seq, n)
    L.ref_upper_valid(buf, n)                      # step 1 (the reference works on the sequence in place)
    t = buf.raw[:n]
    N = ord("N")
    get_hash = L.ref_get_hash
    rev = C.create_string_buffer(k)
    ambig = 0                                      # step 2: the counter, armed by the last N among the first k bases
    for i in range(k - 1, -1, -1):
        if t[i] == N:
            ambig = i + 1
            break
    values, first = [], {}
    for i in range(n - k + 1):
        if t[i + k - 1] == N:
            ambig = k
        if ambig == 0:                             # step 3: canonical hash, palindromes skipped
            kmer = t[i:i + k]
            fwd = get_hash(kmer, k)
            L.ref_revcomp(kmer, rev, k)
            bwd = get_hash(rev.raw[:k], k)
            if fwd != bwd:
                c = min(fwd, bwd)
                first.setdefault(c, i)             # step 4: first position among the k-mers not skipped
                values.append(c)
        if ambig > 0:
            ambig -= 1
    sketch = pymap.ref_streaming_minhash(np.array(values, dtype=np.uint64), s)   # StreamingMinHash itself
    return _records(sketch, first, w, seq_id)      # steps 5 and 6


def streaming_sketch_multi(seqs, k: int, w: int, s: int, seq_ids=None):
    """The records of several sequences grouped in input order (what wfm_streaming_minmers returns)."""
    ids = list(seq_ids) if seq_ids is not None else list(range(len(seqs)))
    parts = [streaming_sketch(x, k, w, s, sid) for x, sid in zip(seqs, ids)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=MINMER)


_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def brute_force(seq: bytes, k: int, w: int, s: int, seq_id: int = 0):
    """Every k-mer without a non-ACGT base (case-insensitive) and with distinct strand hashes, as (canonical hash, position);
    the s smallest pairs are the sketch, and a hash's position is the smallest of all its occurrences."""
    t = bytes(b if b in b"ACGT" else ord("N") for b in seq.upper())
    pairs = []
    for i in range(len(t) - k + 1):
        kmer = t[i:i + k]
        if b"N" in kmer:
            continue
        fwd = pymap.get_hash(kmer, which="ref")
        bwd = pymap.get_hash(kmer.translate(_COMP)[::-1], which="ref")
        if fwd != bwd:
            pairs.append((min(fwd, bwd), i))
    pairs.sort()
    first = {}
    for h, i in pairs:
        first.setdefault(h, i)
    return _records([h for h, _ in pairs[:s]], first, w, seq_id)
