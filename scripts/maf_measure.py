"""What --maf costs (profiles/maf.md).  Four parts:

  stage LABEL FASTA MAPPING OUTDIR [REPS]
                   align_paf in one process with the switch off / --maf / --maf with split 50 / --cs=long, every mode once as warm-up,
                   then REPS rounds alternating; host clock = ms_total of the summary; then one pass each with WFM_DEBUG=1 for the stages'
                   own lines (the library's `[wfm] maf` line has the kernels' device events, the driver's `[wflign] maf` line upload,
                   device call and text).  The PAF of every mode is held against the PAF with the switch off.
  offline FASTA ALIGNED.paf OUTDIR [REPS]
                   wfmh_maf_paf on an existing aligned PAF, host clock around the call; the file is held against the align phase's where
                   OUTDIR has one (LABEL lpa).
  rows [GIB] [REPS]
                   GIB GiB of rows through wfm_maf_rows alone: problems of 4 Mi columns each, windows of ONE stored sequence by reference,
                   all on one run list -- `mixed` (runs of 18 - 20 matches between 1X, 2I, 2D) and `long` (one = run per problem).  Host
                   clock around the call, and the library's own line with WFM_DEBUG=1 (device events around index and blocks + write).
  splits           does the host time of wfm_maf_rows follow `split`, or the order of the calls?  660 seeded problems of 32 000 columns
                   (42 MB of rows, some gap stretches of 60 and 70 bases), ONE seqset, calls with split 0 / 50 / 10^9 in a mixed order,
                   each with the library's own line (WFM_DEBUG=1) and the host clock around the call.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from wfmash_amd import capi, synth  # noqa: E402


def stage(label, fa, paf, outdir, reps):
    h = capi.Handle(0)
    modes = [("off", None, 0), ("maf", 0, 0), ("maf50", 50, 0), ("cslong", None, 2)]

    def run(name, split, cs):
        capi.set_maf(os.path.join(outdir, "%s_%s.maf" % (label, name)) if split is not None else None, split or 0)
        capi.set_cs(cs)
        out = os.path.join(outdir, "%s_%s.paf" % (label, name))
        s = capi.align_paf(h, fa, paf, out, params=dict(threads=16))
        counts = capi.maf_counts()
        capi.set_maf(None)
        capi.set_cs(0)
        return dict(ms_total=round(s.ms_total, 2), written=int(s.written), batches=int(s.batches), maf=counts)

    for m in modes:
        run(*m)
    plain = open(os.path.join(outdir, "%s_off.paf" % label), "rb").read()
    same = {m[0]: open(os.path.join(outdir, "%s_%s.paf" % (label, m[0])), "rb").read() == plain for m in modes[1:3]}
    print(json.dumps({"label": label, "paf_bytes": len(plain), "paf_equal_to_off": same,
                      "maf_bytes": os.path.getsize(os.path.join(outdir, "%s_maf.maf" % label)),
                      "maf50_bytes": os.path.getsize(os.path.join(outdir, "%s_maf50.maf" % label))}), flush=True)
    res = {m[0]: [] for m in modes}
    for _ in range(reps):
        for m in modes:
            res[m[0]].append(run(*m))
    for name in res:
        print(json.dumps({"label": label, "mode": name, "ms_total": [r["ms_total"] for r in res[name]], "last": res[name][-1]}), flush=True)
    os.environ["WFM_DEBUG"] = "1"
    for _ in range(reps):
        for m in modes[1:]:
            sys.stderr.write("==== %s %s (WFM_DEBUG) ====\n" % (label, m[0]))
            sys.stderr.flush()
            run(*m)
    h.close()


def offline(fa, paf, outdir, reps):
    h = capi.Handle(0)
    out = os.path.join(outdir, "offline.maf")
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        counts = capi.maf_paf(h, fa, paf, out)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    h.close()
    ref = os.path.join(outdir, "lpa_maf.maf")
    print(json.dumps({"offline": "wfmh_maf_paf", "paf_bytes": os.path.getsize(paf), "counts": counts, "first_call_ms": ms[0], "ms": ms[1:],
                      "equal_to_the_align_phase": open(out, "rb").read() == open(ref, "rb").read() if os.path.exists(ref) else None}), flush=True)


def rows(gib, reps):
    cols = 4 << 20
    n = int(gib * (1 << 30)) // (2 * cols)
    unit = [(18, 0), (1, 1), (20, 0), (2, 2), (19, 0), (1, 1), (20, 0), (2, 3)]  # 83 columns, 81 bases of each side
    k = cols // 83
    mixed = [(ln << 2) | op for ln, op in unit] * k
    plen = 81 * k
    fill = cols - 83 * k  # a last = run, so that the problem has `cols` columns
    mixed.append((fill << 2) | 0)
    plen += fill
    shapes = {"mixed": (np.array(mixed, dtype=np.uint32), plen), "long": (np.array([(cols << 2) | 0], dtype=np.uint32), cols)}
    h = capi.Handle(0)
    store = h.seqstore()
    assert store.add(synth.random_dna(0x3AF, 2 * cols)) == 0
    for name, (words, length) in shapes.items():
        refs = [dict(pattern_seq=0, pattern_off=0, plen=length, text_seq=0, text_off=cols, tlen=length, text_revcomp=0, mode=capi.WFM_MODE_END2END_UNI)] * n
        S = h.upload_refs(store, refs)
        results = [(0, -1, 0, 2 * length, len(words))] * n
        ms = []
        os.environ.pop("WFM_DEBUG", None)
        for r in range(reps + 2):
            if r == reps + 1:
                os.environ["WFM_DEBUG"] = "1"
                sys.stderr.write("==== rows %s (WFM_DEBUG) ====\n" % name)
                sys.stderr.flush()
            t0 = time.perf_counter()
            blocks, out, per = h.maf_rows(S, results, words, 0)
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        assert len(blocks) == n and len(out) == 2 * cols * n and all(c.flags == 0 for c in per)
        assert out[:2 * cols] == out[-2 * cols:]  # every problem spells the same rows
        print(json.dumps({"rows": name, "problems": n, "runs_each": len(words), "row_bytes": len(out), "sequence_bytes_read": 2 * length * n,
                          "first_call_ms": ms[0], "ms": ms[1:-1], "with_debug_ms": ms[-1]}), flush=True)
        del out
        S.free()
    store.free()
    h.close()


def splits():
    import random
    rng = random.Random(7)
    items, results, words = [], [], []
    for i in range(660):
        runs, left = [], 32000
        while left > 0:
            m = min(left, rng.randint(20, 400))
            runs.append((m, 0))
            left -= m
            if left > 0:
                runs.append(rng.choice([(1, 1), (1, 1), (2, 2), (3, 3), (60, 2), (1, 1), (70, 3)] if rng.random() < 0.05 else [(1, 1), (2, 2), (1, 3)]))
        plen = sum(n for n, o in runs if o != 2)
        tlen = sum(n for n, o in runs if o != 3)
        items.append((synth.random_dna(i, plen), synth.random_dna(i + 5000, tlen), capi.WFM_MODE_END2END_UNI))
        w = [(n << 2) | o for n, o in runs]
        results.append((0, -1, len(words), plen + tlen, len(w)))
        words += w
    words = np.array(words, dtype=np.uint32)
    h = capi.Handle(0)
    S = h.upload(items)
    os.environ["WFM_DEBUG"] = "1"
    for split in (0, 50, 0, 50, 50, 0, 0, 10**9, 50, 10**9, 0, 50):
        t0 = time.perf_counter()
        b, r, p = h.maf_rows(S, results, words, split)
        print(json.dumps({"split": split, "blocks": len(b), "row_bytes": len(r), "python_call_ms": round((time.perf_counter() - t0) * 1e3, 2)}), flush=True)
        del b, r
    S.free()
    h.close()


if __name__ == "__main__":
    a = sys.argv
    if a[1] == "stage":
        stage(a[2], a[3], a[4], a[5], int(a[6]) if len(a) > 6 else 3)
    elif a[1] == "offline":
        offline(a[2], a[3], a[4], int(a[5]) if len(a) > 5 else 3)
    elif a[1] == "splits":
        splits()
    else:
        rows(float(a[2]) if len(a) > 2 else 1.0, int(a[3]) if len(a) > 3 else 3)
