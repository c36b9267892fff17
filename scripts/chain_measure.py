"""What --chain costs (profiles/chain.md).  Three parts:

  stage LABEL FASTA MAPPING BED OUTDIR [REPS]
                   align_paf in one process with the switch off / --chain / --chain swapped / --lift / --coverage / all three, every
                   mode once as warm-up, then REPS rounds alternating; host clock = ms_total of the summary; then one pass each with
                   WFM_DEBUG=1 for the stages' own lines (the library's `[wfm] chain:` line has the two kernels' device events).  The
                   PAF of every mode is held against the PAF with the switch off.
  offline FASTA ALIGNED.paf OUTDIR [REPS]
                   wfmh_chain_paf on an existing aligned PAF, host clock around the call (it reads the FASTA index and the PAF, makes the
                   chains, writes the file); the file is held against the align phase's where OUTDIR has one (LABEL lpa).
  long [RUNS] [REPS]
                   ONE problem of RUNS runs (10^6), seeded, through wfm_chain_runs alone: one workgroup's work by construction.  Host
                   clock around the call, and the library's own line with WFM_DEBUG=1.
"""
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from wfmash_amd import capi  # noqa: E402


def stage(label, fa, paf, bed_path, outdir, reps):
    h = capi.Handle(0)
    modes = [("off", 0, False, False), ("chain", 1, False, False), ("swap", 2, False, False), ("lift", 0, True, False), ("coverage", 0, False, True),
             ("all", 1, True, True)]

    def run(name, chain, lift, cover):
        capi.set_chain(os.path.join(outdir, "%s_%s.chain" % (label, name)) if chain else None, chain == 2)
        capi.set_lift(bed_path if lift else None, os.path.join(outdir, "%s_%s.lift" % (label, name)) if lift else None)
        capi.set_coverage(os.path.join(outdir, "%s_%s.bg" % (label, name)) if cover else None)
        out = os.path.join(outdir, "%s_%s.paf" % (label, name))
        s = capi.align_paf(h, fa, paf, out, params=dict(threads=16))
        counts = capi.chain_counts()
        capi.set_chain(None)
        capi.set_lift(None, None)
        capi.set_coverage(None)
        return dict(ms_total=round(s.ms_total, 2), written=int(s.written), batches=int(s.batches), chain=counts)

    for m in modes:
        run(*m)
    plain = open(os.path.join(outdir, "%s_off.paf" % label), "rb").read()
    same = {m[0]: open(os.path.join(outdir, "%s_%s.paf" % (label, m[0])), "rb").read() == plain for m in modes[1:]}
    print(json.dumps({"label": label, "paf_bytes": len(plain), "paf_equal_to_off": same,
                      "chain_bytes": os.path.getsize(os.path.join(outdir, "%s_chain.chain" % label)),
                      "chain_equal_alone_and_beside": open(os.path.join(outdir, "%s_chain.chain" % label), "rb").read() ==
                      open(os.path.join(outdir, "%s_all.chain" % label), "rb").read()}), flush=True)
    res = {m[0]: [] for m in modes}
    for _ in range(reps):
        for m in modes:
            res[m[0]].append(run(*m))
    for name in res:
        print(json.dumps({"label": label, "mode": name, "ms_total": [r["ms_total"] for r in res[name]], "last": res[name][-1]}), flush=True)
    os.environ["WFM_DEBUG"] = "1"
    for m in modes[1:]:
        sys.stderr.write("==== %s %s (WFM_DEBUG) ====\n" % (label, m[0]))
        sys.stderr.flush()
        run(*m)
    h.close()


def offline(fa, paf, outdir, reps):
    h = capi.Handle(0)
    out = os.path.join(outdir, "offline.chain")
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        counts = capi.chain_paf(h, fa, paf, out)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    h.close()
    ref = os.path.join(outdir, "lpa_chain.chain")
    print(json.dumps({"offline": "wfmh_chain_paf", "paf_bytes": os.path.getsize(paf), "counts": counts, "first_call_ms": ms[0], "ms": ms[1:],
                      "equal_to_the_align_phase": open(out, "rb").read() == open(ref, "rb").read() if os.path.exists(ref) else None}), flush=True)


def long_record(n_runs, reps):
    rng = random.Random(0x10E6)
    runs, last = [], None
    for k in range(n_runs):
        op = rng.choice([o for o in range(4) if o != last]) if 0 < k < n_runs - 1 else 0
        if op == last:
            op = 1
        runs.append((rng.randrange(1, 40) << 2) | op)
        last = op
    runs = np.array(runs, dtype=np.uint32)
    h = capi.Handle(0)
    ms = []
    for r in range(reps + 1):
        if r == reps:
            os.environ["WFM_DEBUG"] = "1"
        t0 = time.perf_counter()
        blocks, per = h.chain_runs([(0, n_runs, 0)], runs)
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    h.close()
    print(json.dumps({"long": "wfm_chain_runs, one problem", "runs": n_runs, "blocks": int(per[0]["count"]), "flags": int(per[0]["flags"]),
                      "first_call_ms": ms[0], "ms": ms[1:-1], "with_debug_ms": ms[-1]}), flush=True)


if __name__ == "__main__":
    a = sys.argv
    if a[1] == "stage":
        stage(a[2], a[3], a[4], a[5], a[6], int(a[7]) if len(a) > 7 else 3)
    elif a[1] == "offline":
        offline(a[2], a[3], a[4], int(a[5]) if len(a) > 5 else 3)
    else:
        long_record(int(a[2]) if len(a) > 2 else 1000000, int(a[3]) if len(a) > 3 else 3)
