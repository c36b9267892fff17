"""align_paf on (fasta, mapping paf) with --cs off / short / long / left-align / left-align + short, alternating; host clock = ms_total of
the summary.  Then one pass each with WFM_DEBUG=1 for the stage lines.  Usage: cs_measure.py LABEL FASTA MAPPING OUTDIR [REPS]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wfmash_amd import capi  # noqa: E402

label, fa, paf, outdir = sys.argv[1:5]
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
threads = 16
h = capi.Handle(0)
MODES = [("off", 0, False), ("short", 1, False), ("long", 2, False), ("left", 0, True), ("left+short", 1, True)]


def run(name, form, left):
    capi.set_cs(form)
    capi.set_left_align(left)
    out = os.path.join(outdir, "%s_%s.paf" % (label, name.replace("+", "_")))
    t0 = time.perf_counter()
    s = capi.align_paf(h, fa, paf, out, params=dict(threads=threads))
    wall = (time.perf_counter() - t0) * 1e3
    counts = capi.cs_counts()
    capi.set_cs(0)
    capi.set_left_align(False)
    return dict(ms_total=round(s.ms_total, 2), wall_ms=round(wall, 2), records=int(s.records), written=int(s.written), batches=int(s.batches),
                cs=counts, out_bytes=os.path.getsize(out))


for name, form, left in MODES:  # warm-up: every mode once (first use allocates the calls' device blocks and loads their kernels)
    run(name, form, left)
res = {m[0]: [] for m in MODES}
for _ in range(reps):
    for name, form, left in MODES:
        res[name].append(run(name, form, left))
for name in res:
    print(json.dumps({"label": label, "mode": name, "ms_total": [r["ms_total"] for r in res[name]], "wall_ms": [r["wall_ms"] for r in res[name]],
                      "last": res[name][-1]}), flush=True)
os.environ["WFM_DEBUG"] = "1"
for name, form, left in MODES[1:]:
    sys.stderr.write("==== %s %s (WFM_DEBUG) ====\n" % (label, name))
    sys.stderr.flush()
    run(name, form, left)
h.close()
