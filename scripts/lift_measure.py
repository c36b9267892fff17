"""What --lift costs (profiles/lift.md).  Three parts:

  bed FASTA OUT.bed [WIDTH]
                   a BED of WIDTH-base windows (1000) tiling every sequence of FASTA.
  stage LABEL FASTA MAPPING BED OUTDIR [REPS]
                   align_paf in one process with the switch off / --lift / --coverage / --variants / all three, every mode once as
                   warm-up, then REPS rounds alternating; host clock = ms_total of the summary; then one pass each with WFM_DEBUG=1
                   for the stages' own lines (the library's `[wfm] lift:` line splits the device call into index + count and write +
                   copy down).  The PAF of every mode is held against the PAF with the switch off.
  offline FASTA ALIGNED.paf BED OUTDIR [REPS] [MODEL_RECORDS]
                   wfmh_lift_paf on an existing aligned PAF, host clock around the call (it reads the FASTA index, the BED and the PAF,
                   lifts, writes the file); then, for orientation, the brute-force model of tests/lift_model.py on the first
                   MODEL_RECORDS lines (20) with the clock around it, and its lines held against the file's first ones.
"""
import gzip
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wfmash_amd import capi  # noqa: E402


def sequence_table(fasta):
    """names and lengths in file order"""
    names, lengths = [], []
    with (gzip.open(fasta, "rt") if fasta.endswith(".gz") else open(fasta)) as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                lengths.append(0)
            else:
                lengths[-1] += len(line.strip())
    return names, lengths


def bed(fasta, out, width):
    names, lengths = sequence_table(fasta)
    n = 0
    with open(out, "w") as f:
        for name, length in zip(names, lengths):
            for a in range(0, length, width):
                f.write("%s\t%d\t%d\t%s:%d\n" % (name, a, min(length, a + width), name, a // width))
                n += 1
    print(json.dumps({"bed": out, "sequences": len(names), "bases": sum(lengths), "intervals": n, "width": width}), flush=True)


def stage(label, fa, paf, bed_path, outdir, reps):
    h = capi.Handle(0)
    modes = [("off", False, False, False), ("lift", True, False, False), ("coverage", False, True, False), ("variants", False, False, True),
             ("all", True, True, True)]

    def run(name, lift, cover, var):
        capi.set_lift(bed_path if lift else None, os.path.join(outdir, "%s_%s.lift" % (label, name)) if lift else None)
        capi.set_coverage(os.path.join(outdir, "%s_%s.bg" % (label, name)) if cover else None)
        capi.set_variants(os.path.join(outdir, "%s_%s.vcf" % (label, name)) if var else None)
        out = os.path.join(outdir, "%s_%s.paf" % (label, name))
        s = capi.align_paf(h, fa, paf, out, params=dict(threads=16))
        counts = capi.lift_counts()
        capi.set_lift(None, None)
        capi.set_coverage(None)
        capi.set_variants(None)
        return dict(ms_total=round(s.ms_total, 2), written=int(s.written), batches=int(s.batches), lift=counts)

    for m in modes:
        run(*m)
    plain = open(os.path.join(outdir, "%s_off.paf" % label), "rb").read()
    same = {m[0]: open(os.path.join(outdir, "%s_%s.paf" % (label, m[0])), "rb").read() == plain for m in modes[1:]}
    print(json.dumps({"label": label, "paf_bytes": len(plain), "paf_equal_to_off": same,
                      "lift_equal_alone_and_beside": open(os.path.join(outdir, "%s_lift.lift" % label), "rb").read() ==
                      open(os.path.join(outdir, "%s_all.lift" % label), "rb").read()}), flush=True)
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


def offline(fa, paf, bed_path, outdir, reps, model_records):
    h = capi.Handle(0)
    out = os.path.join(outdir, "offline.lift")
    ms = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        counts = capi.lift_paf(h, fa, paf, bed_path, out)
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    h.close()
    print(json.dumps({"offline": "wfmh_lift_paf", "paf_bytes": os.path.getsize(paf), "counts": counts, "first_call_ms": ms[0], "ms": ms[1:]}), flush=True)
    from tests import lift_model as M
    names, lengths = sequence_table(fa)
    lines = [l for l in open(paf) if "\tcg:Z:" in l][:model_records]
    t0 = time.perf_counter()
    text, mc = M.lift_paf(lines, open(bed_path).read(), names, lengths)
    model_ms = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps({"offline": "python model", "records": len(lines), "lines": mc[1], "ms": model_ms,
                      "equal_to_the_head_of_the_file": open(out).read().startswith(text)}), flush=True)


if __name__ == "__main__":
    a = sys.argv
    if a[1] == "bed":
        bed(a[2], a[3], int(a[4]) if len(a) > 4 else 1000)
    elif a[1] == "stage":
        stage(a[2], a[3], a[4], a[5], a[6], int(a[7]) if len(a) > 7 else 3)
    else:
        offline(a[2], a[3], a[4], a[5], int(a[6]) if len(a) > 6 else 3, int(a[7]) if len(a) > 7 else 20)
