"""Times of the transitive closure on synthetic lists (profiles/transitive.md): records at depth 8 over a world sized for them, and a pile
of 1000 records over the same bases; wfm_trans_add, the index, the closure at depth 2 and to the fixed point, and device memory per run and
per arc; beside them the fast NumPy form of tests/trans_model.py on the same input where it ends within a minute.

    python scripts/transitive_time.py [--runs 100000,1000000,10000000] [--numpy-max 1000000] > out.jsonl"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import trans_model as TM  # noqa: E402
from wfmash_amd import capi  # noqa: E402

RUNS_PER_RECORD = 257  # 128 x (= run, gap run) and a last = run


def make(n_runs, depth, rng, pile=False):
    """records of RUNS_PER_RECORD runs (~12.9 kb of target each), `depth` of them over every target base; the queries lie in the second half
    of the world at random places.  pile: 1000 records over the same 13 kb"""
    n_rec = 1000 if pile else max(1, n_runs // RUNS_PER_RECORD)
    lens = rng.integers(50, 151, size=(n_rec, 128))
    gaps = rng.integers(1, 4, size=(n_rec, 128))
    ops = rng.integers(1, 4, size=(n_rec, 128))  # X, I or D
    words = np.empty((n_rec, RUNS_PER_RECORD), dtype=np.uint32)
    words[:, 0:256:2] = lens << 2
    words[:, 1:256:2] = (gaps << 2) | ops
    words[:, 256] = 100 << 2
    P = lens.sum(1) + 100 + np.where(ops != 2, gaps, 0).sum(1)
    T = lens.sum(1) + 100 + np.where(ops != 3, gaps, 0).sum(1)
    span = int(P.max()) + 1
    half = 2 * span if pile else max(2 * span, (n_rec * span) // depth + span)
    t = np.zeros(n_rec, dtype=np.int64) if pile else rng.integers(0, half - span, size=n_rec)
    q = half + rng.integers(0, half - span, size=n_rec)
    rev = rng.random(n_rec) < 0.3
    probs = np.zeros(n_rec, dtype=capi.TRANS_PROB_DTYPE)
    probs["t"], probs["q"] = t, q
    probs["runs_off"] = np.arange(n_rec, dtype=np.uint64) * RUNS_PER_RECORD
    probs["n_runs"] = RUNS_PER_RECORD
    probs["flags"] = rev
    return probs, words.reshape(-1), 2 * half


def model_records(probs, words):
    out = []
    for p in probs:
        w = words[int(p["runs_off"]):int(p["runs_off"]) + int(p["n_runs"])]
        out.append((int(p["t"]), int(p["q"]), bool(p["flags"]), [(int(x) >> 2, "=XID"[int(x) & 3]) for x in w]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="100000,1000000,10000000")
    ap.add_argument("--numpy-max", type=int, default=1000000)
    ap.add_argument("--fixed-max", type=int, default=2000000, help="the largest list whose closure is also taken to the fixed point")
    ap.add_argument("--seeds", type=int, default=100)
    args = ap.parse_args()
    h = capi.Handle(0)
    L = h._L
    cases = [(int(v), False) for v in args.runs.split(",") if v] + [(1000 * RUNS_PER_RECORD, True)]
    for n_runs, pile in cases:
        rng = np.random.default_rng(n_runs + pile)
        probs, words, n_bases = make(n_runs, 8, rng, pile)
        seeds = [(int(a), int(a) + 1000) for a in rng.integers(0, n_bases // 2 - 14000 if not pile else 10000, size=args.seeds)]
        row = dict(case="pile" if pile else "depth8", records=len(probs), runs=len(words), n_bases=n_bases, seeds=len(seeds))
        obj = h.transitive(n_bases)
        flags = np.zeros(len(probs), dtype=np.uint32)
        t0 = time.perf_counter()
        step = 1 << 16  # (records a call, as a batch of the driver)
        for a in range(0, len(probs), step):
            part = probs[a:a + step].copy()
            lo, hi = int(part["runs_off"][0]), int(part["runs_off"][-1]) + RUNS_PER_RECORD
            part["runs_off"] -= lo
            w = words[lo:hi]
            rc = L.wfm_trans_add(h._p, obj._p, part.ctypes.data, len(part), w.ctypes.data, len(w), flags.ctypes.data)
            assert rc == 0, (rc, h.last_error())
        row["add_ms"] = (time.perf_counter() - t0) * 1e3
        c = obj.counts()
        row["device_bytes_kept"] = c[1] * 16 + c[2] * 72
        row["bytes_per_run"] = c[1] * 16 / len(words)
        # (to the fixed point a seed reaches most of the world: ten seeds, and not on the largest list)
        calls = [(2, "depth2", seeds), (2, "depth2_warm", seeds)]
        if len(words) <= args.fixed_max:
            calls += [(0, "fixed", seeds[:10]), (0, "fixed_warm", seeds[:10])]
        for depth, key, sd in calls:
            t0 = time.perf_counter()
            ivs, per = obj.closure(sd, depth)
            row[key + "_ms"] = (time.perf_counter() - t0) * 1e3
            cc = obj.counts()
            row[key] = dict(rounds=cc[3], intervals=cc[4], pairs=cc[5], bases=int(per["bases"].sum()))
        obj.close()
        if len(words) <= args.numpy_max:
            recs = model_records(probs, words)
            t0 = time.perf_counter()
            fast = TM.Fast(recs)
            row["numpy_build_ms"] = (time.perf_counter() - t0) * 1e3
            for depth, key, sd in ((2, "numpy_depth2_ms", seeds), (0, "numpy_fixed_ms", seeds[:10])):
                t0 = time.perf_counter()
                got = fast.closures(sd, depth)
                row[key] = (time.perf_counter() - t0) * 1e3
            assert [(int(a), int(b), int(s)) for a, b, s in zip(ivs["start"], ivs["end"], ivs["seed"])] == got[0]  # (the last device call was to the fixed point)
        print(json.dumps(row), flush=True)
    h.close()


if __name__ == "__main__":
    main()
