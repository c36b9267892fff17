"""bench.py's launch contract: `python bench.py --gpus N` without a torch.distributed environment starts N ranks
itself (one process per GPU under torch.distributed.run, rendezvous on 127.0.0.1); under the driver's own launcher
(WORLD_SIZE set) it joins the existing job.  --rank-check stops after the ranks have found each other (gloo, no GPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _clean_env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    return env


def _json_lines(text):
    out = []
    dec = json.JSONDecoder()
    for line in text.splitlines():
        line = line.strip()
        while line.startswith("{"):  # two ranks may share a line of the pipe
            try:
                obj, end = dec.raw_decode(line)
            except ValueError:
                break
            out.append(obj)
            line = line[end:].lstrip()
    return out


def test_gpus_flag_launches_that_many_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rank-check"], cwd=ROOT, env=_clean_env(), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [j for j in _json_lines(r.stdout) if j.get("rank_check")]
    assert sorted(j["rank"] for j in lines) == [0, 1]
    assert all(j["n_gpus"] == 2 and j["ranks_seen"] == [0, 1] for j in lines)


def test_gpus_flag_must_agree_with_the_launcher():
    env = dict(_clean_env(), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rank-check"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_print_one_line_for_the_job():
    """The N>1 path end to end on the one-GPU box: two ranks share the device (gloo instead of RCCL), each aligns its own
    shard, the CIGAR payload is gathered to rank 0, rank 0 prints the one JSON line with n_gpus = 2."""
    env = dict(_clean_env(), WFM_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--pairs", "4", "--full", "--no-cpu-baseline"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [j for j in _json_lines(r.stdout) if "metric" in j]
    assert len(lines) == 1
    j = lines[0]
    assert j["n_gpus"] == 2 and j["steps"] == 1 and j["scaling"] == "weak"
    assert j["value"] > 0 and j["roofline"]["frac"] > 0


def test_strong_scaling_shards_one_file_over_the_ranks():
    """--scaling strong: the same --total-pairs records at every N, dealt out by dist.shard_records -- every record on
    exactly one rank, the shards level."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rank-check", "--scaling", "strong", "--total-pairs", "13"], cwd=ROOT,
                       env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = sorted((j for j in _json_lines(r.stdout) if j.get("rank_check")), key=lambda j: j["rank"])
    assert [j["scaling"] for j in lines] == ["strong", "strong"]
    assert sorted(lines[0]["records"] + lines[1]["records"]) == list(range(13))
    assert abs(len(lines[0]["records"]) - len(lines[1]["records"])) <= 1
    one = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--rank-check", "--scaling", "strong", "--total-pairs", "13"], cwd=ROOT,
                         env=_clean_env(), capture_output=True, text=True, timeout=600)
    assert [j["records"] for j in _json_lines(one.stdout) if j.get("rank_check")] == [list(range(13))]


@pytest.mark.gpu
def test_strong_scaling_two_ranks_on_one_gpu():
    env = dict(_clean_env(), WFM_BENCH_SHARE_GPU="1")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--scaling", "strong", "--total-pairs", "6",
                        "--no-cpu-baseline"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    (j,) = [j for j in _json_lines(r.stdout) if "metric" in j]
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["config"]["pairs_total"] == 6 and j["config"]["pairs_per_gpu"] == 3
    assert j["value"] > 0


@pytest.mark.gpu
def test_c4_all_vs_all_two_ranks_give_the_records_of_one(tmp_path):
    """bench.py --config C4 (north_star's C4 as one job: all eight haplotypes against all eight, the queries sharded over the ranks for the
    map phase, the mapping records of all queries exchanged and sharded by weight for the align phase, the PAF gathered to rank 0): two ranks
    sharing the one GPU of the box must produce, byte for byte, the records one rank produces."""
    outs = []
    for n in (1, 2):
        out = tmp_path / f"c4.n{n}.paf"
        env = dict(_clean_env(), WFM_BENCH_SHARE_GPU="1")
        r = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--config", "C4", "--c4-mbp", "1.5", "--steps", "1", "--warmup", "0",
                            "--no-cpu-baseline", "--out-paf", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stderr[-3000:]
        (j,) = [j for j in _json_lines(r.stdout) if "metric" in j]
        assert j["n_gpus"] == n and j["scaling"] == "strong" and j["value"] > 0
        assert j["config"]["queries_total"] == 8 and j["config"]["records_total"] > 50
        assert j["roofline"]["bound"] == "valu"
        outs.append(out.read_bytes())
    assert len(outs[0]) > 10000 and outs[0] == outs[1]


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_stays_in_budget_and_ignores_the_outputs(tmp_path):
    """--dump-outputs past its byte budget: a sample of the records fixed by the inputs alone, float32 / float64 arrays within the budget."""
    import numpy as np
    from wfmash_amd.capi import AlignResult
    bench = _bench_module()
    pairs = [(b"A" * (100 + 7 * i), b"C" * (90 + 5 * i)) for i in range(40)]
    budget = 20_000
    dumps = []
    for op in (b"M", b"MX"):  # two runs whose outputs differ, not their inputs
        res = [AlignResult(0, i, op * (len(p) // len(op)), 1, 0) for i, (p, _) in enumerate(pairs)]
        d = tmp_path / op.decode()
        bench._dump_alignments(str(d), res, list(range(100, 140)), pairs, "", budget)
        arrays = {f.stem: np.load(f) for f in d.iterdir()}
        assert set(arrays) == {"record", "status", "score", "cigar_len", "cigar_ops"}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(f.stat().st_size for f in d.iterdir()) <= budget
        assert 0 < len(arrays["record"]) < len(pairs)
        assert arrays["cigar_len"].sum() == len(arrays["cigar_ops"])
        dumps.append(arrays)
    assert list(dumps[0]["record"]) == list(dumps[1]["record"])
    assert list(dumps[0]["score"]) == [r - 100 for r in dumps[0]["record"]]


def test_dump_outputs_refuses_the_c4_job(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--config", "C4", "--dump-outputs", str(tmp_path)], cwd=ROOT, env=_clean_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path, oracle):
    """A plain run prints the headline line alone (no roofline passes, CPU baseline or secondary legs) and --dump-outputs writes the
    last timed step's status, score and CIGAR of every record: the oracle's, record for record; the same again in a second process."""
    import numpy as np
    from wfmash_amd import synth
    dumps = []
    for run in range(2):
        d = tmp_path / f"out{run}"
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--pairs", "4", "--dump-outputs", str(d)],
                           cwd=ROOT, env=_clean_env(), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        (j,) = [j for j in _json_lines(r.stdout) if "metric" in j]
        assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
        assert not {"roofline", "cpu_baseline", "secondary", "legs"} & set(j)
        dumps.append({f.stem: np.load(f) for f in d.iterdir()})
    a = dumps[0]
    assert set(a) == {"record", "status", "score", "cigar_len", "cigar_ops"}
    assert all(np.array_equal(a[k], dumps[1][k]) for k in a)
    pairs = synth.pairs("C3", n_pairs=4)
    assert list(a["record"]) == [0, 1, 2, 3] and not a["status"].any()
    ops, scores, _, failed = oracle.align_batch_biwfa([p for p, _ in pairs], [q for _, q in pairs])
    assert list(a["score"]) == [int(s) for s in scores]
    cig = a["cigar_ops"].astype(np.uint8).tobytes()
    ends = np.cumsum(a["cigar_len"]).astype(np.int64)
    assert [cig[e - n:e] for e, n in zip(ends, a["cigar_len"].astype(np.int64))] == list(ops)
