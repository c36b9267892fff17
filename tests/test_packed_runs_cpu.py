"""The two sources of packed runs (wfmash_amd/host/packed_runs.hpp) against each other -- a record's ops as the align batch packs them, and
the same record's PAF line as the --*-paf modes pack it -- through a stand-alone program under ASan and UBSan, without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_runs_under_sanitizers(tmp_path):
    """scripts/micro/packed_runs_check.cpp: the header alone, driven by a program of its own with its own main, run directly.  The two
    runtimes are linked INTO the program (-static-libasan, -static-libubsan) and nothing is preloaded for it; no sanitizer goes near
    Python or the GPU"""
    exe = str(tmp_path / "packed_runs_check")
    src = os.path.join(ROOT, "scripts", "micro", "packed_runs_check.cpp")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    r = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "packed_runs_check: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


def test_packed_runs_header_names_no_device_header():
    """the header and what it includes are host code: no HIP header, nothing of csrc/"""
    host = os.path.join(ROOT, "wfmash_amd", "host")
    seen, todo = set(), ["packed_runs.hpp"]
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        for line in open(os.path.join(host, name)).read().splitlines():
            if not line.startswith("#include"):
                continue
            inc = line.split()[1]
            assert "hip/" not in inc and "csrc" not in inc, (name, inc)
            if inc.startswith('"') and "/" not in inc:
                todo.append(inc.strip('"'))
    assert {"packed_runs.hpp", "cigar_ops.hpp", "chain_text.hpp", "coverage_text.hpp", "verify_parse.hpp"} <= seen, seen
