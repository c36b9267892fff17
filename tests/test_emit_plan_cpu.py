"""The chunk plan of the passes that emit lists (wfmash_amd/csrc/wfa_emit_plan.h) against a linear planner, through a stand-alone program
under ASan and UBSan, without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emit_plan_under_sanitizers(tmp_path):
    """scripts/micro/emit_plan_check.cpp: the header alone, driven by a program of its own with its own main, run directly.  The two
    runtimes are linked INTO the program (-static-libasan, -static-libubsan) and nothing is preloaded for it; no sanitizer goes near
    Python or the GPU"""
    exe = str(tmp_path / "emit_plan_check")
    src = os.path.join(ROOT, "scripts", "micro", "emit_plan_check.cpp")
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        src, "-o", exe], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr[-2000:]
    r = subprocess.run(["timeout", "-k", "10", "60", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "emit_plan_check: ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-2000:])


def test_plan_header_names_no_device_header():
    text = open(os.path.join(ROOT, "wfmash_amd", "csrc", "wfa_emit_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
