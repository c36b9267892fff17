"""CPU tests of -P / --max-length: "inf" lifts the limit as in the reference's parser (parse_args.hpp:472-483)."""
import os
import subprocess

from tests import filter_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "wfmash_amd", "wfmash-hip")


def _cli(args, cwd):
    return subprocess.run([CLI] + args, cwd=str(cwd), capture_output=True, text=True, timeout=60)


def test_max_length_inf_is_accepted(tmp_path):
    """-P inf gets past the parser: the run is refused for its missing -B directory, before a device is opened"""
    fa = FC.write_fai(str(tmp_path))
    for flag in ("-P", "--max-length"):
        r = _cli([flag, "inf", "-B", "/nonexistent/dir", fa], tmp_path)
        assert r.returncode == 1
        assert "-P expects a size" not in r.stderr
        assert "(-B) /nonexistent/dir does not exist or is not writable" in r.stderr


def test_max_length_still_refuses_nonsense(tmp_path):
    fa = FC.write_fai(str(tmp_path))
    r = _cli(["-P", "infinite", fa], tmp_path)
    assert r.returncode == 1 and "-P expects a size such as 5000, 50k, 1m" in r.stderr
    r = _cli(["-P", "0", fa], tmp_path)
    assert r.returncode == 1 and "max mapping length must be greater than 0" in r.stderr
