"""The GPU-free side of --verify / --verify-paf: the layout of wfm_check_t, the exported symbols, and the PAF line parser of the
verifier (wfmash_amd/host/verify_paf.cpp) through its test hook."""
import ctypes as C

from wfmash_amd import capi


def _line(qs=100, qe=140, strand="+", ts=2000, te=2042, cg="cg:Z:20=1X5=2I10=4D2=", qlen=5000, tlen=9000, extra=("gi:f:0.97", "bi:f:0.95")):
    f = ["q#1#chr1", str(qlen), str(qs), str(qe), strand, "t#1#chr2", str(tlen), str(ts), str(te), "37", "44", "60"] + list(extra)
    if cg is not None:
        f.append(cg)
    return "\t".join(f)


def test_check_layout_and_constants():
    assert C.sizeof(capi.Check) == 48
    assert [f[0] for f in capi.Check._fields_][:6] == ["flags", "score", "bad_p", "bad_t", "bad_run", "n_runs"]
    assert (capi.WFM_CK_NOT_CHECKED, capi.WFM_CK_BAD_RUN, capi.WFM_CK_SPANS, capi.WFM_CK_M_DIFFERS, capi.WFM_CK_X_EQUAL, capi.WFM_CK_SCORE,
            capi.WFM_CK_COUNTS) == (1, 2, 4, 8, 16, 32, 64)
    assert capi.CHECK_SLICE == 16384


def test_symbols_exported():
    L = capi.load()
    assert "wfm_check_runs" in capi.EXPORTS
    for name in ("wfm_check_runs", "wfmh_set_verify", "wfmh_verify_counts", "wfmh_verify_paf", "wfmh_test_verify_parse"):
        getattr(L, name)
    for name in ("wfmh_set_verify", "wfmh_verify_counts", "wfmh_verify_paf", "wfmh_test_verify_parse"):
        assert name in capi.HOST_EXPORTS


def test_verify_counts_without_a_run():
    capi.set_verify(True)
    assert capi.verify_counts() == (0, 0, 0, 0)
    capi.set_verify(False)
    assert capi.verify_counts() == (0, 0, 0, 0)


def test_parse_forward_and_reverse_lines():
    assert capi.host_verify_parse(_line()) == "\t".join(["ok", "q#1#chr1", "100", "140", "+", "t#1#chr2", "2000", "2042", "20=1X5=2I10=4D2="])
    got = capi.host_verify_parse(_line(strand="-", cg="cg:Z:40=2D"))
    assert got == "\t".join(["ok", "q#1#chr1", "100", "140", "-", "t#1#chr2", "2000", "2042", "40=2D"])
    # the tag may stand anywhere behind the twelve fixed fields
    assert capi.host_verify_parse(_line(extra=(), cg="cg:Z:7X") + "\tmd:f:0.9").split("\t")[-1] == "7X"


def test_parse_takes_the_coordinates_as_written():
    """no padding, no clamping, no strand arithmetic: a window of length 0 and a window at the very end come back as they stand"""
    got = capi.host_verify_parse(_line(qs=0, qe=0, ts=8999, te=9000, cg="cg:Z:1D")).split("\t")
    assert got[0] == "ok" and got[2:4] == ["0", "0"] and got[6:8] == ["8999", "9000"]
    got = capi.host_verify_parse(_line(qs=4999, qe=5000, strand="-", ts=0, te=1, cg="cg:Z:1=")).split("\t")
    assert got[2:5] == ["4999", "5000", "-"] and got[6:8] == ["0", "1"]


def test_parse_unverifiable_lines():
    assert capi.host_verify_parse(_line(cg=None)).split("\t")[0] == "unverifiable"
    assert capi.host_verify_parse(_line(cg="cg:Z:40M")).split("\t")[0] == "unverifiable"
    assert capi.host_verify_parse(_line(cg="cg:Z:20=3M17=")).split("\t")[0] == "unverifiable"
    # (an op outside =XID wins over whatever else is wrong with the CIGAR)
    assert capi.host_verify_parse(_line(cg="cg:Z:0=40M")).split("\t")[0] == "unverifiable"


def test_parse_refuses_bad_counts_and_fields():
    for cg in ("cg:Z:20=0X20=", "cg:Z:0=", "cg:Z:%d=" % (1 << 30), "cg:Z:%d=" % (1 << 40), "cg:Z:=", "cg:Z:12", "cg:Z:5=X"):
        assert capi.host_verify_parse(_line(cg=cg)).split("\t")[0] == "malformed", cg
    assert capi.host_verify_parse(_line(cg="cg:Z:%d=" % ((1 << 30) - 1))).split("\t")[0] == "ok"
    assert capi.host_verify_parse(_line(strand="*")).split("\t")[0] == "malformed"
    assert capi.host_verify_parse(_line(qs=141)).split("\t")[0] == "malformed"       # runs backwards
    assert capi.host_verify_parse(_line(te=9001)).split("\t")[0] == "malformed"      # past the length the line states
    assert capi.host_verify_parse(_line(ts="12a")).split("\t")[0] == "malformed"
    assert capi.host_verify_parse("q\t1\t0\t1\t+\tt").split("\t")[0] == "malformed"
