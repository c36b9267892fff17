"""The binding's table of ctypes prototypes (wfmash_amd/capi.py: PROTOTYPES) against the list of exported names, without the library."""
from wfmash_amd import capi


def test_prototype_table_covers_the_record_passes_exactly():
    first, last = capi.EXPORTS.index("wfm_check_runs"), capi.EXPORTS.index("wfm_trans_free_list")
    covered = capi.EXPORTS[first:last + 1]
    assert len(covered) == len(set(covered)) and len(capi.EXPORTS) == len(set(capi.EXPORTS))
    # (a dict holds a name once; the source must not state one twice either, where the later entry would win silently)
    text = open(capi.__file__).read()
    for name in covered:
        assert name in capi.PROTOTYPES, name
        assert text.count('"%s": ' % name) == 1, name
    assert set(capi.PROTOTYPES) <= set(capi.EXPORTS), sorted(set(capi.PROTOTYPES) - set(capi.EXPORTS))
    assert set(capi.PROTOTYPES) == set(covered), sorted(set(capi.PROTOTYPES) - set(covered))
    for name, (restype, argtypes) in capi.PROTOTYPES.items():
        assert restype is None or restype is capi.C.c_int, name
        assert isinstance(argtypes, list) and argtypes, name
