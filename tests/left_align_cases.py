"""Hand-built left-alignment problems with their expected CIGARs written out: (name, P, T, CIGAR in, CIGAR expected).  Shared by
tests/test_left_align_cpu.py (the model gives the expectation) and tests/test_left_align_gpu.py (the device gives it, and the model's)."""

F6, F8, TAIL9, TAIL10 = b"CGTTGC", b"CGTTGCCG", b"GTCCATGCA", b"GTCCATGCAT"
LEFT10 = b"CGTACGTTGC"
CAG = b"CAG"

HAND = [
    # 3D inside A x 20: all the way to the left flank
    ("hp_3d", LEFT10 + b"A" * 20 + TAIL10, LEFT10 + b"A" * 17 + TAIL10, "27=3D10=", "10=3D27="),
    # 6I inside (CAG) x 12: a gap of two periods rotates through the whole repeat
    ("cag_6i", LEFT10 + CAG * 10 + TAIL10, LEFT10 + CAG * 12 + TAIL10, "40=6I10=", "10=6I40="),
    # 4I inside (CAG) x 12: no multiple of the period, the rotation ends after the gap's own length
    ("cag_4i", LEFT10 + CAG * 12 + TAIL10, LEFT10 + CAG * 6 + b"CAGC" + CAG * 6 + TAIL10, "32=4I24=", "28=4I28="),
    # a gap directly behind an X run: the bases rotate, there is no room
    ("behind_x", F8 + b"A" + b"AAA" + b"AAGTCCATG", F8 + b"C" + b"AAGTCCATG", "8=1X3D9=", "8=1X3D9="),
    # the M run before the gap is used up and the gap ends against the X run: one run fewer
    ("m_consumed", F8 + b"T" + b"AAAA" + b"AAA" + b"AGTCCATGC", F8 + b"G" + b"AAAA" + b"AGTCCATGC", "8=1X4=3D9=", "8=1X3D13="),
    # an X run follows the gap: the d bases become an M run of their own, one run more
    ("x_follows", F6 + b"A" * 6 + b"AAA" + b"T" + TAIL9, F6 + b"A" * 6 + b"G" + TAIL9, "12=3D1X9=", "6=3D6=1X9="),
    # 2I3D side by side move together
    ("i_d_adjacent", F6 + b"A" * 9 + TAIL10, F6 + b"A" * 8 + TAIL10, "12=2I3D10=", "6=2I3D16="),
    # two D gaps in one homopolymer: exactly one M base stays between them
    ("two_d", F6 + b"A" * 14 + TAIL9, F6 + b"A" * 9 + TAIL9, "10=2D5=3D9=", "6=2D1=3D17="),
    # the M run before the gap is the CIGAR's first run: it keeps one base
    ("first_m", b"A" * 10 + TAIL10, b"A" * 7 + TAIL10, "7=3D10=", "1=3D16="),
    # a gap as first run and a gap as last run are not touched
    ("end_gaps", b"AAA" + b"AAAACGTTGCGTCCATG", b"AAAACGTTGCGTCCATG" + b"TG", "3D17=2I", "3D17=2I"),
    # four gaps linked through short M runs in one homopolymer: gaps 2 - 4 move only because their left neighbour moved
    ("chain4", F6 + b"A" * 23 + TAIL9, F6 + b"A" * 22 + TAIL9, "20=1D2=1I2=2D2=1I9=", "6=1D1I2D1I29="),
    # N equals N
    ("n_stretch", F6 + b"N" * 50 + TAIL10, F6 + b"N" * 46 + TAIL10, "52=4D10=", "6=4D56="),
]

# a homopolymer of 70 000 bases with a 5-base deletion at its right end: the extension passes the lane path's threshold and the wave
# path's 1024-byte steps and ends at index 1 (one base before the repeat; the first run keeps one base either way) or at index 0
LONG = [
    ("hp70k_offset1", b"C" + b"A" * 70000 + TAIL10, b"C" + b"A" * 69995 + TAIL10, "69996=5D10=", "1=5D70005="),
    ("hp70k_offset0", b"A" * 70000 + TAIL10, b"A" * 69995 + TAIL10, "69995=5D10=", "1=5D70004="),
]
