"""Hand-spelled cases of the net across records, with the pieces written out: what tests/test_chain_net_cpu.py holds tests/net_model.py
against and tests/test_chain_net_gpu.py the device.  A problem is (order, score, base, [(op, length)]); a piece (order, t, q, size)."""
from tests.net_model import OP_D, OP_I, OP_M, OP_X, SCORE_EQ

# name, n_bases, problems, the pieces sorted by (order, t), per record in order (score as used, pieces, bases won, bases aligned)
HAND = [
    ("higher_score_wins", 200,
     [(0, 10, 100, [(OP_M, 50)]), (1, 20, 120, [(OP_M, 10)])],
     [(0, 100, 0, 20), (0, 130, 30, 20), (1, 120, 0, 10)],
     [(10, 2, 40, 50), (20, 1, 10, 10)]),
    ("equal_scores_smaller_order_wins", 64,
     [(5, 7, 0, [(OP_M, 30)]), (2, 7, 10, [(OP_M, 30)])],
     [(2, 10, 0, 30), (5, 0, 0, 10)],
     [(7, 1, 30, 30), (7, 1, 10, 30)]),
    ("low_record_cut_into_three", 128,
     [(0, 1, 0, [(OP_M, 100)]), (1, 5, 20, [(OP_M, 10)]), (2, 9, 60, [(OP_X, 15)])],
     [(0, 0, 0, 20), (0, 30, 30, 30), (0, 75, 75, 25), (1, 20, 0, 10), (2, 60, 0, 15)],
     [(1, 3, 75, 100), (5, 1, 10, 10), (9, 1, 15, 15)]),
    ("gap_of_the_high_record_filled_by_the_low", 40,
     [(0, 50, 0, [(OP_M, 10), (OP_D, 5), (OP_M, 10)]), (1, 3, 5, [(OP_I, 4), (OP_M, 20)])],
     [(0, 0, 0, 10), (0, 15, 10, 10), (1, 10, 9, 5)],
     [(50, 2, 20, 20), (3, 1, 5, 20)]),
    ("abutting_blocks_of_two_records", 20,
     [(0, 5, 0, [(OP_M, 10)]), (1, 5, 10, [(OP_M, 10)])],
     [(0, 0, 0, 10), (1, 10, 0, 10)],
     [(5, 1, 10, 10), (5, 1, 10, 10)]),
    ("identical_intervals", 30,
     [(3, 4, 7, [(OP_M, 9)]), (1, 4, 7, [(OP_M, 9)]), (2, 6, 7, [(OP_X, 9)])],
     [(2, 7, 0, 9)],
     [(4, 0, 0, 9), (6, 1, 9, 9), (4, 0, 0, 9)]),
    ("score_is_the_equal_columns", 64,
     # 3=2X4= has 7 = columns, 8= has 8: the second wins where both lie, and the insertion moves q alone
     [(0, SCORE_EQ, 10, [(OP_M, 3), (OP_X, 2), (OP_M, 4)]), (1, SCORE_EQ, 15, [(OP_M, 2), (OP_I, 3), (OP_M, 6)])],
     [(0, 10, 0, 5), (1, 15, 0, 2), (1, 17, 5, 6)],
     [(7, 1, 5, 9), (8, 2, 8, 8)]),
    ("gap_runs_only_is_a_record_without_blocks", 32,
     [(0, 9, 4, [(OP_D, 5), (OP_I, 2)]), (1, 2, 4, [(OP_M, 5)])],
     [(1, 4, 0, 5)],
     [(9, 0, 0, 0), (2, 1, 5, 5)]),
]
