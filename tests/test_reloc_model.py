"""CPU: tools/reloc_model.py (the candidate rule of ssx_kfdb_relocalize_query and the acceptance rule of LoopClosing::Relocalize) held
to cases worked out by hand."""
import numpy as np
import pytest

from tools.reloc_model import accept, select_candidates


def sel(scores, K, threshold, ratio, ids=None):
    ids = np.arange(len(scores)) * 2 + 1 if ids is None else ids          # ids 1, 3, 5, ...: an id is not its row
    rows, kf, f = select_candidates(np.array(scores, np.float64), ids, K, threshold, ratio)
    assert rows.dtype == np.int32 and kf.dtype == np.int64 and f.dtype == np.float32
    assert list(kf) == [int(ids[r]) for r in rows]
    return list(rows), [float(x) for x in f]


def test_order_threshold_and_ratio():
    s = [0.10, 0.50, 0.30, 0.40, 0.05]
    assert sel(s, 8, 0.0, 0.0)[0] == [1, 3, 2, 0, 4]                      # descending score
    assert sel(s, 3, 0.0, 0.0)[0] == [1, 3, 2]                            # cut to K
    assert sel(s, 1, 0.0, 0.0)[0] == [1]
    assert sel(s, 8, 0.25, 0.0)[0] == [1, 3, 2]                           # f >= threshold
    assert sel(s, 8, 0.0, 0.75)[0] == [1, 3]                              # f >= 0.75 * 0.5 = 0.375
    assert sel(s, 8, 0.45, 0.5)[0] == [1]                                 # both screens
    assert sel(s, 8, 0.6, 0.0)[0] == []                                   # a threshold above the best empties the set
    rows, f = sel(s, 2, 0.0, 0.0)
    assert f == [float(np.float32(0.5)), float(np.float32(0.4))]          # the scores come back as floats


def test_a_threshold_or_a_ratio_that_is_met_exactly_keeps_the_row():
    assert sel([0.25, 0.5], 8, 0.25, 0.5)[0] == [1, 0]                    # 0.25 >= 0.25 and 0.25 >= 0.5 * 0.5, all exact in float


def test_ties_inside_the_set_come_in_row_order():
    s = [0.2, 0.7, 0.7, 0.1, 0.7]
    assert sel(s, 8, 0.0, 0.0)[0] == [1, 2, 4, 0, 3]
    assert sel(s, 8, 0.0, 1.0)[0] == [1, 2, 4]


def test_a_tie_straddling_rank_K_keeps_the_lower_rows():
    s = [0.3, 0.9, 0.3, 0.3, 0.3]
    assert sel(s, 3, 0.0, 0.0)[0] == [1, 0, 2]
    assert sel(s, 2, 0.0, 0.0)[0] == [1, 0]
    assert sel([0.4, 0.4, 0.4], 1, 0.0, 0.0)[0] == [0]


def test_all_scores_zero_or_negative_or_none_at_all():
    assert sel([0.0, 0.0, 0.0], 4, 0.0, 0.0)[0] == []                     # f > 0 is required: ratio * 0 = 0 would admit everything
    assert sel([0.0, -0.0, -1e-3], 4, 0.0, 0.0)[0] == []
    assert sel([], 4, 0.0, 0.5)[0] == []


def test_ratio_zero_and_ratio_one():
    s = [1e-6, 0.8, 0.0, 0.2]
    assert sel(s, 8, 0.0, 0.0)[0] == [1, 3, 0]                            # ratio 0: every positive score
    assert sel(s, 8, 0.0, 1.0)[0] == [1]                                  # ratio 1: the best alone (and its ties)


def test_two_doubles_that_narrow_to_one_float_tie():
    a, b = 0.5, 0.5 + 1e-12
    assert a != b and np.float32(a) == np.float32(b)
    # as doubles row 1 is the larger; as floats they tie, and row 0 comes first
    assert sel([a, b, 0.1], 8, 0.0, 0.0)[0] == [0, 1, 2]
    assert sel([a, b, 0.1], 1, 0.0, 0.0)[0] == [0]
    assert sel([a, b, 0.1], 8, 0.0, 1.0)[0] == [0, 1]                     # the smaller double passes ratio 1: the rule is on floats
    # a double just below a float boundary rounds up to it: the threshold is compared with the float
    c = 0.75 - 1e-12
    assert c < 0.75 and np.float32(c) == np.float32(0.75)
    assert sel([c], 8, 0.75, 0.0)[0] == [0]


def test_the_ratio_bar_is_a_float_product():
    best, ratio = np.float32(0.3), np.float32(0.7)
    bar = ratio * best
    assert bar.dtype == np.float32 and float(bar) != float(ratio) * float(best)     # the double product differs: the case tells them apart
    below = np.nextafter(bar, np.float32(0))
    assert sel([float(best), float(bar), float(below)], 8, 0.0, float(ratio))[0] == [0, 1]


def test_misuse():
    for K, thr, ratio in ((0, 0.0, 0.5), (9, 0.0, 0.5), (4, -0.1, 0.5), (4, float("nan"), 0.5), (4, 0.0, 1.5), (4, 0.0, -0.1), (4, 0.0, float("nan")),
                          (4, 0.0, float("inf"))):
        with pytest.raises(ValueError):
            select_candidates(np.array([0.5]), np.array([1]), K, thr, ratio)
    with pytest.raises(ValueError):
        select_candidates(np.array([0.5, 0.2]), np.array([1]), 4, 0.0, 0.5)


def test_accept():
    assert accept([30, 45, 12], 20) == 1                                  # the most refined inliers
    assert accept([45, 45, 12], 20) == 0                                  # a tie: the lower rank
    assert accept([None, 45, 45], 20) == 1                                # a skipped candidate never wins
    assert accept([20, 19], 20) == -1                                     # MORE than the bar
    assert accept([21, 19], 20) == 0
    assert accept([], 20) == -1
    assert accept([None, None], 0) == -1
    assert accept([0, 0], 0) == -1
