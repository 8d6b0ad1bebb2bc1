"""The contract of relocalisation, in plain numpy (the style of tools/pnp_model.py): which stored keyframes a lost frame is matched
against (ssx_kfdb_relocalize_query, csrc/loop.hip: k_kfdb_topk) and which of their poses is accepted (LoopClosing::Relocalize).

select_candidates  Every stored keyframe has a double L1 score against the frame's BowVector (ssx_kfdb_detect_loop's scores).  The rule
                   works on the scores NARROWED TO FLOAT, as DetectLoop's comparison does (loopclosing.cpp:85):
                     f = float(score);  f_best = max f
                     candidate  <=>  f > 0  and  f >= threshold  and  f >= float(ratio) * f_best      (a float multiply)
                   ordered by f descending, then by row ascending (rows are in id order: the lower id first), cut to K.  This is the
                   descending order of the key k_kfdb_score builds, (float bits << 32) | ~row: floats > 0 order like their bit patterns.
                   The head of the list is therefore the winner of ssx_kfdb_detect_loop(min_id_gap = 0, threshold).
accept             Each candidate that had enough map points got a pose (ssx_pnp_pose_batch) with a number of refined inliers.  The
                   accepted candidate has the most, the lower rank winning a tie, and must have MORE than min_inliers."""
import numpy as np

MAX_CANDIDATES = 8      # SSX_RELOC_MAX_CANDIDATES


def select_candidates(scores_f64, ids, K, threshold, ratio):
    """-> (rows int32 [m], ids int64 [m], f float32 [m]), m <= K: the candidates in order"""
    if not 1 <= int(K) <= MAX_CANDIDATES:
        raise ValueError("K outside [1, %d]" % MAX_CANDIDATES)
    ratio32, thr32 = np.float32(ratio), np.float32(threshold)
    if not (np.isfinite(ratio32) and 0 <= ratio32 <= 1) or not thr32 >= 0:
        raise ValueError("ratio outside [0, 1] or a negative / NaN threshold")
    scores = np.ascontiguousarray(scores_f64, dtype=np.float64).reshape(-1)
    ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
    if len(ids) != len(scores):
        raise ValueError("one id per score")
    f = scores.astype(np.float32)
    if len(f) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.float32)
    f_best = f.max()
    bar = ratio32 * f_best                                      # float32 * float32 -> float32
    rows = np.nonzero((f > 0) & (f >= thr32) & (f >= bar))[0]
    order = np.lexsort((rows, -f[rows].astype(np.float64)))     # f descending, then row ascending (negating a float is exact)
    rows = rows[order][:int(K)].astype(np.int32)
    return rows, ids[rows], f[rows]


def accept(results, min_inliers):
    """results[rank] = refined inliers of the candidate of that rank, or None where it was skipped (too few map points) or no pose was
    found -> the accepted rank, or -1"""
    best, best_n = -1, int(min_inliers)
    for rank, n in enumerate(results):
        if n is not None and int(n) > best_n:                   # `>`: the bar is exclusive, and a tie keeps the lower rank
            best, best_n = rank, int(n)
    return best
