"""CPU: the contract of the guided search (tools/guided_model.py) on hand-made inputs.  The camera is the identity with fx = fy = 1,
cx = cy = 0 and every point lies at Z = 1, so that u = X and v = Y exactly and every edge case below is exact."""
import numpy as np
import pytest

from tools import guided_model as gm

K4 = (1.0, 1.0, 0.0, 0.0)
T_ID = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0)
ROWS, COLS = 200, 320


def bits(n):
    """a descriptor with the first n bits set"""
    d = np.zeros(256, np.uint8)
    d[:n] = 1
    return np.packbits(d)


def run(points, feats, descs, db=None, taken=None, radius=10.0, max_distance=50, ratio_pct=90, T=T_ID, K=K4):
    """points: [(x, y, z, kf, cls)]; feats: [(x, y)]; descs: [(class, bits set)].  Keyframe 7 holds class c as bits(0) unless db is given"""
    if db is None:
        db = {7: (np.stack([bits(0)] * 4), np.arange(4, dtype=np.int32))}
    p = np.array(points, np.float64).reshape(-1, 5)
    return gm.search_by_projection(db, K, T, ROWS, COLS, np.array(feats, np.float32).reshape(-1, 2), taken,
                                   np.stack([bits(n) for _, n in descs]) if descs else np.zeros((0, 32), np.uint8),
                                   np.array([c for c, _ in descs], np.int32), p[:, 3].astype(np.int64), p[:, 4].astype(np.int32), p[:, :3], radius,
                                   max_distance, ratio_pct)


def test_every_status_is_reached():
    db = {7: (np.stack([bits(0), bits(0), bits(0)]), np.array([0, 1, 2], np.int32)), 9: None}
    feats = [(50, 50), (52, 50), (150, 150), (100, 20), (100, 20.5)]
    descs = [(0, 3), (1, 40), (2, 60), (3, 10), (4, 10)]
    points = [(50, 50, 1, 7, 0),      # MATCHED: feature 0 at 3, second at 40
              (50, 50, -1, 7, 0),     # BEHIND
              (400, 50, 1, 7, 0),     # OUTSIDE
              (50, 50, 1, 9, 0),      # NO_DESCRIPTOR: stored without descriptors
              (50, 50, 1, 8, 0),      # NO_DESCRIPTOR: not stored
              (50, 50, 1, 7, 5),      # NO_DESCRIPTOR: no descriptor of that class
              (250, 100, 1, 7, 0),    # NO_FEATURE
              (150, 150, 1, 7, 1),    # DISTANCE: 60 > 50
              (100, 20, 1, 7, 1),     # RATIO: 10 against 10
              (51, 50, 1, 7, 2)]      # CLAIMED: feature 0 at 3 as well, the lower point wins
    r = run(points, feats, descs, db=db)
    assert r["status"].tolist() == [gm.MATCHED, gm.BEHIND, gm.OUTSIDE, gm.NO_DESCRIPTOR, gm.NO_DESCRIPTOR, gm.NO_DESCRIPTOR, gm.NO_FEATURE, gm.DISTANCE,
                                    gm.RATIO, gm.CLAIMED]
    assert r["feat"].tolist() == [0] + [-1] * 9 and r["n_matched"] == 1
    assert r["d1"].tolist() == [3, -1, -1, -1, -1, -1, -1, 60, 10, 3] and r["d2"].tolist() == [40, -1, -1, -1, -1, -1, -1, -1, 10, 40]
    assert r["uv"][1].tolist() == [0.0, 0.0] and r["uv"][2].tolist() == [400.0, 50.0] and r["uv"][0].tolist() == [50.0, 50.0]
    assert set(r["status"].tolist()) == set(range(8))


def test_the_window_edge_is_inclusive():
    feats = [(60, 50), (50, 60.5)]
    descs = [(0, 1), (1, 1)]
    r = run([(50, 50, 1, 7, 0)], feats, descs, radius=10.0)
    assert r["status"].tolist() == [gm.MATCHED] and r["feat"].tolist() == [0] and r["d2"].tolist() == [-1]      # |60 - 50| == radius is inside, 10.5 is not
    assert run([(50, 50, 1, 7, 0)], feats, descs, radius=9.999)["status"].tolist() == [gm.NO_FEATURE]
    assert run([(50, 50, 1, 7, 0)], feats, descs, radius=10.5)["d2"].tolist() == [1]
    assert run([(60, 50, 1, 7, 0)], feats, descs, radius=0.0)["feat"].tolist() == [0]                          # a window of one pixel position


def test_the_image_borders():
    feats = [(0, 0), (COLS - 1, ROWS - 1)]
    descs = [(0, 0), (1, 0)]
    pts = [(0, 0, 1, 7, 0), (COLS, 5, 1, 7, 0), (5, ROWS, 1, 7, 0), (-0.25, 5, 1, 7, 0), (5, -0.25, 1, 7, 0), (COLS - 0.5, ROWS - 0.5, 1, 7, 0)]
    r = run(pts, feats, descs, radius=2.0)
    assert r["status"].tolist() == [gm.MATCHED, gm.OUTSIDE, gm.OUTSIDE, gm.OUTSIDE, gm.OUTSIDE, gm.MATCHED]    # u == 0 inside, u == cols outside
    assert r["feat"].tolist() == [0, -1, -1, -1, -1, 1]


def test_behind_and_non_finite():
    r = run([(1, 1, 0, 7, 0), (1, 1, -2, 7, 0), (1e308, 1, 1, 7, 0)], [(1, 1)], [(0, 0)], T=(10.0, 10.0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0))
    assert r["status"].tolist() == [gm.BEHIND] * 3 and not r["uv"].any()                                       # zc == 0, zc < 0, xc overflows


def test_max_distance_is_inclusive():
    r = run([(50, 50, 1, 7, 0)], [(50, 50)], [(0, 50)], max_distance=50)
    assert r["status"].tolist() == [gm.MATCHED] and r["d1"].tolist() == [50]
    r = run([(50, 50, 1, 7, 0)], [(50, 50)], [(0, 51)], max_distance=50)
    assert r["status"].tolist() == [gm.DISTANCE] and r["d1"].tolist() == [51] and r["feat"].tolist() == [-1]


def test_the_ratio_is_strict():
    feats, pts = [(50, 50), (51, 50)], [(50, 50, 1, 7, 0)]
    assert run(pts, feats, [(0, 9), (1, 10)], ratio_pct=90)["status"].tolist() == [gm.RATIO]                   # 100 * 9 == 90 * 10
    assert run(pts, feats, [(0, 9), (1, 11)], ratio_pct=90)["status"].tolist() == [gm.MATCHED]                 # 900 < 990
    assert run(pts, feats, [(0, 0), (1, 0)], ratio_pct=100)["status"].tolist() == [gm.RATIO]                   # 0 < 0 fails
    assert run(pts, feats, [(0, 0), (1, 1)], ratio_pct=100)["status"].tolist() == [gm.MATCHED]
    assert run(pts, feats, [(0, 0), (1, 200)], ratio_pct=0)["status"].tolist() == [gm.RATIO]                   # ratio 0 accepts nothing that has a second
    assert run(pts, feats[:1], [(0, 5)], ratio_pct=0)["status"].tolist() == [gm.MATCHED]                       # ... and everything that has none


def test_the_distance_is_the_least_over_all_replicas():
    db = {7: (np.stack([bits(100), bits(30), bits(200)]), np.array([0, 0, 1], np.int32))}
    r = run([(50, 50, 1, 7, 0)], [(50, 50), (51, 50)], [(0, 90), (0, 33), (1, 120), (1, 60)], db=db, max_distance=256, ratio_pct=100)
    assert r["d1"].tolist() == [3] and r["d2"].tolist() == [20] and r["feat"].tolist() == [0]                  # |30 - 33|, |100 - 120|


def test_best_feature_ties_go_to_the_lower_index():
    r = run([(50, 50, 1, 7, 0)], [(52, 50), (50, 50), (51, 50)], [(2, 4), (1, 4), (0, 9)], ratio_pct=100, max_distance=50)
    assert r["d1"].tolist() == [4] and r["d2"].tolist() == [4] and r["status"].tolist() == [gm.RATIO]          # the second is the OTHER feature at 4
    r = run([(50, 50, 1, 7, 0)], [(52, 50), (50, 50)], [(1, 0), (0, 0)], ratio_pct=100)
    assert r["status"].tolist() == [gm.RATIO]
    # a tie that is accepted needs no second in the window: two points, each alone with its feature
    db = {7: (np.stack([bits(4), bits(4)]), np.array([0, 1], np.int32))}
    r = run([(50, 50, 1, 7, 0)], [(50, 50), (50, 50)], [(1, 4), (0, 4), (1, 200)], db=db, taken=np.array([0, 0], np.uint8), ratio_pct=100, max_distance=256)
    assert r["d1"].tolist() == [0] and r["d2"].tolist() == [0] and r["status"].tolist() == [gm.RATIO]
    r = run([(50, 50, 1, 7, 0)], [(50, 50), (50, 50)], [(1, 4), (0, 4)], db=db, taken=np.array([1, 0], np.uint8))
    assert r["feat"].tolist() == [1] and r["d2"].tolist() == [-1]                                              # a taken feature is no candidate, not even as a second


def test_claim_ties_go_to_the_lower_point():
    db = {7: (np.stack([bits(3), bits(3), bits(1)]), np.array([0, 1, 2], np.int32))}
    pts = [(50, 50, 1, 7, 0), (51, 50, 1, 7, 1), (49, 50, 1, 7, 2)]
    r = run(pts, [(50, 50), (150, 150)], [(0, 0)], db=db)
    assert r["d1"].tolist() == [3, 3, 1] and r["status"].tolist() == [gm.CLAIMED, gm.CLAIMED, gm.MATCHED] and r["feat"].tolist() == [-1, -1, 0]
    r = run(pts[:2], [(50, 50), (150, 150)], [(0, 0)], db=db)
    assert r["status"].tolist() == [gm.MATCHED, gm.CLAIMED] and r["n_matched"] == 1                            # equal d1: the lower point
    # the loser does not fall back to its second
    r = run(pts[:2], [(50, 50), (52, 50)], [(0, 0), (1, 200)], db=db, max_distance=256)
    assert r["status"].tolist() == [gm.MATCHED, gm.CLAIMED] and r["feat"].tolist() == [0, -1]


def test_empty_sides():
    assert run([], [(1, 1)], [(0, 0)])["n_matched"] == 0
    r = run([(50, 50, 1, 7, 0), (50, 50, -1, 7, 0), (-1, 0, 1, 7, 0)], [], [])
    assert r["status"].tolist() == [gm.NO_FEATURE, gm.BEHIND, gm.OUTSIDE] and r["n_matched"] == 0
    r = run([(50, 50, 1, 7, 0)], [(50, 50)], [])                                                               # a feature without descriptors is no candidate
    assert r["status"].tolist() == [gm.NO_FEATURE]


def test_the_arguments_are_checked():
    for kw in (dict(radius=-1.0), dict(radius=float("nan")), dict(max_distance=257), dict(max_distance=-1), dict(ratio_pct=101), dict(ratio_pct=-1)):
        with pytest.raises(ValueError):
            run([(50, 50, 1, 7, 0)], [(50, 50)], [(0, 0)], **kw)
    with pytest.raises(ValueError):
        run([(50, 50, 1, 7, 0)], [(50, 50)], [(1, 0)])


def test_the_projection_rounds_every_operation_on_its_own():
    T = (0.36, 0.48, -0.8, 0.1, -0.8, 0.6, 0.0, -0.2, 0.48, 0.64, 0.6, 0.3)
    K = (458.654, 457.296, 367.215, 248.375)
    xyz = np.array([[0.3, -0.7, 5.1], [1e-3, 2e-3, 0.9]])
    behind, uv = gm.project(K, T, xyz)
    for p in range(2):
        X, Y, Z = (float(x) for x in xyz[p])
        c = [((T[4 * r] * X + T[4 * r + 1] * Y) + T[4 * r + 2] * Z) + T[4 * r + 3] for r in range(3)]         # python floats: one rounding each
        assert not behind[p] and uv[p, 0] == K[0] * (c[0] / c[2]) + K[2] and uv[p, 1] == K[1] * (c[1] / c[2]) + K[3]


def test_refine_accept():
    assert gm.refine_accept(30, 30) and gm.refine_accept(30, 45) and not gm.refine_accept(30, 29)
    assert not gm.refine_accept(30, 45, found=False) and gm.refine_accept(0, 0, found=True)


def test_gather_points():
    A = lambda pid: (pid, True, False)
    feats = {1: [A(10), None, A(11)],
             3: [A(11), A(12), (13, False, False), (14, True, True), None, A(15)],
             5: [A(12), A(16)],
             8: [A(17), A(10)],
             9: [A(18)]}
    ids = [1, 3, 5, 8, 9]
    # the accepted keyframe first, then 3 and 8 (distance 1, the lower id first), then 1 and 9
    assert gm.gather_points(ids, 5, 2, feats, first_points=[16]) == [(12, 5, 0), (11, 3, 0), (15, 3, 5), (17, 8, 0), (10, 8, 1), (18, 9, 0)]
    assert gm.gather_points(ids, 5, 0, feats, first_points=[]) == [(12, 5, 0), (16, 5, 1)]
    assert gm.gather_points(ids, 1, 1, feats, first_points=[]) == [(10, 1, 0), (11, 1, 2), (12, 3, 1), (15, 3, 5)]                  # no keyframe before the first
    assert gm.gather_points(ids, 9, 2, feats, first_points=[10, 17]) == [(18, 9, 0), (12, 5, 0), (16, 5, 1)]    # 8 has nothing left
