"""GPU: the guided search of relocalisation (ssx_kfdb_project_match / ssx_kfdb_guided_search: k_kfdb_project, k_kfdb_claim) against
its contract tools/guided_model.py.  Everything is integer arithmetic or f64 with every operation rounded on its own: every output
array is compared on bytes, uv included.

The database is crafted with ssx_kfdb_add: keyframe 4 with random descriptors whose classes have 0, 1, 8, 20 and 70 replicas spread
over its 64-entry chunks (70: more than a wavefront holds at once), keyframe 9 stored without descriptors, keyframe 15 with one
descriptor of 1 to 7 set bits per class, so that many points are equally far from an all-zero frame descriptor."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import loop as sloop
from ssvio_amd import orb as sorb
from ssvio_amd import voc as svoc
from ssvio_amd._lib import KP_DTYPE, dbl_p, i32_p, u8_p
from tools import guided_model as gm
from tools.synth import make_stereo_pair, make_vocabulary

pytestmark = pytest.mark.gpu

ROWS, COLS = 200, 320
LEVELS = 8
K_ID, T_ID = (1.0, 1.0, 0.0, 0.0), (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0)
K_CAM = (310.5, 309.25, 158.75, 101.5)
BOW = (np.array([1], np.int32), np.array([1.0]))
REPLICAS = {0: 1, 1: 8, 2: 20, 3: 70}                           # keyframe 4; class 5 has none
OUT_KEYS = ("feat", "d1", "d2", "status", "uv")


def bits(n):
    d = np.zeros(256, np.uint8)
    d[:n] = 1
    return np.packbits(d)


def rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


T_CAM = np.hstack([rot((0.3, -1.0, 0.2), 0.4), np.array([[0.4], [-0.2], [0.7]])]).reshape(-1)


@pytest.fixture(scope="module")
def store():
    """the stored keyframes as the model takes them (made once, never changed)"""
    rng = np.random.default_rng(5)
    cls4 = np.concatenate([np.full(n, c, np.int32) for c, n in REPLICAS.items()] + [np.repeat(np.arange(10, 40, dtype=np.int32), rng.integers(1, 9, 30))])
    cls4 = cls4[rng.permutation(len(cls4))]
    desc4 = rng.integers(0, 256, (len(cls4), 32), dtype=np.uint8)
    desc4[np.nonzero(cls4 == 0)[0][0]] = 0                      # class 0: one all-zero descriptor, so that a frame descriptor bits(n) is n away
    cls15 = np.arange(130, dtype=np.int32)
    desc15 = np.stack([bits(c % 7 + 1) for c in cls15])
    assert len(cls4) > 192 and all((cls4 == c).sum() == n for c, n in REPLICAS.items()) and not (cls4 == 5).any()
    return {4: (desc4, cls4), 9: None, 15: (desc15, cls15)}


@pytest.fixture(scope="module")
def db(ctx, store):
    d = sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    for kf_id, entry in store.items():
        d.add(kf_id, BOW, *(entry if entry is not None else ()))
    assert d.size() == (3, 3, sum(len(e[1]) for e in store.values() if e is not None))
    yield d
    d.close()


def both(db, store, K4, T, feat_xy, cur_desc, cur_cls, point_kf, point_cls, xyz, taken=None, **kw):
    """-> (the library's result, the model's), after comparing every byte"""
    got = db.project_match(K4, T, ROWS, COLS, feat_xy, cur_desc, cur_cls, point_kf, point_cls, xyz, taken=taken, **kw)
    want = gm.search_by_projection(store, K4, T, ROWS, COLS, feat_xy, taken, cur_desc, cur_cls, point_kf, point_cls, xyz, kw.get("radius", 10.0),
                                   kw.get("max_distance", 50), kw.get("ratio_pct", 90))
    for key in OUT_KEYS:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert got[key].tobytes() == want[key].tobytes(), (key, got[key][:16], want[key][:16])
    assert got["n_matched"] == want["n_matched"] == int((want["status"] == gm.MATCHED).sum())
    return got, want


def lists(points, feats, descs):
    """the hand-made form of tests/test_guided_model.py: points [(x, y, z, kf, cls)], feats [(x, y)], descs [(class, bits set)]"""
    p = np.array(points, np.float64).reshape(-1, 5)
    return dict(feat_xy=np.array(feats, np.float32).reshape(-1, 2), cur_desc=np.stack([bits(n) for _, n in descs]) if descs else np.zeros((0, 32), np.uint8),
                cur_cls=np.array([c for c, _ in descs], np.int32), point_kf=p[:, 3].astype(np.int64), point_cls=p[:, 4].astype(np.int32), xyz=p[:, :3])


def scenario(store, P, n_cur, seed):
    """P points that land near the features of a frame of n_cur descriptors, under T_CAM.  A feature's descriptors are noisy copies of
    stored descriptors of a point aimed at it, so that every verdict occurs."""
    rng = np.random.default_rng(seed)
    F = max((n_cur + 7) // 8, 1) if n_cur else 40
    feat_xy = np.stack([rng.uniform(0, COLS, F), rng.uniform(0, ROWS, F)], axis=1).astype(np.float32)
    feat_xy[: F // 3] = np.round(feat_xy[: F // 3])             # whole pixels too
    aim = rng.integers(0, F, P)
    uv = feat_xy[aim].astype(np.float64) + rng.choice([0.0, 3.0, 9.5, 10.0, 14.0], (P, 2)) * rng.choice([-1.0, 1.0], (P, 2))
    z = rng.uniform(0.5, 20.0, P) * rng.choice([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0], P)      # some behind the camera
    cam = np.stack([(uv[:, 0] - K_CAM[2]) / K_CAM[0] * z, (uv[:, 1] - K_CAM[3]) / K_CAM[1] * z, z], axis=1)
    R, t = T_CAM.reshape(3, 4)[:, :3], T_CAM.reshape(3, 4)[:, 3]
    xyz = (cam - t) @ R                                         # R^T (cam - t)
    point_kf = rng.choice([4, 15, 9, 99], P, p=[0.5, 0.4, 0.05, 0.05]).astype(np.int64)
    point_cls = np.where(point_kf == 15, rng.integers(0, 130, P), rng.choice([0, 1, 2, 3, 5, 12, 20, 33], P)).astype(np.int32)
    cur_cls = np.sort(rng.integers(0, F, n_cur)).astype(np.int32) if n_cur else np.zeros(0, np.int32)
    cur_desc = rng.integers(0, 256, (n_cur, 32), dtype=np.uint8)
    for j in range(n_cur):
        at = np.nonzero(aim == cur_cls[j])[0]
        if len(at) == 0 or rng.random() < 0.2:
            continue
        p = int(rng.choice(at))
        entry = store.get(int(point_kf[p]))
        mine = None if entry is None else entry[0][entry[1] == point_cls[p]]
        if mine is None or len(mine) == 0:
            continue
        src = np.unpackbits(mine[rng.integers(0, len(mine))])
        src ^= (rng.random(256) < rng.choice([0.0, 0.02, 0.1, 0.2])).astype(np.uint8)
        cur_desc[j] = np.packbits(src)
    taken = (rng.random(F) < 0.1).astype(np.uint8) if seed % 2 else None
    return dict(feat_xy=feat_xy, cur_desc=cur_desc, cur_cls=cur_cls, point_kf=point_kf, point_cls=point_cls, xyz=xyz, taken=taken)


@pytest.mark.parametrize("P", (0, 1, 63, 64, 65, 130))
@pytest.mark.parametrize("n_cur", (0, 1, 63, 64, 65, 4100))
def test_random_frames_against_the_model(db, store, P, n_cur):
    for seed in (P + n_cur, P + n_cur + 1):                     # taken null and set
        both(db, store, K_CAM, T_CAM, **scenario(store, P, n_cur, seed))


def test_every_verdict_occurs_in_the_largest_case(db, store):
    got, want = both(db, store, K_CAM, T_CAM, ratio_pct=80, **scenario(store, 130, 4100, 1))
    assert set(want["status"].tolist()) == set(range(8)), np.bincount(want["status"], minlength=8)
    assert got["n_matched"] >= 10


def test_all_points_claim_one_feature(db, store):
    """130 points of keyframe 15, one per class and hence 1 to 7 away from the all-zero descriptor of the one feature in reach: every
    point is accepted, the lowest distance wins and, of the 19 points that have it, the lowest point"""
    rng = np.random.default_rng(9)
    cls = rng.permutation(130).astype(np.int32)
    xy = np.stack([100.0 + rng.uniform(-9, 9, 130), 100.0 + rng.uniform(-9, 9, 130)], axis=1)
    got, _ = both(db, store, K_ID, T_ID, feat_xy=np.array([[100, 100], [250, 30], [20, 180]], np.float32), cur_desc=np.zeros((2, 32), np.uint8),
                  cur_cls=np.array([0, 1], np.int32), point_kf=np.full(130, 15, np.int64), point_cls=cls, xyz=np.concatenate([xy, np.ones((130, 1))], axis=1))
    win = int(np.nonzero(cls % 7 == 0)[0][0])
    assert (got["d1"] == cls % 7 + 1).all() and (got["d2"] == -1).all() and got["n_matched"] == 1
    assert got["status"][win] == gm.MATCHED and got["feat"][win] == 0 and (np.delete(got["status"], win) == gm.CLAIMED).all() and (np.delete(got["feat"], win) == -1).all()


def test_points_of_different_keyframes_interleaved_and_an_unknown_one(db, store):
    feats = [(30 + 25 * i, 60) for i in range(8)]
    descs = [(i, 2 + i) for i in range(8)]
    points = [(30, 60, 1, 4, 0), (55, 60, 1, 15, 0), (80, 60, 1, 4, 0), (105, 60, 1, 15, 8), (130, 60, 1, 99, 0), (155, 60, 1, 9, 0), (180, 60, 1, 4, 5), (205, 60, 1, 15, 129)]
    got, _ = both(db, store, K_ID, T_ID, **lists(points, feats, descs))
    S = gm
    assert got["status"].tolist() == [S.MATCHED, S.MATCHED, S.MATCHED, S.MATCHED, S.NO_DESCRIPTOR, S.NO_DESCRIPTOR, S.NO_DESCRIPTOR, S.MATCHED]
    assert got["d1"].tolist() == [2, 2, 4, 3, -1, -1, -1, 5]    # keyframe 15: |bits(c % 7 + 1) xor bits(n)|


def test_the_exact_edges(db, store):
    S = gm
    one = [(50, 50, 1, 4, 0)]
    # the window: |60 - 50| == radius is inside, 10.5 is not
    feats, descs = [(60, 50), (50, 60.5)], [(0, 1), (1, 1)]
    got, _ = both(db, store, K_ID, T_ID, **lists(one, feats, descs))
    assert got["status"].tolist() == [S.MATCHED] and got["feat"].tolist() == [0] and got["d2"].tolist() == [-1]
    assert both(db, store, K_ID, T_ID, radius=9.999, **lists(one, feats, descs))[0]["status"].tolist() == [S.NO_FEATURE]
    assert both(db, store, K_ID, T_ID, radius=10.5, **lists(one, feats, descs))[0]["d2"].tolist() == [1]
    assert both(db, store, K_ID, T_ID, radius=0.0, **lists([(60, 50, 1, 4, 0)], feats, descs))[0]["feat"].tolist() == [0]
    # the image borders: u == 0 is inside, u == cols outside; behind the camera
    pts = [(0, 0, 1, 4, 0), (COLS, 5, 1, 4, 0), (5, ROWS, 1, 4, 0), (-0.25, 5, 1, 4, 0), (5, -0.25, 1, 4, 0), (COLS - 0.5, ROWS - 0.5, 1, 15, 0), (0, ROWS - 0.5, 1, 15, 7),
           (COLS - 0.5, 0, 1, 15, 14), (5, 5, 0, 4, 0), (5, 5, -3, 4, 0), (1e308, 5, 1, 4, 0)]
    got, _ = both(db, store, K_ID, (10.0, 10.0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0), radius=2.0,
                  **lists(pts, [(0, 0), (COLS - 1, ROWS - 1), (1, ROWS - 1), (COLS - 1, 1)], [(0, 0), (1, 0), (2, 0), (3, 0)]))
    assert got["status"].tolist()[8:] == [S.BEHIND] * 3 and not got["uv"][8:].any()
    got, _ = both(db, store, K_ID, T_ID, radius=2.0, **lists(pts, [(0, 0), (COLS - 1, ROWS - 1), (1, ROWS - 1), (COLS - 1, 1)], [(0, 0), (1, 0), (2, 0), (3, 0)]))
    assert got["status"].tolist() == [S.MATCHED] + [S.OUTSIDE] * 4 + [S.MATCHED] * 3 + [S.BEHIND] * 2 + [S.OUTSIDE]
    assert got["feat"].tolist()[:8] == [0, -1, -1, -1, -1, 1, 2, 3]
    # the distance bar is inclusive, the ratio strict
    assert both(db, store, K_ID, T_ID, **lists(one, [(50, 50)], [(0, 50)]))[0]["status"].tolist() == [S.MATCHED]
    assert both(db, store, K_ID, T_ID, **lists(one, [(50, 50)], [(0, 51)]))[0]["status"].tolist() == [S.DISTANCE]
    two = [(50, 50), (51, 50)]
    assert both(db, store, K_ID, T_ID, **lists(one, two, [(0, 9), (1, 10)]))[0]["status"].tolist() == [S.RATIO]
    assert both(db, store, K_ID, T_ID, **lists(one, two, [(0, 9), (1, 11)]))[0]["status"].tolist() == [S.MATCHED]
    assert both(db, store, K_ID, T_ID, ratio_pct=100, **lists(one, two, [(0, 0), (1, 0)]))[0]["status"].tolist() == [S.RATIO]
    assert both(db, store, K_ID, T_ID, ratio_pct=0, **lists(one, two[:1], [(0, 5)]))[0]["status"].tolist() == [S.MATCHED]
    # ties: the lower feature, the lower point; a taken feature is no candidate
    got, _ = both(db, store, K_ID, T_ID, ratio_pct=100, **lists(one, [(52, 50), (50, 50), (51, 50)], [(2, 4), (1, 4), (0, 9)]))
    assert got["d1"].tolist() == [4] and got["d2"].tolist() == [4] and got["status"].tolist() == [S.RATIO]
    got, _ = both(db, store, K_ID, T_ID, taken=np.array([0, 1, 0], np.uint8), **lists(one, [(52, 50), (50, 50), (51, 50)], [(2, 4), (1, 4), (0, 9)]))
    assert got["feat"].tolist() == [2] and got["d1"].tolist() == [4] and got["d2"].tolist() == [9]
    got, _ = both(db, store, K_ID, T_ID, **lists([(50, 50, 1, 15, 7), (51, 50, 1, 15, 0), (49, 50, 1, 15, 1)], [(50, 50), (150, 150)], [(0, 0)]))
    assert got["d1"].tolist() == [1, 1, 2] and got["status"].tolist() == [S.MATCHED, S.CLAIMED, S.CLAIMED] and got["feat"].tolist() == [0, -1, -1]
    # every replica counts on both sides: class 2 of keyframe 4 has 20 descriptors, class 3 has 70 (two batches)
    desc4, cls4 = store[4]
    for c in (1, 2, 3):
        mine = desc4[cls4 == c]
        for k in (0, len(mine) - 1):
            got, _ = both(db, store, K_ID, T_ID, max_distance=0, feat_xy=np.array([[50, 50]], np.float32), cur_desc=np.stack([bits(128), mine[k]]),
                          cur_cls=np.zeros(2, np.int32), point_kf=[4], point_cls=[c], xyz=[[50, 50, 1]])
            assert got["status"].tolist() == [S.MATCHED] and got["d1"].tolist() == [0]


def test_empty_sides(db, store):
    S = gm
    pts = [(50, 50, 1, 4, 0), (50, 50, -1, 4, 0), (-1, 0, 1, 4, 0), (50, 50, 1, 99, 0)]
    want = [S.NO_FEATURE, S.BEHIND, S.OUTSIDE, S.NO_DESCRIPTOR]
    assert both(db, store, K_ID, T_ID, **lists(pts, [], []))[0]["status"].tolist() == want                      # F == 0
    assert both(db, store, K_ID, T_ID, **lists(pts, [(50, 50)], []))[0]["status"].tolist() == want              # n_cur == 0
    assert both(db, store, K_ID, T_ID, taken=np.zeros(0, np.uint8), **lists(pts, [], []))[0]["n_matched"] == 0
    got, _ = both(db, store, K_ID, T_ID, **lists([], [(50, 50)], [(0, 0)]))                                     # P == 0
    assert got["n_matched"] == 0 and len(got["status"]) == 0


# ---- the refusals: raw calls, so that null pointers and untouched outputs can be stated ------------------------------------------------
def raw_args(P=2, F=2, n_cur=2):
    a = dict(K4=np.array(K_ID), T=np.array(T_ID, np.float64), rows=ROWS, cols=COLS, F=F, feat_xy=np.full((max(F, 1), 2), 50, np.float32),
             taken=np.zeros(max(F, 1), np.uint8), n_cur=n_cur, cur_desc=np.zeros((max(n_cur, 1), 32), np.uint8), cur_cls=np.zeros(max(n_cur, 1), np.int32), P=P,
             point_kf=np.full(max(P, 1), 4, np.int64), point_cls=np.zeros(max(P, 1), np.int32), xyz=np.tile([50.0, 50.0, 1.0], (max(P, 1), 1)), radius=10.0,
             max_distance=50, ratio_pct=90)
    for k in ("feat_out", "d1_out", "d2_out", "status_out"):
        a[k] = np.full(max(P, 1), 77, np.int32)
    a["uv_out"] = np.full((max(P, 1), 2), 77.0)
    a["n_matched"] = np.full(1, 77, np.int32)
    return a


OUTPUTS = ("feat_out", "d1_out", "d2_out", "status_out", "uv_out", "n_matched")


def p_(a, t):
    return None if a is None else a.ctypes.data_as(t)


def tail(a):
    return (a["P"], p_(a["point_kf"], sloop.i64_p), p_(a["point_cls"], i32_p), p_(a["xyz"], dbl_p), a["radius"], a["max_distance"], a["ratio_pct"], p_(a["feat_out"], i32_p),
            p_(a["d1_out"], i32_p), p_(a["d2_out"], i32_p), p_(a["status_out"], i32_p), p_(a["uv_out"], dbl_p), p_(a["n_matched"], i32_p))


def raw_project(db, a, handle=True):
    return db.ctx.lib.ssx_kfdb_project_match(db.handle if handle else None, p_(a["K4"], dbl_p), p_(a["T"], dbl_p), a["rows"], a["cols"], a["F"],
                                             p_(a["feat_xy"], C.POINTER(C.c_float)), p_(a["taken"], u8_p), a["n_cur"], p_(a["cur_desc"], u8_p), p_(a["cur_cls"], i32_p), *tail(a))


def untouched(a):
    return all(a[k] is None or (a[k] == 77).all() for k in OUTPUTS)


def nan_at(arr, i, v=float("nan")):
    out = np.array(arr, np.float64)
    out[i] = v
    return out


REFUSED = [("K4", None), ("T", None), ("n_matched", None), ("point_kf", None), ("point_cls", None), ("xyz", None), ("feat_out", None), ("d1_out", None),
           ("d2_out", None), ("status_out", None), ("feat_xy", None), ("cur_desc", None), ("cur_cls", None), ("P", -1), ("F", -1), ("n_cur", -1),
           ("cur_cls", np.array([0, 2], np.int32)), ("cur_cls", np.array([-1, 0], np.int32)), ("radius", -0.5), ("radius", float("nan")), ("radius", float("inf")),
           ("max_distance", -1), ("max_distance", 257), ("ratio_pct", -1), ("ratio_pct", 101), ("K4", nan_at(K_ID, 2)), ("K4", nan_at(K_ID, 0, float("inf"))),
           ("T", nan_at(T_ID, 11)), ("T", nan_at(T_ID, 0, float("-inf"))), ("rows", 0), ("cols", 0)]


def test_project_match_refusals_leave_the_outputs_untouched(db):
    before = db.size()
    for key, value in REFUSED:
        a = raw_args()
        a[key] = value
        assert raw_project(db, a) == -1, (key, value)           # SSX_ERR_INVALID_ARG
        assert untouched(a), (key, value)
    a = raw_args()
    assert raw_project(db, a, handle=False) == -1 and untouched(a)
    a = raw_args(P=65536)
    assert raw_project(db, a) == -5 and untouched(a)            # SSX_ERR_UNSUPPORTED
    a = raw_args(P=65535)
    a["uv_out"] = None                                          # nullable
    assert raw_project(db, a) == 0 and (a["status_out"] == gm.MATCHED).sum() == 1 and a["n_matched"][0] == 1 and (a["d1_out"] == 0).all()
    a = raw_args()
    assert raw_project(db, a) == 0 and a["status_out"].tolist() == [gm.MATCHED, gm.CLAIMED] and a["uv_out"].tolist() == [[50.0, 50.0]] * 2
    assert db.size() == before


# ---- ssx_kfdb_guided_search on an image ----------------------------------------------------------------------------------------------
def expand(features, levels=LEVELS):
    out = np.repeat(np.ascontiguousarray(features, dtype=KP_DTYPE), levels)
    out["octave"] = np.tile(np.arange(levels, dtype=np.int32), len(features))
    out["response"] = -1.0
    out["class_id"] = np.repeat(np.arange(len(features), dtype=np.int32), levels)
    return out


@pytest.fixture(scope="module")
def ex(ctx):
    return sorb.ORBextractor(ctx, nfeatures=2000)


@pytest.fixture(scope="module")
def frame(po, ex):
    """the frame and its descriptors and class ids, obtained as tests/test_reloc_query_gpu.py obtains them (computed once, never changed)"""
    img = make_stereo_pair(seed=140, h=ROWS, w=COLS, n_blobs=400)[0]
    feats = po.orb_detect(img, prm=po.orb_params(nfeatures=60))
    kps, desc = ex.ScreenAndComputeKPsParams_CalcDescriptors(img, expand(feats))
    cls = np.ascontiguousarray(kps["class_id"])
    assert 30 <= len(feats) <= 120 and len(desc) > 100
    return dict(img=img, feats=feats, desc=desc, cls=cls, feat_xy=np.stack([feats["x"], feats["y"]], axis=1).astype(np.float32))


@pytest.fixture(scope="module")
def fstore(frame):
    """keyframe 3: the frame's own descriptors with a few bits flipped, under the frame's class ids; keyframe 6 without descriptors"""
    rng = np.random.default_rng(21)
    noisy = np.unpackbits(frame["desc"], axis=1)
    noisy ^= (rng.random(noisy.shape) < 0.03).astype(np.uint8)
    return {3: (np.packbits(noisy, axis=1), frame["cls"].copy()), 6: None}


@pytest.fixture(scope="module")
def fdb(ctx, fstore, frame, ex):
    """that database, with the frame itself left PENDING as keyframe 20 by a keyframe step"""
    voc = make_vocabulary(k=10, L=3)
    V = svoc.Vocabulary.from_arrays(ctx, 10, 3, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    d = sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    d.add(3, BOW, *fstore[3])
    d.add(6, BOW)
    d.process_keyframe(V, 20, frame["img"], frame["feats"], ex.prm, threshold=0.5, pyramid_levels=LEVELS, min_db_size=100)
    yield d
    d.close(); V.close()


def frame_points(frame, P, seed=3):
    rng = np.random.default_rng(seed)
    F = len(frame["feats"])
    aim = rng.integers(0, F, P)
    uv = frame["feat_xy"][aim].astype(np.float64) + rng.uniform(-4, 4, (P, 2))
    z = rng.uniform(2.0, 30.0, P)
    cam = np.stack([(uv[:, 0] - K_CAM[2]) / K_CAM[0] * z, (uv[:, 1] - K_CAM[3]) / K_CAM[1] * z, z], axis=1)
    R, t = T_CAM.reshape(3, 4)[:, :3], T_CAM.reshape(3, 4)[:, 3]
    kf = np.where(rng.random(P) < 0.9, 3, 6).astype(np.int64)
    return dict(point_kf=kf, point_cls=aim.astype(np.int32), xyz=(cam - t) @ R)


def pending_bytes(d):
    pe = d.pending()
    return (pe["kf_id"], pe["keypoints"].tobytes(), pe["desc"].tobytes(), pe["class_id"].tobytes(), pe["bow"][0].tobytes(), pe["bow"][1].tobytes())


def test_guided_search_equals_project_match_on_the_frames_descriptors(fdb, fstore, frame, ex):
    before = (fdb.size(), pending_bytes(fdb), fdb.match_features(3, frame["desc"], frame["cls"])[0].tobytes())
    steps = {}
    for P, taken in ((130, None), (1, None), (130, (np.arange(len(frame["feats"])) % 5 == 0).astype(np.uint8)), (0, None)):
        pts = frame_points(frame, P)
        for radius in (10.0, 3.0):
            a = fdb.guided_search(frame["img"], frame["feats"], ex.prm, K_CAM, T_CAM, taken=taken, radius=radius, pyramid_levels=LEVELS, **pts)
            steps[P] = fdb.debug_last_step()
            b = fdb.guided_search(frame["img"], frame["feats"], ex.prm, K_CAM, T_CAM, taken=taken, radius=radius, pyramid_levels=LEVELS, **pts)
            c = fdb.project_match(K_CAM, T_CAM, ROWS, COLS, frame["feat_xy"], frame["desc"], frame["cls"], taken=taken, radius=radius, **pts)
            m = gm.search_by_projection(fstore, K_CAM, T_CAM, ROWS, COLS, frame["feat_xy"], taken, frame["desc"], frame["cls"], pts["point_kf"], pts["point_cls"],
                                        pts["xyz"], radius, 50, 90)
            for key in OUT_KEYS:
                assert a[key].tobytes() == b[key].tobytes() == c[key].tobytes() == m[key].tobytes(), (P, radius, key)
            assert a["n_matched"] == b["n_matched"] == c["n_matched"] == m["n_matched"]
            if P == 130 and radius == 10.0:
                assert a["n_matched"] >= 20 and (a["status"] == gm.CLAIMED).any() and (a["status"] == gm.NO_DESCRIPTOR).any(), np.bincount(a["status"], minlength=8)
    # the shape was planned by the keyframe step: ONE synchronisation, and neither number depends on P
    assert steps[1]["syncs"] == steps[130]["syncs"] == steps[0]["syncs"] == 1
    assert steps[1]["launches"] == steps[130]["launches"] == steps[0]["launches"] >= 4
    assert steps[130]["bytes_down"] > steps[1]["bytes_down"] > 0
    # the database is only read: the stored keyframes and the pending one are as before
    assert (fdb.size(), pending_bytes(fdb), fdb.match_features(3, frame["desc"], frame["cls"])[0].tobytes()) == before


def test_guided_search_without_features(fdb, frame, ex):
    pts = frame_points(frame, 5)
    r = fdb.guided_search(frame["img"], frame["feats"][:0], ex.prm, K_CAM, T_CAM, pyramid_levels=LEVELS, **pts)
    inside = (r["uv"][:, 0] >= 0) & (r["uv"][:, 0] < COLS) & (r["uv"][:, 1] >= 0) & (r["uv"][:, 1] < ROWS)
    assert r["n_matched"] == 0 and inside.any() and set(r["status"][inside].tolist()) <= {gm.NO_FEATURE, gm.NO_DESCRIPTOR}


def test_guided_search_refusals_leave_the_outputs_untouched(fdb, frame, ex):
    lib, img, feats = fdb.ctx.lib, frame["img"], np.ascontiguousarray(frame["feats"], dtype=KP_DTYPE)
    before = (fdb.size(), pending_bytes(fdb))

    def call(a, image=img, stride=None, rows=ROWS, cols=COLS, prm=ex.prm, n_features=len(feats), features=feats, levels=LEVELS, handle=True):
        return lib.ssx_kfdb_guided_search(fdb.handle if handle else None, p_(image, u8_p), image.strides[0] if stride is None and image is not None else (stride or 0),
                                          rows, cols, C.byref(prm) if prm is not None else None, n_features, None if features is None else features.ctypes.data_as(C.c_void_p),
                                          levels, p_(a["taken"], u8_p) if a["taken"] is not None and len(a["taken"]) == len(feats) else None, p_(a["K4"], dbl_p),
                                          p_(a["T"], dbl_p), *tail(a))

    for key, value in REFUSED:
        if key in ("feat_xy", "cur_desc", "cur_cls", "F", "n_cur", "rows", "cols"):
            continue                                            # (arguments of the stage form alone)
        a = raw_args()
        a[key] = value
        assert call(a) == -1 and untouched(a), (key, value)
    for kw in (dict(handle=False), dict(image=None), dict(prm=None), dict(stride=COLS - 1), dict(rows=0), dict(cols=0), dict(n_features=-1), dict(features=None),
               dict(levels=0), dict(levels=9)):
        a = raw_args()
        assert call(a, **kw) == -1 and untouched(a), kw
    a = raw_args()
    assert call(a, n_features=8192, features=np.zeros(8192, KP_DTYPE)) == -5 and untouched(a)                   # 65536 pyramid keypoints
    a = raw_args(P=65536)
    assert call(a) == -5 and untouched(a)
    a = raw_args()
    assert call(a) == 0 and not untouched(a)
    assert (fdb.size(), pending_bytes(fdb)) == before
