"""GPU parity of the per-keyframe step of loop closing (ssx_kfdb_process_keyframe / _add_pending / _pending: ProcessNewKeyframe,
DetectLoop, MatchFeatures and AddToKeyframeDatabase of src/ssvio/loopclosing.cpp:596-634, :72-103, :105-145, :646-649 as one call
with the keyframe left on the device) against the five calls it replaces: ssx_orb_describe_at, ssx_voc_transform,
ssx_kfdb_detect_loop, ssx_kfdb_match_features, ssx_kfdb_add.  Those are bit-exact against the CPU oracle (test_orb_gpu.py,
test_voc_gpu.py, test_loop_db_gpu.py), and everything here is integer or ordered-double arithmetic, so every comparison is on bytes."""
import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import loop as sloop
from ssvio_amd import orb as sorb
from ssvio_amd import voc as svoc
from ssvio_amd._lib import KP_DTYPE, SsxError
from tools.synth import make_stereo_pair, make_vocabulary

pytestmark = pytest.mark.gpu

LEVELS = 8
THRESHOLD = 0.6            # a revisit of the same image scores 1.0; different places of the synthetic scenes stay far below


def expand(features, levels=LEVELS):
    """pyramid keypoint i * levels + level = features[i] with octave = level, response = -1, class_id = i (loopclosing.cpp:607-619)"""
    out = np.repeat(np.ascontiguousarray(features, dtype=KP_DTYPE), levels)
    out["octave"] = np.tile(np.arange(levels, dtype=np.int32), len(features))
    out["response"] = -1.0
    out["class_id"] = np.repeat(np.arange(len(features), dtype=np.int32), levels)
    return out


def five_calls(db, V, ex, kf_id, img, features, min_db_size, min_id_gap, threshold=THRESHOLD, levels=LEVELS):
    """the step as a caller of the five existing entry points runs it -> (result in process_keyframe's form, the keyframe's arrays)"""
    kps, desc = ex.ScreenAndComputeKPsParams_CalcDescriptors(img, expand(features, levels))
    cls = np.ascontiguousarray(kps["class_id"])
    bow = V.transform(desc)
    r = dict(n_pyramid=len(kps), n_bow=len(bow[0]), detect_ran=len(db) > min_db_size, n_scored=0, found=False, score=None, loop_kf_id=None, n_pairs=0,
             min_distance=-1, pairs=np.zeros((0, 2), np.int32))
    if r["detect_ran"]:
        r["found"], r["loop_kf_id"], r["score"], r["n_scored"] = db.detect_loop(kf_id, bow, threshold, min_id_gap=min_id_gap)
        if r["found"]:
            r["pairs"], r["min_distance"] = db.match_features(r["loop_kf_id"], desc, cls)
            r["n_pairs"] = len(r["pairs"])
    return r, dict(kf_id=kf_id, keypoints=kps, desc=desc, class_id=cls, bow=bow)


def same_result(a, b):
    for key in ("n_pyramid", "n_bow", "detect_ran", "n_scored", "found", "loop_kf_id", "n_pairs", "min_distance"):
        assert a[key] == b[key], (key, a[key], b[key])
    assert (a["score"] is None) == (b["score"] is None)
    if a["score"] is not None:
        assert np.float32(a["score"]).tobytes() == np.float32(b["score"]).tobytes()
    assert a["pairs"].tobytes() == b["pairs"].tobytes() and a["pairs"].shape == b["pairs"].shape


def same_keyframe(kf, pend):
    assert pend["kf_id"] == kf["kf_id"]
    assert len(pend["keypoints"]) == len(kf["keypoints"]) and pend["keypoints"].tobytes() == kf["keypoints"].tobytes()
    assert pend["desc"].tobytes() == kf["desc"].tobytes()
    assert pend["class_id"].tobytes() == kf["class_id"].tobytes()
    assert pend["bow"][0].tobytes() == kf["bow"][0].tobytes() and pend["bow"][1].tobytes() == kf["bow"][1].tobytes()


def same_contents(A, B, query_id, query, min_id_gap=0):
    """the stored BowVectors are equal when a query scores the same doubles against every keyframe of both"""
    assert A.size() == B.size()
    a = A.detect_loop(query_id, query, 0.0, min_id_gap=min_id_gap, with_scores=True)
    b = B.detect_loop(query_id, query, 0.0, min_id_gap=min_id_gap, with_scores=True)
    assert a[:4] == b[:4] and a[4].tobytes() == b[4].tobytes() and len(a[4]) == len(A)


def small_scene(po, seed, nfeatures=150):
    img = make_stereo_pair(seed=100 + seed, h=200, w=320, n_blobs=400)[0]
    return img, po.orb_detect(img, prm=po.orb_params(nfeatures=nfeatures))


@pytest.fixture(scope="module")
def V(ctx):
    voc = make_vocabulary(k=10, L=3)
    v = svoc.Vocabulary.from_arrays(ctx, 10, 3, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    yield v
    v.close()


@pytest.fixture(scope="module")
def ex(ctx):
    return sorb.ORBextractor(ctx, nfeatures=2000)


@pytest.fixture(scope="module")
def drive(ctx, po, V, ex):
    """30 keyframes over 16 places, 14 of them revisits.  Database A by the five calls, database B by process_keyframe + add_pending; the
    commit is skipped when at least 10 pairs came back, as the reference skips it after a confirmed loop (loopclosing.cpp:57-66)."""
    places = list(range(6)) + [0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11, 0, 12, 6, 13, 7, 1, 14, 8, 9, 15, 2, 10]
    assert len(places) == 30
    scenes = {s: small_scene(po, s) for s in sorted(set(places))}
    A, B = sloop.KeyframeDatabase(ctx, keyframes_hint=4), sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    log = []
    for i, place in enumerate(places):
        img, feats = scenes[place]
        kf_id = 2 * i + 1
        ra, kf = five_calls(A, V, ex, kf_id, img, feats, min_db_size=2, min_id_gap=3)
        rb = B.process_keyframe(V, kf_id, img, feats, ex.prm, THRESHOLD, pyramid_levels=LEVELS, min_db_size=2, min_id_gap=3)
        stats = B.debug_last_step()
        pend = B.pending()
        if ra["n_pairs"] < 10:
            A.add(kf_id, kf["bow"], kf["desc"], kf["class_id"])
        if rb["n_pairs"] < 10:
            B.add_pending()
        log.append(dict(a=ra, b=rb, kf=kf, pend=pend, stats=stats, sizes=(A.size(), B.size())))
    yield A, B, log, scenes
    A.close()
    B.close()


def test_the_step_equals_the_five_calls(drive, V, ex):
    A, B, log, scenes = drive
    for i, e in enumerate(log):
        same_result(e["a"], e["b"])
        same_keyframe(e["kf"], e["pend"])
        assert e["sizes"][0] == e["sizes"][1], i
    assert any(e["b"]["found"] and e["b"]["n_pairs"] >= 10 for e in log)
    assert any(not e["b"]["found"] and e["b"]["detect_ran"] and e["b"]["n_scored"] > 0 for e in log)
    assert any(not e["b"]["detect_ran"] for e in log)
    assert 6 <= len(A) < 30 and log[0]["b"]["n_pyramid"] > 300 and log[0]["b"]["n_bow"] > 100
    same_contents(A, B, 1000, log[7]["kf"]["bow"])
    # the stored descriptors and class ids too: MatchFeatures against every stored keyframe
    cur = log[-1]["kf"]
    for e in log:
        if e["a"]["n_pairs"] < 10:
            pa, ma = A.match_features(e["kf"]["kf_id"], cur["desc"], cur["class_id"])
            pb, mb = B.match_features(e["kf"]["kf_id"], cur["desc"], cur["class_id"])
            assert ma == mb and pa.tobytes() == pb.tobytes()


def test_budget(drive):
    """one synchronisation and the header when no loop is found, two and 8 bytes per pair when one is (ssx_kfdb_debug_last_step)"""
    _, _, log, _ = drive
    for e in log:
        s, r = e["stats"], e["b"]
        assert s["bytes_up"] < 200 * 320 + 28 * LEVELS * 150 + 4 * 256, s      # the image and the keypoints, nothing else
        assert 0 < s["launches"] <= 20
        if r["found"] and r["n_pairs"] > 0:
            assert s["syncs"] == 2 and s["bytes_down"] <= 256 + 8 * len(r["pairs"]), s
        else:
            assert s["syncs"] == 1 and s["bytes_down"] <= 256, s


BOW_SIZES = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 9000)


@pytest.mark.parametrize("k,L,weighting", [(10, 3, 0), (7, 2, 1), (3, 5, 2), (20, 2, 3), (2, 1, 0), (2, 8, 0)])
def test_bow_assembly_at_the_sizes_where_it_can_break(ctx, po, k, L, weighting):
    """k_voc_words + k_kf_bow (ssx_kfdb_debug_bow) against ssx_voc_transform and the oracle's BowVector: around a wavefront's chunk of the
    norm chain (64), around the LDS sort (4096 keys), runs as long as the input (two words), stopped words."""
    rng = np.random.default_rng(100 * k + L)
    random = rng.integers(0, 256, (BOW_SIZES[-1], 32), dtype=np.uint8)
    tiled = np.tile(rng.integers(0, 256, (40, 32), dtype=np.uint8), (BOW_SIZES[-1] // 40, 1))       # 40 distinct descriptors: long runs
    plain = make_vocabulary(k=k, L=L, seed=k + L, stop_fraction=0.0)                               # every feature is kept: n keys exactly
    stopped = dict(plain, weight=plain["weight"].copy())
    leaves = np.nonzero(plain["is_leaf"])[0]
    stopped["weight"][leaves[::3]] = 0.0                                                           # a third of the words stopped
    for voc in (plain, stopped):
        V = svoc.Vocabulary.from_arrays(ctx, k, L, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], weighting=weighting)
        for feats in (random, tiled):
            for n in BOW_SIZES:
                ids, vals = sloop.debug_bow(V, feats[:n])
                t_ids, t_vals = V.transform(feats[:n])
                assert ids.tobytes() == t_ids.tobytes() and vals.tobytes() == t_vals.tobytes(), (n, len(ids), len(t_ids))
                word, w = po.voc_transform_features(voc, feats[:n])
                o_ids, o_vals = po.bow_vector(word, w, weighting=weighting)
                assert ids.tobytes() == o_ids.tobytes() and vals.tobytes() == o_vals.tobytes(), n
        V.close()


def test_bow_vector_longer_than_the_lds_query_stage(ctx, po, ex):
    """2000 features x 8 levels on a KITTI-sized image and a vocabulary of 10 000 words: more than 4096 words in the BowVector, so k_kfdb_score
    searches the query in global memory, and more than 4096 keys, so k_kf_bow sorts in its global scratch"""
    voc = make_vocabulary(k=10, L=4)
    V4 = svoc.Vocabulary.from_arrays(ctx, 10, 4, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    img = make_stereo_pair(seed=0)[0]
    feats = po.orb_detect(img, prm=po.orb_params(nfeatures=2000))
    rng = np.random.default_rng(8)
    A, B = sloop.KeyframeDatabase(ctx, keyframes_hint=4), sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    ra, kf = five_calls(A, V4, ex, 0, img, feats, 2, 20)
    rb = B.process_keyframe(V4, 0, img, feats, ex.prm, THRESHOLD, min_db_size=2, min_id_gap=20)
    same_result(ra, rb)
    assert ra["n_bow"] > 4096 and rb["n_bow"] > 4096, ra["n_bow"]
    same_keyframe(kf, B.pending())
    A.add(0, kf["bow"], kf["desc"], kf["class_id"])
    B.add_pending()
    for i in range(1, 6):                                     # some more keyframes sharing words with it
        pick = np.sort(rng.choice(len(kf["bow"][0]), 900, replace=False))
        vals = kf["bow"][1][pick] * rng.uniform(0.7, 1.3, 900)
        for db in (A, B):
            db.add(i, (kf["bow"][0][pick], vals / vals.sum()), kf["desc"][:50], kf["class_id"][:50])
    ra, kf2 = five_calls(A, V4, ex, 40, img, feats, 2, 20)    # the revisit
    rb = B.process_keyframe(V4, 40, img, feats, ex.prm, THRESHOLD, min_db_size=2, min_id_gap=20)
    same_result(ra, rb)
    assert rb["n_bow"] > 4096 and rb["found"] and rb["loop_kf_id"] == 0 and rb["n_scored"] == 6 and rb["n_pairs"] >= 10
    same_keyframe(kf2, B.pending())
    stats = B.debug_last_step()
    assert stats["syncs"] == 2 and stats["bytes_down"] <= 256 + 8 * len(rb["pairs"]), stats
    A.close(); B.close(); V4.close()


def test_empty_ends(ctx, po, V, ex):
    img, feats = small_scene(po, 0)
    img2, feats2 = small_scene(po, 1)
    border = feats[:40].copy()
    border["x"] = np.linspace(0.0, 18.0, 40, dtype=np.float32)    # within 19 px of the left border on every level
    empty_voc = svoc.Vocabulary.from_arrays(ctx, 10, 3, [-1], [0], np.zeros((1, 32), np.uint8), [0.0])
    A, B = sloop.KeyframeDatabase(ctx, keyframes_hint=2), sloop.KeyframeDatabase(ctx, keyframes_hint=2)
    cases = [("plain", V, img, feats, 0), ("plain 2", V, img2, feats2, 0), ("no features", V, img, feats[:0], 0), ("border", V, img, border, 0),
             ("empty vocabulary", empty_voc, img, feats, 0), ("database too small", V, img, feats, 100), ("revisit", V, img, feats, 0)]
    for kf_id, (name, voc, im, ft, min_db) in enumerate(cases):
        ra, kf = five_calls(A, voc, ex, kf_id, im, ft, min_db, 1)
        rb = B.process_keyframe(voc, kf_id, im, ft, ex.prm, THRESHOLD, min_db_size=min_db, min_id_gap=1)
        same_result(ra, rb)
        same_keyframe(kf, B.pending())
        if name in ("no features", "border"):
            assert rb["n_pyramid"] == 0 and rb["n_bow"] == 0 and not rb["found"], name
        if name == "empty vocabulary":
            assert rb["n_pyramid"] > 300 and rb["n_bow"] == 0 and not rb["found"]
        if name == "database too small":
            assert not rb["detect_ran"] and rb["n_scored"] == 0 and not rb["found"] and rb["n_bow"] > 100
        if name == "revisit":
            assert rb["found"] and rb["loop_kf_id"] == 0 and rb["n_scored"] == 6
        A.add(kf_id, kf["bow"], kf["desc"], kf["class_id"])       # each of them can be committed
        B.add_pending()
        assert A.size() == B.size()
    same_contents(A, B, 100, five_calls(A, V, ex, 100, img2, feats2, 0, 1)[1]["bow"])
    A.close(); B.close(); empty_voc.close()


def test_pending_survives_growth_and_foreign_adds(ctx, po, V, ex):
    img, feats = small_scene(po, 2)
    rng = np.random.default_rng(12)
    A, B = sloop.KeyframeDatabase(ctx, keyframes_hint=1), sloop.KeyframeDatabase(ctx, keyframes_hint=1)
    ra, kf = five_calls(A, V, ex, 5000, img, feats, 0, 1)
    rb = B.process_keyframe(V, 5000, img, feats, ex.prm, THRESHOLD, min_db_size=0, min_id_gap=1)
    same_result(ra, rb)
    # 300 keyframes with smaller ids and a large one: the arena (48 KB at first) and the table (256 rows at first) both grow, more than once
    big = (np.arange(3000, dtype=np.int32), np.full(3000, 1.0 / 3000))
    big_desc = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    for db in (A, B):
        for i in range(300):
            db.add(i, (np.arange(i, i + 40, dtype=np.int32), np.full(40, 0.025)), big_desc[i:i + 3], np.arange(3, dtype=np.int32))
        db.add(300, big, big_desc, np.arange(3000, dtype=np.int32))
    same_keyframe(kf, B.pending())                                # still there
    A.add(5000, kf["bow"], kf["desc"], kf["class_id"])
    B.add_pending()
    same_contents(A, B, 10 ** 6, kf["bow"])
    pa, ma = A.match_features(5000, kf["desc"], kf["class_id"])
    pb, mb = B.match_features(5000, kf["desc"], kf["class_id"])
    assert ma == mb == 0 and pa.tobytes() == pb.tobytes() and len(pb) >= 10
    A.close(); B.close()


def test_misuse_leaves_the_database_usable(ctx, po, V, ex):
    img, feats = small_scene(po, 3)
    A, B = sloop.KeyframeDatabase(ctx, keyframes_hint=2), sloop.KeyframeDatabase(ctx, keyframes_hint=2)

    def status_of(call):
        with pytest.raises(SsxError) as e:
            call()
        return e.value.status, e.value

    assert status_of(B.add_pending)[0] == _lib.SSX_ERR_INVALID_ARG            # nothing pending
    assert status_of(B.pending)[0] == _lib.SSX_ERR_INVALID_ARG
    ra, kf = five_calls(A, V, ex, 10, img, feats, 0, 1)
    A.add(10, kf["bow"], kf["desc"], kf["class_id"])
    B.process_keyframe(V, 10, img, feats, ex.prm, THRESHOLD, min_db_size=0, min_id_gap=1)
    B.add_pending()
    assert status_of(B.add_pending)[0] == _lib.SSX_ERR_INVALID_ARG            # a keyframe is committed once
    B.process_keyframe(V, 10, img, feats, ex.prm, THRESHOLD, min_db_size=0, min_id_gap=1)
    assert status_of(B.add_pending)[0] == _lib.SSX_ERR_INVALID_ARG            # ids must ascend
    # a vocabulary of another context
    other = _lib.Context(0)
    voc = make_vocabulary(k=10, L=3)
    foreign = svoc.Vocabulary.from_arrays(other, 10, 3, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    assert status_of(lambda: B.process_keyframe(foreign, 20, img, feats, ex.prm, THRESHOLD))[0] == _lib.SSX_ERR_INVALID_ARG
    assert status_of(B.add_pending)[0] == _lib.SSX_ERR_INVALID_ARG            # a call that fails leaves nothing pending
    foreign.close(); other.close()
    many = np.zeros(8192, KP_DTYPE)                                           # 8192 x 8 = 65536 pyramid keypoints
    assert status_of(lambda: B.process_keyframe(V, 20, img, many, ex.prm, THRESHOLD))[0] == _lib.SSX_ERR_UNSUPPORTED
    assert status_of(lambda: B.process_keyframe(V, 20, img, feats, ex.prm, THRESHOLD, pyramid_levels=0))[0] == _lib.SSX_ERR_INVALID_ARG
    assert A.size() == B.size()
    # pairs_cap too small: SSX_ERR_CAPACITY, the first pairs written, the keyframe still pending and committable
    ra, kf = five_calls(A, V, ex, 20, img, feats, 0, 1)
    assert ra["found"] and ra["n_pairs"] > 12
    st, err = status_of(lambda: B.process_keyframe(V, 20, img, feats, ex.prm, THRESHOLD, min_db_size=0, min_id_gap=1, pairs_cap=7))
    assert st == _lib.SSX_ERR_CAPACITY and err.result["n_pairs"] == ra["n_pairs"] and err.result["min_distance"] == ra["min_distance"]
    assert err.result["pairs"].tobytes() == ra["pairs"][:7].tobytes()
    same_keyframe(kf, B.pending())
    A.add(20, kf["bow"], kf["desc"], kf["class_id"])
    B.add_pending()
    # after all of it B answers like A
    img2, feats2 = small_scene(po, 4)
    for kf_id, (im, ft) in ((30, (img2, feats2)), (40, (img, feats))):
        ra, kf = five_calls(A, V, ex, kf_id, im, ft, 0, 1)
        rb = B.process_keyframe(V, kf_id, im, ft, ex.prm, THRESHOLD, min_db_size=0, min_id_gap=1)
        same_result(ra, rb)
        same_keyframe(kf, B.pending())
    same_contents(A, B, 100, kf["bow"])
    A.close(); B.close()
