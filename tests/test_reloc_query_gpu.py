"""GPU: the candidate query of relocalisation (ssx_kfdb_relocalize_query: k_kfdb_topk and the job-indexed match behind the keyframe step's
describe / BowVector / score kernels) against the composition of the single calls it replaces, on a twin database:
ssx_orb_describe_at -> ssx_voc_transform -> ssx_kfdb_detect_loop(..., scores_out) -> tools.reloc_model.select_candidates ->
ssx_kfdb_match_features per candidate.  Everything is integer or ordered-double arithmetic: every comparison is on bytes.

The stored keyframes are synthetic (ssx_kfdb_add): about 20 BowVector entries, some of them words of the query, and 16 to 64
descriptors, some of them noisy copies of the query's, so that a database of 1030 costs nothing and still has graded scores and
matches.  The query is one 320 x 200 image with about 60 features."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import loop as sloop
from ssvio_amd import orb as sorb
from ssvio_amd import voc as svoc
from ssvio_amd._lib import KP_DTYPE, SsxError
from tools.reloc_model import select_candidates
from tools.synth import make_stereo_pair, make_vocabulary

pytestmark = pytest.mark.gpu

LEVELS = 8
ANY_ID = 2 ** 63 - 1                                            # the query id that makes every stored keyframe eligible (min_id_gap 0)
SIZES = (0, 1, 3, 8, 9, 257, 1030)                              # 257, 1030: more rows than k_kfdb_topk has threads / more than one row per thread
SETTINGS = ((1, 0.0, 0.75), (4, 0.0, 0.75), (8, 0.0, 0.0), (8, 0.02, 0.5), (4, 0.0, 1.0))   # (K, threshold, ratio)


def expand(features, levels=LEVELS):
    out = np.repeat(np.ascontiguousarray(features, dtype=KP_DTYPE), levels)
    out["octave"] = np.tile(np.arange(levels, dtype=np.int32), len(features))
    out["response"] = -1.0
    out["class_id"] = np.repeat(np.arange(len(features), dtype=np.int32), levels)
    return out


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
def frame(po, V, ex):
    """the query frame and what the single calls make of it (computed once, never changed)"""
    img = make_stereo_pair(seed=140, h=200, w=320, n_blobs=400)[0]
    feats = po.orb_detect(img, prm=po.orb_params(nfeatures=60))
    kps, desc = ex.ScreenAndComputeKPsParams_CalcDescriptors(img, expand(feats))
    cls = np.ascontiguousarray(kps["class_id"])
    bow = V.transform(desc)
    assert 30 <= len(feats) <= 120 and len(desc) > 100 and len(bow[0]) > 50
    return dict(img=img, feats=feats, desc=desc, cls=cls, bow=bow)


def synthetic_keyframe(rng, frame, n_words=1000):
    """-> (bow, desc, class_id): ~20 words, 0 to 20 of them the query's; 16 to 64 descriptors, half of them the query's with a few bits flipped"""
    q_ids, q_vals = frame["bow"]
    shared = rng.choice(len(q_ids), size=int(rng.integers(0, 21)), replace=False)
    other = np.setdiff1d(np.arange(n_words, dtype=np.int32), q_ids)
    ids = np.union1d(q_ids[shared], rng.choice(other, size=20 - len(shared), replace=False)).astype(np.int32)
    vals = rng.random(len(ids)) + 0.05
    vals /= vals.sum()
    nd = int(rng.integers(16, 65))
    desc = rng.integers(0, 256, (nd, 32), dtype=np.uint8)
    src = rng.choice(len(frame["desc"]), size=nd // 2, replace=False)
    noisy = np.unpackbits(frame["desc"][src], axis=1)
    noisy ^= (rng.random(noisy.shape) < rng.choice([0.0, 0.03, 0.1])).astype(np.uint8)
    desc[:nd // 2] = np.packbits(noisy, axis=1)
    return (ids, vals), desc, rng.integers(0, 500, nd).astype(np.int32)


class Twin:
    """two databases with the same contents: A for the single calls, B for the query"""

    def __init__(self, ctx):
        self.A, self.B, self.ids = sloop.KeyframeDatabase(ctx, keyframes_hint=4), sloop.KeyframeDatabase(ctx, keyframes_hint=4), []

    def add(self, kf_id, bow, desc=None, cls=None):
        self.A.add(kf_id, bow, desc, cls)
        self.B.add(kf_id, bow, desc, cls)
        self.ids.append(kf_id)

    def close(self):
        self.A.close(); self.B.close()


@pytest.fixture(scope="module")
def twins(ctx, frame):
    """one twin per size of SIZES, each a prefix of the same 1030 synthetic keyframes (ids 3, 6, 9, ...: an id is not its row)"""
    rng = np.random.default_rng(77)
    kfs = [synthetic_keyframe(rng, frame) for _ in range(max(SIZES))]
    out = {}
    for n in SIZES:
        t = Twin(ctx)
        for i in range(n):
            t.add(3 * i + 3, *kfs[i])
        out[n] = t
    yield out
    for t in out.values():
        t.close()


def composition(t, frame, K, threshold, ratio):
    """the query as a caller of the parent's entry points runs it"""
    desc, cls, bow = frame["desc"], frame["cls"], frame["bow"]
    found, best_id, best_score, n_scored, scores = t.A.detect_loop(ANY_ID, bow, threshold, min_id_gap=0, with_scores=True)
    rows, ids, f = select_candidates(scores, np.array(t.ids, np.int64), K, threshold, ratio)
    cands = []
    for row, kf_id, score in zip(rows, ids, f):
        try:
            pairs, md = t.A.match_features(int(kf_id), desc, cls)
            cands.append(dict(kf_id=int(kf_id), score=score, row=int(row), no_descriptors=False, n_pairs=len(pairs), min_distance=md, pairs=pairs))
        except SsxError as e:
            assert "without descriptors" in str(e)
            cands.append(dict(kf_id=int(kf_id), score=score, row=int(row), no_descriptors=True, n_pairs=0, min_distance=-1, pairs=np.zeros((0, 2), np.int32)))
    return dict(n_pyramid=len(desc), n_bow=len(bow[0]), n_scored=n_scored, candidates=cands), (found, best_id, best_score)


def same_query(a, b):
    for key in ("n_pyramid", "n_bow", "n_scored"):
        assert a[key] == b[key], (key, a[key], b[key])
    assert len(a["candidates"]) == len(b["candidates"]), ([c["kf_id"] for c in a["candidates"]], [c["kf_id"] for c in b["candidates"]])
    for ca, cb in zip(a["candidates"], b["candidates"]):
        for key in ("kf_id", "row", "no_descriptors", "n_pairs", "min_distance"):
            assert ca[key] == cb[key], (key, ca, cb)
        assert np.float32(ca["score"]).tobytes() == np.float32(cb["score"]).tobytes()
        assert ca["pairs"].shape == cb["pairs"].shape and ca["pairs"].tobytes() == cb["pairs"].tobytes()


def query(t, V, ex, frame, K, threshold, ratio, **kw):
    return t.B.relocalize_query(V, frame["img"], frame["feats"], ex.prm, max_candidates=K, threshold=threshold, ratio=ratio, pyramid_levels=LEVELS, **kw)


@pytest.mark.parametrize("n", SIZES)
def test_the_query_equals_the_composition(twins, V, ex, frame, n):
    t = twins[n]
    seen, most_pairs = [], 0
    for K, threshold, ratio in SETTINGS:
        want, (found, best_id, best_score) = composition(t, frame, K, threshold, ratio)
        got = query(t, V, ex, frame, K, threshold, ratio)
        same_query(want, got)
        assert got["n_scored"] == n
        # the head of the list is DetectLoop's winner
        assert found == (len(got["candidates"]) > 0)
        if found:
            assert got["candidates"][0]["kf_id"] == best_id and np.float32(got["candidates"][0]["score"]).tobytes() == np.float32(best_score).tobytes()
        seen.append(len(got["candidates"]))
        most_pairs = max([most_pairs] + [c["n_pairs"] for c in got["candidates"]])
    if n >= 257:
        assert seen[0] == 1 and seen[2] == 8 and most_pairs >= 5, (seen, most_pairs)   # the cases are not vacuous
    if n == 0:
        assert seen == [0] * len(SETTINGS)
    if n in (1, 3):
        assert max(seen) <= n                                    # K larger than the database


def test_ties_come_in_id_order_and_a_tie_at_rank_K_keeps_the_lower_id(ctx, V, ex, frame):
    rng = np.random.default_rng(5)
    t = Twin(ctx)
    same = synthetic_keyframe(rng, frame)
    best = (frame["bow"][0], frame["bow"][1])                    # the query's own BowVector: score 1
    t.add(10, *synthetic_keyframe(rng, frame))
    t.add(20, same[0], same[1], same[2])
    t.add(30, best, same[1], same[2])
    t.add(40, same[0], same[1][:20], same[2][:20])               # the same BowVector, other descriptors
    t.add(50, *synthetic_keyframe(rng, frame))
    t.add(60, same[0], same[1], same[2])
    for K in (8, 4, 3, 2, 1):
        want, _ = composition(t, frame, K, 0.0, 0.0)
        got = query(t, V, ex, frame, K, 0.0, 0.0)
        same_query(want, got)
    ids = [c["kf_id"] for c in query(t, V, ex, frame, 8, 0.0, 0.0)["candidates"]]
    assert ids[0] == 30 and [i for i in ids if i in (20, 40, 60)] == [20, 40, 60]
    at = ids.index(20)                                           # 20, 40, 60 are adjacent: cut inside the tie
    assert [c["kf_id"] for c in query(t, V, ex, frame, at + 2, 0.0, 0.0)["candidates"]] == ids[:at] + [20, 40]
    assert [c["kf_id"] for c in query(t, V, ex, frame, at + 1, 0.0, 0.0)["candidates"]] == ids[:at] + [20]
    t.close()


def test_a_threshold_or_a_ratio_that_empties_the_set(twins, V, ex, frame):
    t = twins[9]
    got = query(t, V, ex, frame, 8, 2.0, 0.0)                    # an L1 score is at most 1
    assert got["candidates"] == [] and got["n_scored"] == 9 and got["n_pyramid"] == len(frame["desc"])
    same_query(composition(t, frame, 8, 2.0, 0.0)[0], got)
    got = query(t, V, ex, frame, 8, float("inf"), 1.0)
    assert got["candidates"] == []
    # ratio 1 keeps the best (and its ties) only
    got = query(t, V, ex, frame, 8, 0.0, 1.0)
    assert len(got["candidates"]) == 1
    # nothing to query: no features, no surviving keypoint, an empty vocabulary
    assert t.B.relocalize_query(V, frame["img"], frame["feats"][:0], ex.prm)["candidates"] == []
    border = frame["feats"][:40].copy()
    border["x"] = np.linspace(0.0, 18.0, len(border), dtype=np.float32)
    r = t.B.relocalize_query(V, frame["img"], border, ex.prm, threshold=0.0, ratio=0.0)
    assert r["candidates"] == [] and r["n_pyramid"] == 0 and r["n_bow"] == 0 and r["n_scored"] == 9
    empty_voc = svoc.Vocabulary.from_arrays(t.B.ctx, 10, 3, [-1], [0], np.zeros((1, 32), np.uint8), [0.0])
    r = t.B.relocalize_query(empty_voc, frame["img"], frame["feats"], ex.prm, threshold=0.0, ratio=0.0)
    assert r["candidates"] == [] and r["n_pyramid"] == len(frame["desc"]) and r["n_bow"] == 0
    empty_voc.close()


def test_candidates_without_descriptors_and_one_beyond_the_lds_sort(ctx, V, ex, frame):
    """a keyframe stored without descriptors is flagged and the others are complete; one stored with none at all (an empty set) has no
    pairs; one with 5000 copies of the query's descriptors keeps more than 4096 pairs, so k_kfdb_pairs sorts in its global scratch"""
    rng = np.random.default_rng(6)
    t = Twin(ctx)
    q_ids, q_vals = frame["bow"]
    t.add(1, *synthetic_keyframe(rng, frame))
    t.add(2, (q_ids, q_vals))                                    # the best score, no descriptors
    t.add(3, (q_ids[::2], q_vals[::2] / q_vals[::2].sum()), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32))
    many = frame["desc"][rng.integers(0, len(frame["desc"]), 5000)]
    t.add(4, (q_ids[1::2], q_vals[1::2] / q_vals[1::2].sum()), many, np.arange(5000, dtype=np.int32))
    t.add(5, *synthetic_keyframe(rng, frame))
    want, _ = composition(t, frame, 8, 0.0, 0.0)
    got = query(t, V, ex, frame, 8, 0.0, 0.0)
    same_query(want, got)
    by_id = {c["kf_id"]: c for c in got["candidates"]}
    assert got["candidates"][0]["kf_id"] == 2 and by_id[2]["no_descriptors"] and by_id[2]["n_pairs"] == 0 and by_id[2]["min_distance"] == -1
    assert not by_id[3]["no_descriptors"] and by_id[3]["n_pairs"] == 0 and by_id[3]["min_distance"] == -1
    assert by_id[4]["n_pairs"] > 4096 and by_id[4]["min_distance"] == 0
    assert by_id[1]["n_pairs"] > 0 and by_id[5]["n_pairs"] > 0
    t.close()


def test_the_pending_keyframe_and_the_stored_ones_are_untouched(ctx, po, twins, V, ex, frame):
    src = twins[9]
    db = sloop.KeyframeDatabase(ctx, keyframes_hint=2)
    rng = np.random.default_rng(77)
    for i in range(9):
        db.add(3 * i + 3, *synthetic_keyframe(rng, frame))       # (the same generator and seed as `twins`: the same nine keyframes)
    other = make_stereo_pair(seed=141, h=200, w=320, n_blobs=400)[0]
    db.process_keyframe(V, 1000, other, po.orb_detect(other, prm=po.orb_params(nfeatures=150)), ex.prm, 0.6, pyramid_levels=LEVELS)
    before, size = db.pending(), db.size()
    got = db.relocalize_query(V, frame["img"], frame["feats"], ex.prm, max_candidates=8, threshold=0.0, ratio=0.0, pyramid_levels=LEVELS)
    same_query(composition(src, frame, 8, 0.0, 0.0)[0], got)
    after = db.pending()
    assert db.size() == size and after["kf_id"] == before["kf_id"] == 1000
    for key in ("keypoints", "desc", "class_id"):
        assert after[key].tobytes() == before[key].tobytes() and len(after[key]) == len(before[key]) > 0
    assert after["bow"][0].tobytes() == before["bow"][0].tobytes() and after["bow"][1].tobytes() == before["bow"][1].tobytes()
    db.add_pending()
    assert db.size()[0] == size[0] + 1
    # the committed keyframe is what was pending before the query
    pairs, md = db.match_features(1000, before["desc"], before["class_id"])
    assert md == 0 and len(pairs) >= 10
    db.close()


def test_capacity(twins, V, ex, frame):
    t = twins[257]
    full = query(t, V, ex, frame, 8, 0.0, 0.0)
    counts = [c["n_pairs"] for c in full["candidates"]]
    cap = max(counts) - 1
    assert cap >= 1 and min(counts) <= cap                       # some candidate fits, some does not
    with pytest.raises(SsxError) as e:
        query(t, V, ex, frame, 8, 0.0, 0.0, pairs_cap=cap)
    assert e.value.status == _lib.SSX_ERR_CAPACITY
    part = e.value.result
    assert [c["n_pairs"] for c in part["candidates"]] == counts  # every count is true
    for a, b in zip(full["candidates"], part["candidates"]):
        assert a["kf_id"] == b["kf_id"] and a["min_distance"] == b["min_distance"]
        assert b["pairs"].tobytes() == a["pairs"][:cap].tobytes()
    assert query(t, V, ex, frame, 8, 0.0, 0.0, pairs_cap=max(counts))["candidates"][0]["n_pairs"] == counts[0]


def test_misuse_is_rejected_and_leaves_the_database_as_it_was(ctx, twins, V, ex, frame):
    t = twins[9]
    before = query(t, V, ex, frame, 8, 0.0, 0.0)
    size = t.B.size()

    def status_of(call):
        with pytest.raises(SsxError) as e:
            call()
        return e.value.status

    bad = [dict(K=0), dict(K=9), dict(K=-1), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(ratio=-0.01), dict(ratio=1.01),
           dict(threshold=-0.01), dict(threshold=float("nan"))]
    for kw in bad:
        a = dict(dict(K=4, threshold=0.0, ratio=0.75), **kw)
        assert status_of(lambda: query(t, V, ex, frame, a["K"], a["threshold"], a["ratio"])) == _lib.SSX_ERR_INVALID_ARG, kw
    assert status_of(lambda: t.B.relocalize_query(V, frame["img"], frame["feats"], ex.prm, pyramid_levels=0)) == _lib.SSX_ERR_INVALID_ARG
    assert status_of(lambda: t.B.relocalize_query(V, frame["img"], np.zeros(8192, KP_DTYPE), ex.prm)) == _lib.SSX_ERR_UNSUPPORTED
    other = _lib.Context(0)
    voc = make_vocabulary(k=10, L=3)
    foreign = svoc.Vocabulary.from_arrays(other, 10, 3, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    assert status_of(lambda: t.B.relocalize_query(foreign, frame["img"], frame["feats"], ex.prm)) == _lib.SSX_ERR_INVALID_ARG
    foreign.close(); other.close()
    # null required pointers, through the C entry point itself
    lib, img, feats = ctx.lib, frame["img"], np.ascontiguousarray(frame["feats"], dtype=KP_DTYPE)
    res, pairs = sloop.RelocQueryResult(), np.zeros((4, 64, 2), np.int32)
    good = [t.B.handle, V.handle, _lib.ptr(img, _lib.u8_p), img.strides[0], img.shape[0], img.shape[1], C.byref(ex.prm), len(feats),
            feats.ctypes.data_as(C.c_void_p), LEVELS, 4, 0.0, 0.75, 64, _lib.ptr(pairs, _lib.i32_p), C.byref(res)]
    for k in (0, 1, 2, 6, 8, 14, 15):                             # db, voc, img, prm, features, pairs_out, res
        args = list(good)
        args[k] = None
        assert lib.ssx_kfdb_relocalize_query(*args) == _lib.SSX_ERR_INVALID_ARG, k
    args = list(good); args[3] = img.shape[1] - 1                 # a stride below the width
    assert lib.ssx_kfdb_relocalize_query(*args) == _lib.SSX_ERR_INVALID_ARG
    args = list(good); args[13] = -1
    assert lib.ssx_kfdb_relocalize_query(*args) == _lib.SSX_ERR_INVALID_ARG
    assert t.B.size() == size
    same_query(before, query(t, V, ex, frame, 8, 0.0, 0.0))


def test_budget_is_independent_of_K_and_of_the_database(twins, V, ex, frame):
    """launches and synchronisations (ssx_kfdb_debug_last_step) do not depend on max_candidates or on the stored keyframes; one
    synchronisation once the image shape is planned (never more than two)"""
    stats = {}
    for n in (9, 1030):
        for K in (1, 8):
            query(twins[n], V, ex, frame, K, 0.0, 0.0)           # (the first call of the module may plan the image shape)
            r = query(twins[n], V, ex, frame, K, 0.0, 0.0)
            stats[n, K] = twins[n].B.debug_last_step()
            assert 1 <= len(r["candidates"]) <= K
    first = stats[9, 1]
    for key, s in stats.items():
        assert s["launches"] == first["launches"] and s["syncs"] == first["syncs"], (key, s, first)
    assert 0 < first["launches"] <= 24 and 1 <= first["syncs"] <= 2
    # only the image and the keypoints go up; the result block, the pair counts and the pairs come down
    assert first["bytes_up"] < 200 * 320 + 28 * LEVELS * len(frame["feats"]) + 4 * 256
    for (n, K), s in stats.items():
        r = query(twins[n], V, ex, frame, K, 0.0, 0.0)
        assert s["bytes_down"] <= 256 + sum(8 + 8 * c["n_pairs"] for c in r["candidates"])


def test_two_calls_give_the_same_bytes(twins, V, ex, frame):
    t = twins[1030]
    a = query(t, V, ex, frame, 8, 0.0, 0.5)
    b = query(t, V, ex, frame, 8, 0.0, 0.5)
    same_query(a, b)
    assert len(a["candidates"]) >= 2
