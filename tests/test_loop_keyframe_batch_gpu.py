"""GPU parity of ssx_kfdb_process_keyframe_batch (the per-keyframe step of loop closing for one keyframe of each of several databases,
one launch chain) against the single calls it stands for: ssx_kfdb_add_pending when asked for, then ssx_kfdb_process_keyframe, on a twin
database.  Those are held to the five older entry points and through them to the CPU oracle by test_loop_keyframe_gpu.py, whose scenes,
vocabulary and helpers are used here; everything is integer or ordered-double arithmetic, so every comparison is on bytes."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import loop as sloop
from ssvio_amd import voc as svoc
from ssvio_amd._lib import SsxError
from test_loop_keyframe_gpu import LEVELS, THRESHOLD, V, ex, same_contents, same_keyframe, same_result, small_scene  # noqa: F401 (V, ex: fixtures)
from tools.synth import make_stereo_pair, make_vocabulary

pytestmark = pytest.mark.gpu

PLACES = list(range(6)) + [0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11, 0, 12, 6, 13, 7, 1, 14, 8, 9, 15, 2, 10]     # the drive of test_loop_keyframe_gpu.py
KW = dict(pyramid_levels=LEVELS, min_db_size=2, min_id_gap=3)


@pytest.fixture(scope="module")
def scenes(po):
    return {s: small_scene(po, s) for s in sorted(set(PLACES))}


same_pending = same_keyframe                                     # two downloads of ssx_kfdb_pending


def single(db, V, prm, job, **kw):
    """what a job of the batch call stands for, on the twin database"""
    if job.get("commit_pending"):
        db.add_pending()
    extra = {} if job.get("pairs_cap") is None else dict(pairs_cap=job["pairs_cap"])
    return db.process_keyframe(V, job["kf_id"], job["image"], job["features"], prm, THRESHOLD, **kw, **extra)


def stored_alike(A, B, V, ex, ids, cur, query_id=10 ** 6):
    """size, BowVectors (a query scores the same doubles against every keyframe) and descriptors + class ids (MatchFeatures against every one)"""
    same_contents(A, B, query_id, cur["bow"])
    for kf_id in ids:
        pa, ma = A.match_features(kf_id, cur["desc"], cur["class_id"])
        pb, mb = B.match_features(kf_id, cur["desc"], cur["class_id"])
        assert ma == mb and pa.tobytes() == pb.tobytes()


def border_features(feats):
    out = feats[:40].copy()
    out["x"] = np.linspace(0.0, 18.0, 40, dtype=np.float32)      # within 19 px of the left border on every level: no keypoint survives
    return out


def test_batch_equals_single_calls(ctx, V, ex, scenes):
    """five databases walk the 30 places, database j 3 j calls behind the first: a call mixes empty and full databases, detection that ran
    and that did not, found and not found, eligible prefixes of different lengths, 150 / 90 / 40 / 0 features and once none that survives"""
    B = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(5)]
    T = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(5)]
    counts = {0: [150], 1: [150], 2: [90], 3: [40], 4: [150, 0, 90, 40]}
    commit = [False] * 5
    stored = [[] for _ in range(5)]
    last = [None] * 5
    kinds = []
    sizes = set()
    mixed_detect = mixed_prefix = False
    for call in range(30):
        jobs, who = [], []
        for j in range(5):
            step = call - 3 * j
            if step < 0:
                continue
            img, feats = scenes[PLACES[step]]
            ft = feats[:counts[j][step % len(counts[j])]]
            if j == 3 and step == 9:
                ft = border_features(feats)
            jobs.append(dict(db=B[j], kf_id=2 * step + 1, image=img, features=ft, commit_pending=commit[j]))
            who.append(j)
        sizes.add(len(jobs))
        got = sloop.process_keyframe_batch(V, jobs, ex.prm, THRESHOLD, **KW)
        for j, job, rb in zip(who, jobs, got):
            if job["commit_pending"]:
                stored[j].append(last[j])
            rt = single(T[j], V, ex.prm, job, **KW)
            assert rb["status"] == 0
            same_result(rt, rb)
            pend = B[j].pending()
            same_pending(T[j].pending(), pend)
            assert B[j].size() == T[j].size(), (call, j)
            commit[j] = rb["n_pairs"] < 10                       # the reference skips the commit after a confirmed loop (loopclosing.cpp:57-66)
            last[j] = job["kf_id"]
            if j == 3 and call - 3 * j == 9:
                assert rb["n_pyramid"] == 0 and rb["n_bow"] == 0 and not rb["found"]
        kinds.append([r["found"] for r in got])
        mixed_detect = mixed_detect or len({r["detect_ran"] for r in got}) == 2
        mixed_prefix = mixed_prefix or len({r["n_scored"] for r in got if r["detect_ran"]}) >= 3
    assert sizes == {1, 2, 3, 4, 5} and mixed_detect and mixed_prefix
    assert any(sum(k) >= 2 for k in kinds), "no call with two found jobs"
    assert any(any(k) and not all(k) for k in kinds), "no call with found and not-found jobs together"
    # afterwards: the single-database entry points work on every database, and the contents are the twin's
    cur = B[0].pending()
    for j in range(5):
        if commit[j]:
            B[j].add_pending(); T[j].add_pending(); stored[j].append(last[j])
        stored_alike(T[j], B[j], V, ex, stored[j], cur)
    assert len(B[0]) >= 6
    for db in B + T:
        db.close()


def test_batch_of_one_and_permuted_table(ctx, V, ex, scenes):
    """the bytes of a job do not depend on the number of jobs or on its place in the table"""
    places = [0, 1, 2, 3, 0, 1, 4, 2]
    groups = [[sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(3)] for _ in range(3)]    # in order, reversed, one job per call
    feats_of = [150, 90, 40]
    commit = [False] * 3
    found = False
    for step, place in enumerate(places):
        img, feats = scenes[place]
        img2, feats2 = scenes[places[(step + 3) % len(places)]]
        mk = lambda g, j: dict(db=groups[g][j], kf_id=5 * step + 2, image=img if j != 1 else img2, features=(feats if j != 1 else feats2)[:feats_of[j]],
                               commit_pending=commit[j])
        kw = dict(pyramid_levels=LEVELS, min_db_size=1, min_id_gap=6)
        fwd = sloop.process_keyframe_batch(V, [mk(0, j) for j in range(3)], ex.prm, THRESHOLD, **kw)
        rev = sloop.process_keyframe_batch(V, [mk(1, j) for j in (2, 0, 1)], ex.prm, THRESHOLD, **kw)
        rev = [rev[1], rev[2], rev[0]]
        one = [sloop.process_keyframe_batch(V, [mk(2, j)], ex.prm, THRESHOLD, **kw)[0] for j in range(3)]
        for j in range(3):
            same_result(fwd[j], rev[j]); same_result(fwd[j], one[j])
            p = groups[0][j].pending()
            same_pending(p, groups[1][j].pending()); same_pending(p, groups[2][j].pending())
            commit[j] = fwd[j]["n_pairs"] < 10
            found = found or fwd[j]["found"]
    assert found
    for g in groups:
        for db in g:
            db.close()


def test_eleven_jobs(ctx, V, ex, scenes):
    """more than 8 images in a call: the pyramid's resize kernel takes its looped form and the ORB plan is one for 16 images; k_voc_words
    bisects a table of 11 jobs, two of them empty.  Four calls on 11 databases, the last two revisits, against the twins"""
    n = 11
    B = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(n)]
    T = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(n)]
    counts = [150, 0, 90, 40, 150, 1, 0, 150, 90, 150, 7]
    kw = dict(pyramid_levels=LEVELS, min_db_size=1, min_id_gap=2)
    found = 0
    for step in range(4):
        jobs = []
        for j in range(n):
            img, feats = scenes[(j + (step % 2) * 3) % 16]        # steps 2 and 3 see the places of steps 0 and 1 again
            jobs.append(dict(kf_id=3 * step + 1, image=img, features=feats[:counts[j]], commit_pending=step > 0))
        got = sloop.process_keyframe_batch(V, [dict(q, db=B[j]) for j, q in enumerate(jobs)], ex.prm, THRESHOLD, **kw)
        for j, q in enumerate(jobs):
            rt = single(T[j], V, ex.prm, q, **kw)
            assert got[j]["status"] == 0
            same_result(rt, got[j])
            same_pending(T[j].pending(), B[j].pending())
            assert B[j].size() == T[j].size() and len(B[j]) == step
            found += got[j]["found"]
    assert found >= 4
    cur = T[0].pending()
    for j in range(n):
        B[j].add_pending(); T[j].add_pending()
        stored_alike(T[j], B[j], V, ex, [1, 4, 7, 10], cur)
    for db in B + T:
        db.close()


@pytest.mark.parametrize("hint", [64, 1])
def test_commit_pending(ctx, V, ex, scenes, hint):
    """commit_pending = 1 is add_pending() and then the step: after a 40-feature keyframe one of 150 (the pending buffer the commit reads
    from has to grow for the new keyframe), and with keyframes_hint = 1 the arena grows under the commit as well"""
    A, B = sloop.KeyframeDatabase(ctx, keyframes_hint=hint), sloop.KeyframeDatabase(ctx, keyframes_hint=hint)
    A2, B2 = sloop.KeyframeDatabase(ctx, keyframes_hint=hint), sloop.KeyframeDatabase(ctx, keyframes_hint=hint)   # a second job beside it, never committing
    sizes = [40, 150, 150, 90, 150, 0, 150, 150]
    kw = dict(pyramid_levels=LEVELS, min_db_size=0, min_id_gap=1)
    ids = []
    for step, nf in enumerate(sizes):
        img, feats = scenes[step % 5]
        job = dict(kf_id=10 * step, image=img, features=feats[:nf], commit_pending=step > 0)
        other = dict(kf_id=step, image=scenes[5][0], features=scenes[5][1][:60])
        rb, rb2 = sloop.process_keyframe_batch(V, [dict(job, db=B), dict(other, db=B2)], ex.prm, THRESHOLD, **kw)
        ra, ra2 = single(A, V, ex.prm, job, **kw), single(A2, V, ex.prm, other, **kw)
        if step > 0:
            ids.append(10 * (step - 1))
        same_result(ra, rb); same_result(ra2, rb2)
        same_pending(A.pending(), B.pending()); same_pending(A2.pending(), B2.pending())
        assert A.size() == B.size() and len(B) == step and len(B2) == 0
        if step >= 6:
            assert rb["found"] and rb["loop_kf_id"] == 10 * (step - 5), step     # the revisit of a keyframe that a commit of this very kind stored
    cur = A.pending()
    A.add_pending(); B.add_pending(); ids.append(10 * (len(sizes) - 1))
    stored_alike(A, B, V, ex, ids, cur)
    for db in (A, B, A2, B2):
        db.close()


def test_budget(ctx, V, ex, scenes):
    """launches and synchronisations do not depend on the number of jobs; one synchronisation when no job found a loop, two when one did; what
    goes up is the images, the keypoints and the job tables, what comes down the step headers and the pairs"""
    X = [sloop.KeyframeDatabase(ctx, keyframes_hint=64) for _ in range(5)]
    Y = [sloop.KeyframeDatabase(ctx, keyframes_hint=64)]
    W = [sloop.KeyframeDatabase(ctx, keyframes_hint=64) for _ in range(5)]
    kw = dict(pyramid_levels=LEVELS, min_db_size=0, min_id_gap=1)
    img, feats = scenes[0]
    sloop.process_keyframe_batch(V, [dict(db=w, kf_id=0, image=img, features=feats) for w in W], ex.prm, THRESHOLD, **kw)   # plans for 8 images
    seen = set()
    for step, place in enumerate([0, 1, 2, 0, 3, 1]):
        img, feats = scenes[place]
        stats = []
        for dbs in (X, Y):
            got = sloop.process_keyframe_batch(V, [dict(db=d, kf_id=step, image=img, features=feats, commit_pending=step > 0) for d in dbs], ex.prm,
                                               THRESHOLD, **kw)
            s = sloop.debug_last_batch(ctx)
            n, pairs = len(dbs), sum(len(r["pairs"]) for r in got)
            found = any(r["found"] and r["n_pairs"] > 0 for r in got)
            assert all(r["found"] == got[0]["found"] for r in got)
            assert s["syncs"] == (2 if found else 1), (step, s)
            assert s["bytes_down"] <= 16 * n + 8 * pairs + 256, (step, s)
            assert s["bytes_up"] < n * (img.size + 28 * LEVELS * len(feats)) + 256 * n, (step, s)
            stats.append((s["launches"], s["syncs"], found))
        assert stats[0] == stats[1], (step, stats)
        assert 0 < stats[0][0] <= 20
        seen.add(stats[0][2])
    assert seen == {True, False}
    for db in X + Y + W:
        db.close()


def test_both_sort_paths_side_by_side(ctx, po, ex):
    """a KITTI-sized job of 2000 features x 8 levels (more than 4096 keys: k_kf_bow sorts in its global scratch; more than 4096 words: k_kfdb_score
    searches the query in global memory) beside one of 100 features that takes the LDS paths, in one call; then both find their loop"""
    voc = make_vocabulary(k=10, L=4)
    V4 = svoc.Vocabulary.from_arrays(ctx, 10, 4, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    img = make_stereo_pair(seed=0)[0]
    feats = po.orb_detect(img, prm=po.orb_params(nfeatures=2000))
    rng = np.random.default_rng(8)
    A = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(2)]
    B = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(2)]
    fts = [feats, feats[:100]]
    kw = dict(pyramid_levels=LEVELS, min_db_size=2, min_id_gap=20)
    rb = sloop.process_keyframe_batch(V4, [dict(db=B[j], kf_id=0, image=img, features=fts[j]) for j in range(2)], ex.prm, THRESHOLD, **kw)
    first = []
    for j in range(2):
        ra = A[j].process_keyframe(V4, 0, img, fts[j], ex.prm, THRESHOLD, **kw)
        same_result(ra, rb[j])
        first.append(A[j].pending())
        same_pending(first[j], B[j].pending())
        A[j].add_pending(); B[j].add_pending()
    assert rb[0]["n_bow"] > 4096 and rb[0]["n_pyramid"] > 4096 and 0 < rb[1]["n_bow"] < 4096, (rb[0]["n_bow"], rb[1]["n_bow"])
    for j in range(2):                                            # some more keyframes sharing words with the first
        kf = first[j]
        m = min(900, len(kf["bow"][0]) // 2)
        for i in range(1, 6):
            pick = np.sort(rng.choice(len(kf["bow"][0]), m, replace=False))
            vals = kf["bow"][1][pick] * rng.uniform(0.7, 1.3, m)
            for db in (A[j], B[j]):
                db.add(i, (kf["bow"][0][pick], vals / vals.sum()), kf["desc"][:50], kf["class_id"][:50])
    # (the single calls above left the ORB plan of one image in force: a call on two scratch databases plans for two again, so that the
    # budget below is the step's own)
    scratch = [sloop.KeyframeDatabase(ctx, keyframes_hint=1) for _ in range(2)]
    sloop.process_keyframe_batch(V4, [dict(db=d, kf_id=0, image=img, features=feats[:10]) for d in scratch], ex.prm, THRESHOLD, **kw)
    rb = sloop.process_keyframe_batch(V4, [dict(db=B[j], kf_id=40, image=img, features=fts[j]) for j in range(2)], ex.prm, THRESHOLD, **kw)
    s = sloop.debug_last_batch(ctx)
    for j in range(2):
        ra = A[j].process_keyframe(V4, 40, img, fts[j], ex.prm, THRESHOLD, **kw)
        same_result(ra, rb[j])
        assert rb[j]["found"] and rb[j]["loop_kf_id"] == 0 and rb[j]["n_scored"] == 6 and rb[j]["n_pairs"] >= 10
        same_pending(A[j].pending(), B[j].pending())
    assert rb[0]["n_bow"] > 4096
    assert s["syncs"] == 2 and s["bytes_down"] <= 16 * 2 + 8 * sum(len(r["pairs"]) for r in rb) + 256, s
    for db in A + B + scratch:
        db.close()
    V4.close()


def test_misuse_touches_nothing(ctx, V, ex, scenes):
    img, feats = scenes[3]
    img2, feats2 = scenes[4]
    kw = dict(pyramid_levels=LEVELS, min_db_size=0, min_id_gap=1)
    A = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(2)]
    B = [sloop.KeyframeDatabase(ctx, keyframes_hint=4) for _ in range(2)]
    fresh = sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    for step, (im, ft) in enumerate(((img, feats), (img2, feats2))):
        jobs = [dict(kf_id=10 * step + j, image=im, features=ft[:150 - 50 * j], commit_pending=step > 0) for j in range(2)]
        sloop.process_keyframe_batch(V, [dict(q, db=B[j]) for j, q in enumerate(jobs)], ex.prm, THRESHOLD, **kw)
        for j, q in enumerate(jobs):
            single(A[j], V, ex.prm, q, **kw)
    before = [(db.size(), db.pending()) for db in B]

    def untouched():
        for db, (size, pend) in zip(B, before):
            assert db.size() == size
            same_pending(pend, db.pending())
        assert len(fresh) == 0
        with pytest.raises(SsxError):
            fresh.pending()

    def rejected(jobs, status=_lib.SSX_ERR_INVALID_ARG, tamper=None, n=None, **over):
        table, res, st, keep, (rows, cols) = sloop.step_job_table(jobs)
        if tamper:
            tamper(table)
        args = dict(kw, **over)
        got = ctx.lib.ssx_kfdb_process_keyframe_batch(V.handle if "voc" not in over else over["voc"].handle, len(jobs) if n is None else n, table, rows, cols,
                                                      C.byref(ex.prm), args["pyramid_levels"], args["min_db_size"], args["min_id_gap"], THRESHOLD, 0)
        assert got == status, (got, status)
        untouched()

    good = lambda j, **o: dict(dict(db=B[j], kf_id=50 + j, image=img, features=feats, commit_pending=True), **o)
    rejected([good(0), good(1)], n=-1)
    rejected([good(0), good(1)], tamper=lambda t: setattr(t[1], "db", None))
    rejected([good(0), good(1)], tamper=lambda t: setattr(t[1], "res", None))
    rejected([good(0), good(1)], tamper=lambda t: setattr(t[0], "status_out", None))
    rejected([good(0), good(1, db=B[0])])                                             # two jobs, one database
    rejected([good(0), good(1), dict(db=fresh, kf_id=0, image=img, features=feats, commit_pending=True)])    # nothing pending there
    rejected([good(0), good(1)], status=_lib.SSX_ERR_UNSUPPORTED, tamper=lambda t: setattr(t[1], "n_features", 8192))   # (rejected before it is read)
    wide = np.zeros((img.shape[0], img.shape[1] + 64), np.uint8)
    wide[:, :img.shape[1]] = img
    rejected([good(0), good(1, image=wide[:, :img.shape[1]])])                        # strides that differ
    other = _lib.Context(0)
    voc = make_vocabulary(k=10, L=3)
    foreign_voc = svoc.Vocabulary.from_arrays(other, 10, 3, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    foreign_db = sloop.KeyframeDatabase(other, keyframes_hint=4)
    rejected([good(0), good(1)], voc=foreign_voc)                                     # a vocabulary of another context
    rejected([good(0), dict(db=foreign_db, kf_id=0, image=img, features=feats)])      # a database of another context
    foreign_db.close(); foreign_voc.close(); other.close()
    # an id that does not ascend: the pending keyframe of a database that already holds a later one
    late = sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    late.process_keyframe(V, 5, img, feats, ex.prm, THRESHOLD, **kw)
    late.add_pending()
    late.process_keyframe(V, 5, img, feats, ex.prm, THRESHOLD, **kw)
    kept = late.pending()
    rejected([good(0), dict(db=late, kf_id=6, image=img, features=feats, commit_pending=True)])
    assert len(late) == 1
    same_pending(kept, late.pending())
    late.close()
    assert sloop.process_keyframe_batch(V, [], ex.prm, THRESHOLD, **kw) == []         # n == 0
    untouched()
    # a valid call follows.  Job 0 revisits its first place with too small a capacity: its status alone, the keyframe pending all the same
    jobs = [dict(kf_id=60, image=img, features=feats, commit_pending=True, pairs_cap=7), dict(kf_id=61, image=img2, features=feats2[:100], commit_pending=True)]
    with pytest.raises(SsxError) as e:
        sloop.process_keyframe_batch(V, [dict(q, db=B[j]) for j, q in enumerate(jobs)], ex.prm, THRESHOLD, **kw)
    assert e.value.status == _lib.SSX_ERR_CAPACITY
    rb = e.value.results
    with pytest.raises(SsxError) as e1:
        single(A[0], V, ex.prm, jobs[0], **kw)
    ra = [e1.value.result, single(A[1], V, ex.prm, jobs[1], **kw)]
    assert rb[0]["status"] == _lib.SSX_ERR_CAPACITY and rb[1]["status"] == 0
    assert ra[0]["found"] and ra[0]["n_pairs"] > 12 and ra[1]["found"]
    for j in range(2):
        same_result(ra[j], rb[j])
        same_pending(A[j].pending(), B[j].pending())
        A[j].add_pending(); B[j].add_pending()
        assert A[j].size() == B[j].size() and len(B[j]) == 3
    A[1].process_keyframe(V, 70, img, feats, ex.prm, THRESHOLD, **kw)
    cur = A[1].pending()
    for j in range(2):
        stored_alike(A[j], B[j], V, ex, [j, 10 + j, 60 + j], cur)
    for db in A + B + [fresh]:
        db.close()
