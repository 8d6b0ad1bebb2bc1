"""GPU: the candidate query of several databases in one call (ssx_kfdb_relocalize_query_batch: the job-indexed k_kfdb_topk behind the
job table's chain, the match kernels once over n x K jobs) against the single calls it replaces, ssx_kfdb_add_pending +
ssx_kfdb_relocalize_query per database.  Of a twin, database A takes the single calls and B the batch; every comparison is on bytes.
The frame, the vocabulary and the synthetic keyframes are those of test_reloc_query_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from ssvio_amd import _lib
from ssvio_amd import loop as sloop
from ssvio_amd._lib import KP_DTYPE, SsxError
from test_loop_keyframe_gpu import same_contents, same_keyframe, same_result
from test_reloc_query_gpu import ANY_ID, LEVELS, SETTINGS, Twin, V, ex, expand, frame, same_query, synthetic_keyframe  # noqa: F401 (V, ex, frame: fixtures)
from tools.synth import make_stereo_pair

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 9, 257, 1030)


@pytest.fixture(scope="module")
def kfs(frame):
    rng = np.random.default_rng(77)
    return [synthetic_keyframe(rng, frame) for _ in range(max(SIZES))]


def make_twin(ctx, kfs, n):
    t = Twin(ctx)
    for i in range(n):
        t.add(3 * i + 3, *kfs[i])
    return t


@pytest.fixture(scope="module")
def twins(ctx, kfs):
    """one twin per size of SIZES, each a prefix of the same 1030 synthetic keyframes, and one more of a single keyframe ("none": the
    database of the job that comes without features)"""
    out = {n: make_twin(ctx, kfs, n) for n in SIZES}
    out["none"] = make_twin(ctx, kfs, 1)
    yield out
    for t in out.values():
        t.close()


def single(db, V, ex, frame, K, threshold, ratio, feats=None, **kw):
    return db.relocalize_query(V, frame["img"], frame["feats"] if feats is None else feats, ex.prm, max_candidates=K, threshold=threshold, ratio=ratio,
                               pyramid_levels=LEVELS, **kw)


def job(db, frame, feats=None, **kw):
    return dict(db=db, image=frame["img"], features=frame["feats"] if feats is None else feats, **kw)


def batch(V, ex, jobs, K, threshold, ratio):
    return sloop.relocalize_query_batch(V, jobs, ex.prm, max_candidates=K, threshold=threshold, ratio=ratio, pyramid_levels=LEVELS)


def same_job(want, got):
    same_query(want, got)
    assert got["status"] == _lib.SSX_OK


def same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        same_query(x, y)
        assert x["status"] == y["status"]


@pytest.mark.parametrize("n", SIZES)
def test_one_job_equals_the_single_query(twins, V, ex, frame, n):
    t = twins[n]
    seen = []
    for K, threshold, ratio in SETTINGS:
        want = single(t.A, V, ex, frame, K, threshold, ratio)
        got, = batch(V, ex, [job(t.B, frame)], K, threshold, ratio)
        same_job(want, got)
        assert got["n_scored"] == n
        seen.append(len(got["candidates"]))
    if n >= 257:
        assert seen[0] == 1 and seen[2] == 8                    # the cases are not vacuous
    if n == 0:
        assert seen == [0] * len(SETTINGS)


def mixed(twins, frame):
    order = (1030, 0, 9, 257, "none")
    return order, [job(twins[k].B, frame, feats=frame["feats"][:0] if k == "none" else None) for k in order]


def test_a_mixed_table_and_the_same_table_reversed(twins, V, ex, frame):
    order, jobs = mixed(twins, frame)
    for K, threshold, ratio in ((8, 0.0, 0.0), (4, 0.0, 0.75)):
        want = [single(twins[k].A, V, ex, frame, K, threshold, ratio, feats=frame["feats"][:0] if k == "none" else None) for k in order]
        got = batch(V, ex, jobs, K, threshold, ratio)
        for w, g in zip(want, got):
            same_job(w, g)
        back = batch(V, ex, jobs[::-1], K, threshold, ratio)
        same_bytes(got, back[::-1])
        assert [len(g["candidates"]) for g in got][1] == 0 and got[4]["candidates"] == [] and got[4]["n_pyramid"] == 0 and got[4]["n_scored"] == 1
        assert len(got[0]["candidates"]) == K and len(got[3]["candidates"]) == K and len(got[2]["candidates"]) >= 1


def test_candidates_without_descriptors_and_the_global_sort_beside_a_small_job(ctx, twins, V, ex, frame):
    """the construction of test_candidates_without_descriptors_and_one_beyond_the_lds_sort in one call beside the 9-keyframe job: the two
    jobs' scratch differs (one needs the global sort scratch, one does not)"""
    rng = np.random.default_rng(6)
    t = Twin(ctx)
    q_ids, q_vals = frame["bow"]
    t.add(1, *synthetic_keyframe(rng, frame))
    t.add(2, (q_ids, q_vals))                                    # the best score, no descriptors
    t.add(3, (q_ids[::2], q_vals[::2] / q_vals[::2].sum()), np.zeros((0, 32), np.uint8), np.zeros(0, np.int32))
    many = frame["desc"][rng.integers(0, len(frame["desc"]), 5000)]
    t.add(4, (q_ids[1::2], q_vals[1::2] / q_vals[1::2].sum()), many, np.arange(5000, dtype=np.int32))
    t.add(5, *synthetic_keyframe(rng, frame))
    want = [single(t.A, V, ex, frame, 8, 0.0, 0.0), single(twins[9].A, V, ex, frame, 8, 0.0, 0.0)]
    for jobs, w in (([job(t.B, frame), job(twins[9].B, frame)], want), ([job(twins[9].B, frame), job(t.B, frame)], want[::-1])):
        got = batch(V, ex, jobs, 8, 0.0, 0.0)
        for a, b in zip(w, got):
            same_job(a, b)
    by_id = {c["kf_id"]: c for c in got[1]["candidates"]}
    assert got[1]["candidates"][0]["kf_id"] == 2 and by_id[2]["no_descriptors"] and by_id[2]["n_pairs"] == 0 and by_id[2]["min_distance"] == -1
    assert not by_id[3]["no_descriptors"] and by_id[3]["n_pairs"] == 0 and by_id[3]["min_distance"] == -1
    assert by_id[4]["n_pairs"] > 4096 and by_id[4]["min_distance"] == 0
    assert by_id[1]["n_pairs"] > 0 and by_id[5]["n_pairs"] > 0
    t.close()


# the layout of a stored keyframe (the top of csrc/loop.hip) and how arena and table grow (grow_keep), to place a commit at a growth
def blob_bytes(n_bow, n_desc):
    vals = (n_bow * 4 + 7) & ~7
    cls = vals + n_bow * 8
    desc = (cls + n_desc * 4 + 31) & ~31
    return (desc + n_desc * 32 + 31) & ~31


def capacity_after(cap, need):
    cap = max(cap, 4096)
    while cap < need:
        cap *= 2
    return cap


def other_image(po, seed=141):
    img = make_stereo_pair(seed=seed, h=200, w=320, n_blobs=400)[0]
    return img, po.orb_detect(img, prm=po.orb_params(nfeatures=150))


def test_a_job_commits_its_pending_keyframe_inside_the_call(ctx, po, kfs, twins, V, ex, frame):
    """256 stored keyframes fill the table of a database made with keyframes_hint=4 (4096 bytes of 16-byte rows), and the last of them
    is sized so that the arena has less room than the pending keyframe needs: the commit grows both, each with its own synchronisation"""
    t = Twin(ctx)
    rng = np.random.default_rng(9)
    used, cap = 0, capacity_after(0, 4 * 49152)                  # (ssx_kfdb_create asks for 48 KB per hinted keyframe)
    for i in range(255):
        bow, desc, cls = kfs[i]
        t.add(3 * i + 3, bow, desc, cls)
        used += blob_bytes(len(bow[0]), len(desc))
        cap = capacity_after(cap, used)
    bow = kfs[255][0]
    nd = max(d for d in range(0, 20000) if used + blob_bytes(len(bow[0]), d) <= cap - 2048)
    t.add(3 * 255 + 3, bow, rng.integers(0, 256, (nd, 32), dtype=np.uint8), rng.integers(0, 500, nd).astype(np.int32))
    used += blob_bytes(len(bow[0]), nd)
    assert cap - used < 4096 and len(t.A) == 256
    # the pending keyframe is made from the query image itself: the best candidate there is
    for db in (t.A, t.B):
        db.process_keyframe(V, 5000, frame["img"], frame["feats"], ex.prm, 0.6, pyramid_levels=LEVELS)
    pend = t.B.pending()
    assert blob_bytes(len(pend["bow"][0]), len(pend["desc"])) > cap - used
    # a job without commit beside it: the nine keyframes of twins[9] and a pending keyframe that stays
    side = sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    for i in range(9):
        side.add(3 * i + 3, *kfs[i])
    img2, feats2 = other_image(po)
    side.process_keyframe(V, 1000, img2, feats2, ex.prm, 0.6, pyramid_levels=LEVELS)
    before = side.pending()
    t.A.add_pending()
    want = [single(t.A, V, ex, frame, 8, 0.0, 0.0), single(twins[9].A, V, ex, frame, 8, 0.0, 0.0)]
    batch(V, ex, [job(twins[9].B, frame), job(twins[1].B, frame)], 8, 0.0, 0.0)     # (the single calls planned one image: plan two again)
    got = batch(V, ex, [job(t.B, frame, commit_pending=True), job(side, frame)], 8, 0.0, 0.0)
    stats = sloop.debug_last_batch(ctx)
    same_job(want[0], got[0])
    same_job(want[1], got[1])
    assert stats["syncs"] == 3, stats                            # the arena, the table, the call
    assert got[0]["n_scored"] == 257 and got[0]["candidates"][0]["kf_id"] == 5000 and got[0]["candidates"][0]["row"] == 256
    assert got[0]["candidates"][0]["min_distance"] == 0 and got[0]["candidates"][0]["n_pairs"] >= 10
    same_contents(t.A, t.B, ANY_ID, frame["bow"])
    assert t.A.size() == t.B.size() and len(t.B) == 257
    with pytest.raises(SsxError):
        t.B.pending()                                            # nothing is pending, as after add_pending
    with pytest.raises(SsxError):
        t.B.add_pending()
    # the committed keyframe is what was pending
    pa, pb = t.A.match_features(5000, pend["desc"], pend["class_id"]), t.B.match_features(5000, pend["desc"], pend["class_id"])
    assert pa[0].tobytes() == pb[0].tobytes() and pa[1] == pb[1] == 0 and len(pb[0]) >= 10
    # the job beside it kept its pending keyframe
    after = side.pending()
    same_keyframe(before, after)
    assert len(side) == 9 and len(after["desc"]) > 0
    # and the databases go on alike
    ra = t.A.process_keyframe(V, 6000, img2, feats2, ex.prm, 0.0, pyramid_levels=LEVELS)
    rb = t.B.process_keyframe(V, 6000, img2, feats2, ex.prm, 0.0, pyramid_levels=LEVELS)
    same_result(ra, rb)
    same_keyframe(t.A.pending(), t.B.pending())
    # a second query, now against 257 stored keyframes and without a commit
    same_job(single(t.A, V, ex, frame, 4, 0.0, 0.75), batch(V, ex, [job(t.B, frame)], 4, 0.0, 0.75)[0])
    side.close(); t.close()


def test_budget_is_independent_of_n_of_K_and_of_the_databases(ctx, po, kfs, twins, V, ex, frame):
    """launches and synchronisations (ssx_kfdb_debug_last_batch) after a warm-up call of the shape: equal for n = 1, 2 and 5, for K = 1 and
    8, for 9 and 1030 stored keyframes; ONE synchronisation; a commit without growth adds its launch and no synchronisation"""
    tables = {(1, 9): [9], (1, 1030): [1030], (2, 9): [9, 257], (5, 9): [9, 1030, 257, 1, 0]}
    batch(V, ex, [job(twins[k].B, frame) for k in tables[5, 9]], 8, 0.0, 0.0)      # the largest shape is planned; smaller calls run on it
    stats = {}
    for key, sizes in tables.items():
        for K in (1, 8):
            jobs = [job(twins[k].B, frame) for k in sizes]
            batch(V, ex, jobs, K, 0.0, 0.0)
            r = batch(V, ex, jobs, K, 0.0, 0.0)
            stats[key, K] = sloop.debug_last_batch(ctx)
            assert 1 <= len(r[0]["candidates"]) <= K
    first = stats[(1, 9), 1]
    for key, s in stats.items():
        assert s["launches"] == first["launches"] and s["syncs"] == first["syncs"] == 1, (key, s, first)
    assert 0 < first["launches"] <= 24
    # what comes down: the result blocks, the pair counts and the pairs
    r = batch(V, ex, [job(twins[k].B, frame) for k in tables[5, 9]], 8, 0.0, 0.0)
    s = sloop.debug_last_batch(ctx)
    assert s["bytes_down"] <= 5 * 256 + sum(8 + 8 * c["n_pairs"] for q in r for c in q["candidates"])
    # a commit without growth
    db = sloop.KeyframeDatabase(ctx, keyframes_hint=256)
    for i in range(9):
        db.add(3 * i + 3, *kfs[i])
    db.process_keyframe(V, 5000, frame["img"], frame["feats"], ex.prm, 0.6, pyramid_levels=LEVELS)
    batch(V, ex, [job(db, frame), job(twins[9].B, frame)], 8, 0.0, 0.0)            # (the single step planned one image: plan two again)
    got = batch(V, ex, [job(db, frame, commit_pending=True), job(twins[9].B, frame)], 8, 0.0, 0.0)
    s = sloop.debug_last_batch(ctx)
    assert s["launches"] == first["launches"] + 1 and s["syncs"] == 1, (s, first)
    assert got[0]["n_scored"] == 10 and got[0]["candidates"][0]["kf_id"] == 5000
    db.close()


def test_capacity_is_one_jobs_status(twins, V, ex, frame):
    full = batch(V, ex, [job(twins[k].B, frame) for k in (9, 257, 1030)], 8, 0.0, 0.0)
    counts = [c["n_pairs"] for c in full[1]["candidates"]]
    cap = max(counts) - 1
    assert cap >= 1 and min(counts) <= cap                       # some candidate fits, some does not
    with pytest.raises(SsxError) as e:
        batch(V, ex, [job(twins[9].B, frame), job(twins[257].B, frame, pairs_cap=cap), job(twins[1030].B, frame)], 8, 0.0, 0.0)
    assert e.value.status == _lib.SSX_ERR_CAPACITY
    part = e.value.results
    assert [q["status"] for q in part] == [_lib.SSX_OK, _lib.SSX_ERR_CAPACITY, _lib.SSX_OK]
    same_query(full[0], part[0]); same_query(full[2], part[2])
    assert [c["n_pairs"] for c in part[1]["candidates"]] == counts   # every count is true
    for a, b in zip(full[1]["candidates"], part[1]["candidates"]):
        assert a["kf_id"] == b["kf_id"] and a["min_distance"] == b["min_distance"]
        assert b["pairs"].tobytes() == a["pairs"][:cap].tobytes()
    ok = batch(V, ex, [job(twins[257].B, frame, pairs_cap=max(counts))], 8, 0.0, 0.0)
    same_query(full[1], ok[0])


def test_misuse_is_rejected_and_leaves_every_database_as_it_was(ctx, po, kfs, twins, V, ex, frame):
    from ssvio_amd import voc as svoc
    from tools.synth import make_vocabulary
    a, b = twins[9].B, twins[257].B
    # p: a pending keyframe whose id ascends; low: one whose id does not
    p, low = sloop.KeyframeDatabase(ctx, keyframes_hint=4), sloop.KeyframeDatabase(ctx, keyframes_hint=4)
    for db in (p, low):
        for i in range(3):
            db.add(3 * i + 3, *kfs[i])
    img2, feats2 = other_image(po)
    p.process_keyframe(V, 1000, img2, feats2, ex.prm, 0.6, pyramid_levels=LEVELS)
    low.process_keyframe(V, 9, img2, feats2, ex.prm, 0.6, pyramid_levels=LEVELS)
    dbs = (a, b, p, low)
    state = lambda: [(d.size(), single(d, V, ex, frame, 8, 0.0, 0.0)) for d in dbs]
    pend = lambda: [d.pending() for d in (p, low)]
    before, pend_before = state(), pend()

    def status_of(call):
        with pytest.raises(SsxError) as e:
            call()
        return e.value.status

    good = [job(a, frame), job(p, frame, commit_pending=True), job(b, frame)]
    for kw in (dict(K=0), dict(K=9), dict(K=-1), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(ratio=-0.01), dict(ratio=1.01),
               dict(threshold=-0.01), dict(threshold=float("nan"))):
        s = dict(dict(K=4, threshold=0.0, ratio=0.75), **kw)
        assert status_of(lambda: batch(V, ex, good, s["K"], s["threshold"], s["ratio"])) == _lib.SSX_ERR_INVALID_ARG, kw
    assert status_of(lambda: sloop.relocalize_query_batch(V, good, ex.prm, pyramid_levels=0)) == _lib.SSX_ERR_INVALID_ARG
    # two jobs with one database; commit_pending with nothing pending; an id that does not ascend
    assert status_of(lambda: batch(V, ex, [job(a, frame), job(p, frame, commit_pending=True), job(a, frame)], 4, 0.0, 0.75)) == _lib.SSX_ERR_INVALID_ARG
    assert status_of(lambda: batch(V, ex, [job(p, frame, commit_pending=True), job(a, frame, commit_pending=True)], 4, 0.0, 0.75)) == _lib.SSX_ERR_INVALID_ARG
    assert status_of(lambda: batch(V, ex, [job(p, frame, commit_pending=True), job(low, frame, commit_pending=True)], 4, 0.0, 0.75)) == _lib.SSX_ERR_INVALID_ARG
    # differing strides: the same image as a view of a wider array
    wide = np.zeros((frame["img"].shape[0], frame["img"].shape[1] + 64), np.uint8)
    wide[:, :frame["img"].shape[1]] = frame["img"]
    view = wide[:, :frame["img"].shape[1]]
    assert status_of(lambda: batch(V, ex, [job(p, frame, commit_pending=True), dict(db=a, image=view, features=frame["feats"])], 4, 0.0, 0.75)) == _lib.SSX_ERR_INVALID_ARG
    # more than 65535 pyramid keypoints
    assert status_of(lambda: batch(V, ex, [job(p, frame, commit_pending=True), job(a, frame, feats=np.zeros(8192, KP_DTYPE))], 4, 0.0, 0.75)) == _lib.SSX_ERR_UNSUPPORTED
    # a database of another context
    other = _lib.Context(0)
    foreign = sloop.KeyframeDatabase(other, keyframes_hint=4)
    assert status_of(lambda: batch(V, ex, [job(p, frame, commit_pending=True), job(foreign, frame)], 4, 0.0, 0.75)) == _lib.SSX_ERR_INVALID_ARG
    foreign.close(); other.close()
    # null required pointers and a negative n, through the C entry point itself
    lib, img, feats = ctx.lib, frame["img"], np.ascontiguousarray(frame["feats"], dtype=KP_DTYPE)
    res, status, pairs = (sloop.RelocQueryResult * 2)(), (C.c_int32 * 2)(), np.zeros((2, 4, 64, 2), np.int32)

    def table(**bad):
        t = (sloop.RelocQueryJob * 2)()
        for j, db in enumerate((p, a)):
            t[j] = sloop.RelocQueryJob(db.handle, img.ctypes.data, img.strides[0], len(feats), feats.ctypes.data, 1 if j == 0 else 0, 64,
                                       _lib.ptr(pairs[j], _lib.i32_p), C.pointer(res[j]), C.cast(C.byref(status, 4 * j), _lib.i32_p))
        for key, val in bad.items():
            setattr(t[1], key, val)
        return t

    call = lambda voc, n, t, prm=C.byref(ex.prm): lib.ssx_kfdb_relocalize_query_batch(voc, n, t, img.shape[0], img.shape[1], prm, LEVELS, 4, 0.0, 0.75, 0)
    for bad in (dict(db=None), dict(img=None), dict(features=None), dict(pairs_out=None), dict(res=None), dict(status_out=None), dict(stride=img.shape[1] - 1),
                dict(n_features=-1), dict(pairs_cap=-1)):
        assert call(V.handle, 2, table(**bad)) == _lib.SSX_ERR_INVALID_ARG, bad
    assert call(None, 2, table()) == _lib.SSX_ERR_INVALID_ARG
    assert call(V.handle, 2, None) == _lib.SSX_ERR_INVALID_ARG
    assert call(V.handle, 2, table(), None) == _lib.SSX_ERR_INVALID_ARG
    assert call(V.handle, -1, table()) == _lib.SSX_ERR_INVALID_ARG
    # nothing was touched: the stored keyframes, the queries' answers and the pending keyframes
    after, pend_after = state(), pend()
    for (sa, qa), (sb, qb) in zip(before, after):
        assert sa == sb
        same_query(qa, qb)
    for x, y in zip(pend_before, pend_after):
        same_keyframe(x, y)
    # and the table that was refused nine times over is served
    got = batch(V, ex, good, 4, 0.0, 0.75)
    assert [g["status"] for g in got] == [0, 0, 0] and got[1]["n_scored"] == 4
    p.close(); low.close()


def test_two_calls_write_the_same_bytes(twins, V, ex, frame):
    _, jobs = mixed(twins, frame)
    a = batch(V, ex, jobs, 8, 0.0, 0.5)
    b = batch(V, ex, jobs, 8, 0.0, 0.5)
    same_bytes(a, b)
    assert len(a[0]["candidates"]) >= 2
