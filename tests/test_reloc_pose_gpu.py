"""GPU: ssx_pnp_pose_batch (k_pnp_ransac_jobs, then one launch of the pose-only refinement per kernel class) against the single calls it
batches: per job, bit for bit, ssx_pnp_ransac and -- where that found a pose -- ssx_loop_pose_opt from it, whatever the size of the
table and wherever the job stands in it.  Those single calls are held to tools/pnp_model.py and to the oracle in test_loop_pose_gpu.py."""
import numpy as np
import pytest

from ssvio_amd import _lib, loop
from ssvio_amd._lib import SsxError
from tools.synth import make_loop_pose_problem

pytestmark = pytest.mark.gpu

H, THR = 100, 5.991                                             # the reference's 100 hypotheses and its pixel threshold
# M: no triple (0, 2), a triple and nothing else (3), the smallest that can be found (4), and the three classes of the refinement:
# up to 512 edges (37, 300), up to 1536 (600), beyond (1700)
SIZES = (0, 2, 3, 4, 37, 300, 600, 1700)


def make_job(M, k):
    """job k of size M: 40 % wrong matches, or nothing but wrong matches for every third"""
    p = make_loop_pose_problem(M=M, seed=50 + M, frac_gross=1.0 if k % 3 == 2 else 0.4)
    return dict(xyz=p["xyz"], uv=p["uv"], seed=1000 + 17 * k, K=p["K"])


@pytest.fixture(scope="module")
def pool(ctx):
    """64 jobs, the eight sizes in turn, and what the single calls give for each (computed once, never changed)"""
    jobs = [make_job(SIZES[k % 8], k) for k in range(64)]
    K = jobs[0]["K"]
    want = []
    for q in jobs:
        r = loop.pnp_ransac(ctx, K, q["xyz"], q["uv"], H, THR, seed=q["seed"])
        w = dict(found=r["found"], n_ransac_inliers=r["n_inliers"], best=r["best"], pose=np.array([0, 0, 0, 1.0, 0, 0, 0]),
                 inliers=np.zeros(len(q["xyz"]), np.uint8), n_inliers=0)
        if r["found"]:
            o = loop.loop_pose_opt(ctx, r["pose"], K, q["xyz"], q["uv"])
            w.update(pose=o["pose"], inliers=o["inliers"].copy(), n_inliers=o["n_inliers"])
        want.append(w)
    return K, jobs, want


def same_job(got, want, where):
    for key in ("found", "n_ransac_inliers", "best", "n_inliers"):
        assert got[key] == want[key], (where, key, got[key], want[key])
    assert got["pose"].tobytes() == want["pose"].tobytes(), (where, got["pose"], want["pose"])
    assert got["inliers"].tobytes() == want["inliers"].tobytes(), where


def test_the_pool_covers_what_it_should(pool):
    K, jobs, want = pool
    sizes = [len(q["xyz"]) for q in jobs]
    assert not any(w["found"] for w, m in zip(want, sizes) if m < 4)               # fewer than 4 points: nothing to find
    assert any(not w["found"] for w, m in zip(want, sizes) if m >= 4)              # nothing but wrong matches: a job with points and no pose
    for k, (w, m) in enumerate(zip(want, sizes)):
        if m >= 37 and k % 3 != 2:                                                 # 60 % true matches: found, and refined to a real pose
            assert w["found"] and w["n_inliers"] >= m // 2 and w["n_inliers"] == int(w["inliers"].sum()), (k, m, w["n_inliers"])
    assert {loop.PNP_BATCH_MAX, len(jobs)} == {64}


@pytest.mark.parametrize("idx", [[4], [7], [3], [0], [4, 6, 7], list(range(8)), list(range(64))], ids=["n1_class0", "n1_generic", "n1_m4", "n1_empty", "n3", "n8", "n64"])
def test_every_job_equals_the_single_calls(ctx, pool, idx):
    K, jobs, want = pool
    got = loop.pnp_pose_batch(ctx, K, [jobs[i] for i in idx], H, THR)
    assert len(got) == len(idx)
    for g, i in zip(got, idx):
        same_job(g, want[i], i)


def test_a_job_does_not_depend_on_its_place_in_the_table(ctx, pool):
    K, jobs, want = pool
    rng = np.random.default_rng(3)
    for idx in (list(range(8))[::-1], list(rng.permutation(16)), list(rng.permutation(64))[:23]):
        got = loop.pnp_pose_batch(ctx, K, [jobs[i] for i in idx], H, THR)
        for g, i in zip(got, idx):
            same_job(g, want[i], i)
    # the same job twice in one table
    got = loop.pnp_pose_batch(ctx, K, [jobs[5], jobs[6], jobs[5]], H, THR)
    same_job(got[0], want[5], 5); same_job(got[2], want[5], 5); same_job(got[1], want[6], 6)


def test_the_launch_count_does_not_depend_on_n(ctx, pool):
    K, jobs, want = pool

    def launches(idx):
        _lib.profile_begin(ctx)
        loop.pnp_pose_batch(ctx, K, [jobs[i] for i in idx], H, THR)
        prof = _lib.profile_end(ctx)
        return {name: calls for name, (calls, ms) in prof.items()}

    few, many = launches([4, 6, 7]), launches(list(range(64)))               # both hold all three classes of the refinement
    assert few == many == {"k_pnp_ransac": 1, "k_pose_only": 3}, (few, many)
    assert launches([4, 5]) == {"k_pnp_ransac": 1, "k_pose_only": 1}          # one class: one launch of the refinement
    assert launches([0, 1]) == {}                                             # no triple anywhere: nothing runs


def test_misuse_and_empty_calls(ctx, pool):
    K, jobs, want = pool
    assert loop.pnp_pose_batch(ctx, K, [], H, THR) == []
    for kw in (dict(max_iters=0), dict(max_iters=loop.PNP_MAX_ITERS + 1), dict(reproj_px=-1.0), dict(reproj_px=float("nan"))):
        with pytest.raises(SsxError) as e:
            loop.pnp_pose_batch(ctx, K, [jobs[4]], **dict(dict(max_iters=H, reproj_px=THR), **kw))
        assert e.value.status == _lib.SSX_ERR_INVALID_ARG, kw
    with pytest.raises(SsxError) as e:
        loop.pnp_pose_batch(ctx, np.array([700.0, 700.0, float("inf"), 180.0]), [jobs[4]], H, THR)
    assert e.value.status == _lib.SSX_ERR_INVALID_ARG
    with pytest.raises(SsxError) as e:
        loop.pnp_pose_batch(ctx, K, [jobs[0]] * 65, H, THR)
    assert e.value.status == _lib.SSX_ERR_INVALID_ARG
    # a null array in a job with points, and a null table, through the C entry point itself
    table = (loop.PnpPoseJob * 2)()
    table[0].M = 5
    assert ctx.lib.ssx_pnp_pose_batch(ctx.handle, _lib.ptr(K, _lib.dbl_p), 1, table, H, THR, 5.991, 1.0) == _lib.SSX_ERR_INVALID_ARG
    assert ctx.lib.ssx_pnp_pose_batch(ctx.handle, _lib.ptr(K, _lib.dbl_p), 1, None, H, THR, 5.991, 1.0) == _lib.SSX_ERR_INVALID_ARG
    assert ctx.lib.ssx_pnp_pose_batch(ctx.handle, None, 1, table, H, THR, 5.991, 1.0) == _lib.SSX_ERR_INVALID_ARG
    # the single entry points are what they were
    same_job(loop.pnp_pose_batch(ctx, K, [jobs[6]], H, THR)[0], want[6], 6)
