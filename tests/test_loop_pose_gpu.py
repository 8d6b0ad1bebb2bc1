"""GPU: the pose correction of loop closing -- ssx_pnp_ransac against its model (tools/pnp_model.py) and against ground truth,
ssx_loop_pose_opt against the oracle's composition of OptimizeCurrentPose, ssx_loop_compute_pose against the two chained.
The inputs and what makes them safe to compare are in tests/loop_pose_cases.py and tests/test_pnp_model.py."""
import ctypes as C

import numpy as np
import pytest

import ssvio_amd
from ssvio_amd import ba, loop
from ssvio_amd._lib import SSX_ERR_INVALID_ARG, dbl_p, i32_p, ptr, u8_p
from tools import pnp_model as pm
from tools.synth import make_loop_pose_problem, make_pose_only_problem, pose_inv, pose_mul

import loop_pose_cases as lc

pytestmark = pytest.mark.gpu


def _hooks(ctx):
    loop._bind_pose(ctx.lib)
    ctx.lib.ssx_pnp_debug_samples.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, i32_p]
    ctx.lib.ssx_pnp_debug_counts.argtypes = [C.c_void_p, dbl_p, C.c_int32, dbl_p, dbl_p, C.c_int32, C.c_double, C.c_uint32, i32_p]
    return ctx.lib


def _counts(ctx, p, H, seed):
    out = np.zeros(H, np.int32)
    ctx.check(_hooks(ctx).ssx_pnp_debug_counts(ctx.handle, ptr(p["K"], dbl_p), p["M"], ptr(p["xyz"], dbl_p), ptr(p["uv"], dbl_p), H, lc.THR, seed,
                                               ptr(out, i32_p)))
    return out


def _ransac(ctx, name):
    p = lc.problem(name)
    return p, lc.model(name), loop.pnp_ransac(ctx, p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=lc.CASES[name][4])


@pytest.mark.parametrize("M", [3, 4, 5, 64, 65, 1000])
def test_sample_tap_equals_model(ctx, M):
    for H in (1, 100, 257):
        out = np.full((H, 3), -1, np.int32)
        ctx.check(_hooks(ctx).ssx_pnp_debug_samples(ctx.handle, 7, M, H, ptr(out, i32_p)))
        np.testing.assert_array_equal(out, pm.sample_triples(7, M, H))


@pytest.mark.parametrize("name", [n for n in lc.CASES if n.startswith("clean")])
def test_no_outliers_every_point_is_an_inlier_and_the_first_sound_triple_wins(ctx, name):
    p, m, g = _ransac(ctx, name)
    assert g["found"] and g["n_inliers"] == p["M"] and g["inliers"].all()
    assert g["best"] == m["best"]                             # every sound triple scores M: the lowest hypothesis, then solution, wins
    np.testing.assert_array_equal(_counts(ctx, p, lc.H, lc.CASES[name][4]), m["counts"])
    assert np.abs(g["pose"] - p["gt_pose"]).max() < 1e-3
    assert abs(np.linalg.norm(g["pose"][:4]) - 1) < 1e-14 and g["pose"][3] >= 0


@pytest.mark.parametrize("name", [n for n in lc.CASES if not n.startswith("clean")])
def test_outliers_are_rejected(ctx, name):
    p, m, g = _ransac(ctx, name)
    assert g["found"] == m["found"] is True
    np.testing.assert_array_equal(g["inliers"], m["inliers"])
    if not name.startswith("noisy"):
        np.testing.assert_array_equal(g["inliers"], p["inlier"])
    assert g["n_inliers"] == int(g["inliers"].sum()) == m["n_inliers"]
    assert g["best"] == m["best"]
    assert p["inlier"][list(pm.sample_triple(lc.CASES[name][4], g["best"] >> 2, p["M"]))].all()   # the winner's triple: ground-truth inliers
    np.testing.assert_array_equal(_counts(ctx, p, lc.H, lc.CASES[name][4]), m["counts"])
    np.testing.assert_allclose(g["pose"], m["pose"], rtol=0, atol=1e-12)
    if not name.startswith("noisy"):
        assert max(lc.pose_err(g["pose"], p["gt_pose"])) < lc.gt_bar(name)
    assert abs(np.linalg.norm(g["pose"][:4]) - 1) < 1e-14 and g["pose"][3] >= 0
    again = loop.pnp_ransac(ctx, p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=lc.CASES[name][4])
    assert again["pose"].tobytes() == g["pose"].tobytes() and again["inliers"].tobytes() == g["inliers"].tobytes()


def _compose(po, pr, pose0):
    a = po.pose_only(dict(pr, pose=pose0), rounds=1)
    return po.pose_only(dict(pr, pose=a["pose"]), rounds=4)


@pytest.mark.parametrize("M,pose", lc.REFINE_PARAMS, ids=lc.REFINE_IDS)
def test_loop_pose_opt_matches_oracle_composition(ctx, po, M, pose):
    """OptimizeCurrentPose from the device's own RANSAC pose == pose_only(rounds=1), classification discarded, then
    pose_only(rounds=4) of the oracle from that same pose"""
    p = lc.refine_problem(M, pose)
    r = loop.pnp_ransac(ctx, p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=lc.REFINE_SEED)
    assert r["found"]
    g = loop.loop_pose_opt(ctx, r["pose"], p["K"], p["xyz"], p["uv"])
    o = _compose(po, p, r["pose"])
    assert g["n_inliers"] == o["n_inliers"] == int(g["inliers"].sum())
    np.testing.assert_array_equal(g["inliers"], o["inliers"])
    print("refine", M, pose, "kernel - oracle:", np.abs(g["pose"] - o["pose"]).max(), "bar", lc.refine_bar(M, pose))
    np.testing.assert_allclose(g["pose"], o["pose"], rtol=0, atol=lc.refine_bar(M, pose))   # the bars of test_ba_gpu.py's pose-only tests; lc.REFINE_ORACLE_VS_REF
    if M >= 256:
        eq, et = lc.pose_err(g["pose"], p["gt_pose"])
        assert eq < 5e-3 and et < 5e-3 * lc.x_scale(p)                   # (a rotation error moves t by |X| times it)
    again = loop.loop_pose_opt(ctx, r["pose"], p["K"], p["xyz"], p["uv"])
    assert again["pose"].tobytes() == g["pose"].tobytes() and again["inliers"].tobytes() == g["inliers"].tobytes()


def _pairs(M, seed, n_holes, frac_gross=0.3, gt_pose=None):
    """n = M + n_holes pairs, the holes (expired map points) at the first and the last pair and in between"""
    p = make_loop_pose_problem(M=M, seed=seed, frac_gross=frac_gross, noise_px=0.5, gt_pose=gt_pose)
    n = M + n_holes
    has = np.ones(n, np.uint8)
    has[np.r_[0, n - 1, 1 + np.random.default_rng(seed + 1).permutation(n - 2)[:n_holes - 2]]] = 0
    xyz, uv = np.full((n, 3), np.nan), np.full((n, 2), 1e6)     # what a hole holds must not matter
    xyz[has == 1], uv[has == 1] = p["xyz"], p["uv"]
    uv[has == 0] = np.random.default_rng(seed).uniform(0, 300, (n_holes, 2))
    return p, has, xyz, uv


def _chain(ctx, po, p, has, T_cur, T_loop, seed):
    """ComputeCorrectPose as the two calls and numpy"""
    r = loop.pnp_ransac(ctx, p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=seed)
    g = loop.loop_pose_opt(ctx, r["pose"], p["K"], p["xyz"], p["uv"])
    kept = has.copy()
    kept[has == 1] = g["inliers"]
    err = np.linalg.norm(po.se3_log(pose_mul(T_cur, pose_inv(g["pose"]))))
    return r, g, kept, err, pose_mul(g["pose"], pose_inv(T_loop))


def test_compute_correct_pose_equals_the_chained_calls(ctx, po):
    _compute_correct_pose_equals_the_chained_calls(ctx, po, None)


@pytest.mark.parametrize("pose", list(lc.POSES))
def test_compute_correct_pose_equals_the_chained_calls_away_from_identity(ctx, po, pose):
    _compute_correct_pose_equals_the_chained_calls(ctx, po, pose)


def _compute_correct_pose_equals_the_chained_calls(ctx, po, pose):
    M = 60 if pose is None else 257
    p, has, xyz, uv = _pairs(M, 31, 5, gt_pose=None if pose is None else lc.POSES[pose])
    assert has[0] == 0 and has[-1] == 0 and has.sum() == M
    far = max(1.0, np.abs(p["gt_pose"][4:]).max() / 10.0)                  # products of |t| round at eps |t|: 1 for the scenes near the origin
    T_loop = np.array([0.01, -0.02, 0.03, 1.0, 4.0, -1.0, 2.0])
    T_loop[:4] /= np.linalg.norm(T_loop[:4])
    # |log(T_cur T_corr^-1)| on either side of 1 and of 15 (T_corr is the ground truth to ~1e-3)
    for size, need in ((0.5, False), (2.0, True), (14.0, True), (16.0, False)):
        xi = np.array([0.6, -0.3, 0.7, 0.01, 0.02, -0.01])
        T_cur = pose_mul(po.se3_exp(xi / np.linalg.norm(xi) * size), p["gt_pose"])
        g = loop.compute_correct_pose(ctx, xyz, has, uv, T_cur, T_loop, p["K"], lc.H, seed=6)
        r, o, kept, err, rel = _chain(ctx, po, p, has, T_cur, T_loop, 6)
        assert g["verdict"] == loop.LOOP_OK and g["ok"] and g["n_with_point"] == M
        assert g["n_ransac_inliers"] == r["n_inliers"] and g["best"] == r["best"] and g["n_inliers"] == o["n_inliers"] >= 10
        np.testing.assert_array_equal(g["kept"], kept)
        assert not g["kept"][has == 0].any() and g["kept"].sum() == o["n_inliers"]
        assert g["corrected_pose"].tobytes() == o["pose"].tobytes()             # the same kernels on the same values: the pose never left the device
        assert abs(g["error"] - err) < 1e-12 * far * max(1.0, err) and abs(err - size) < 0.05
        assert g["need_correct"] is need
        np.testing.assert_allclose(g["relative_to_loop"], rel, rtol=0, atol=1e-12 * far)
    again = loop.compute_correct_pose(ctx, xyz, has, uv, T_cur, T_loop, p["K"], lc.H, seed=6)
    assert all(np.asarray(again[k]).tobytes() == np.asarray(g[k]).tobytes() for k in g)


def _frozen(r):
    """a result (dict, or list of dicts) as bytes"""
    if isinstance(r, list):
        return [_frozen(x) for x in r]
    return {k: np.asarray(v).tobytes() for k, v in r.items()}


def test_alternating_calls_on_one_context_equal_first_calls_on_fresh_ones():
    """The pose-only batch and the loop-pose calls keep their pinned blocks apart (the refinement's descriptor lies in the loop-pose
    block, not in the batch's): in whatever order they alternate on one context, each returns the bytes it returns as the first call
    of a fresh context."""
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    p40, has40, xyz40, uv40 = _pairs(35, 41, 5)                              # 40 pairs, 35 with a map point: k_pose_only<2> refines
    p1600 = make_loop_pose_problem(M=1600, seed=42, frac_gross=0.3, noise_px=0.5)   # k_pose_only_generic refines
    batch = [make_pose_only_problem(M=M, seed=50 + M, frac_gross=0.05) for M in (12, 513, 1537)]
    batch.append(dict(pose=ident, K=batch[0]["K"], xyz=np.zeros((0, 3)), uv=np.zeros((0, 2))))
    p200 = make_pose_only_problem(M=200, seed=43, frac_gross=0.05)
    calls = [
        lambda c: loop.compute_correct_pose(c, xyz40, has40, uv40, ident, ident, p40["K"], lc.H, seed=6),
        lambda c: ba.pose_only_opt_batch(c, batch),
        lambda c: loop.compute_correct_pose(c, p1600["xyz"], np.ones(1600, np.uint8), p1600["uv"], ident, ident, p1600["K"], 64, seed=6),
        lambda c: ba.pose_only_opt(c, p200["pose"], p200["K"], p200["xyz"], p200["uv"]),
    ]
    first = []
    for call in calls:
        with ssvio_amd.Context(0) as fresh:
            first.append(_frozen(call(fresh)))
    assert first[0]["verdict"] == first[2]["verdict"] == np.asarray(loop.LOOP_OK).tobytes()       # both refinements ran
    assert first[1][3]["n_inliers"] == np.asarray(0).tobytes() and first[1][3]["pose"] == ident.tobytes()
    with ssvio_amd.Context(0) as one:
        for k in [0, 1, 2, 3, 3, 2, 1, 0]:
            assert _frozen(calls[k](one)) == first[k], k


def test_compute_correct_pose_verdicts(ctx):
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    # 9 pairs with a map point out of 40
    p, has, xyz, uv = _pairs(9, 32, 31, frac_gross=0.0)
    g = loop.compute_correct_pose(ctx, xyz, has, uv, ident, ident, p["K"], lc.H, seed=1)
    assert g["verdict"] == loop.LOOP_FEW_MAP_POINTS and not g["ok"] and g["n_with_point"] == 9
    np.testing.assert_array_equal(g["kept"], has)
    # every pair a wrong match: no pose explains four of them (so says the model, whose counts the kernel's equal)
    p = make_loop_pose_problem(M=40, seed=33, frac_gross=1.0)
    m = pm.pnp_ransac(p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=2)
    assert not m["found"] and m["counts"].max() == 3
    g = loop.compute_correct_pose(ctx, p["xyz"], np.ones(40, np.uint8), p["uv"], ident, ident, p["K"], lc.H, seed=2)
    assert g["verdict"] == loop.LOOP_NO_POSE and g["n_ransac_inliers"] == 0 and g["best"] == -1 and g["kept"].all()
    # a pose that only 7 pairs agree with
    p = make_loop_pose_problem(M=12, seed=31, frac_gross=0.4)
    assert p["inlier"].sum() == 7
    g = loop.compute_correct_pose(ctx, p["xyz"], np.ones(12, np.uint8), p["uv"], ident, ident, p["K"], lc.H, seed=3)
    assert g["verdict"] == loop.LOOP_FEW_INLIERS and g["n_inliers"] == 7 and g["n_ransac_inliers"] == 7
    np.testing.assert_array_equal(g["kept"], p["inlier"])
    assert np.abs(g["corrected_pose"] - p["gt_pose"]).max() < 1e-3


def test_misuse_is_refused_and_the_context_stays_usable(ctx):
    lib = _hooks(ctx)
    p = lc.problem("out30-64")
    K, xyz, uv = p["K"], p["xyz"], p["uv"]
    pose, inl = np.zeros(7), np.zeros(64, np.uint8)
    n, best, found = C.c_int32(), C.c_int32(), C.c_int32()

    def ransac(K=K, M=64, xyz=xyz, uv=uv, H=lc.H, pose=pose, n=C.byref(n), found=C.byref(found), thr=lc.THR):
        return lib.ssx_pnp_ransac(ctx.handle, ptr(K, dbl_p), M, ptr(xyz, dbl_p), ptr(uv, dbl_p), H, thr, 1, ptr(pose, dbl_p), ptr(inl, u8_p), n,
                                  C.byref(best), found)
    bad_K = [K * np.array([1, np.nan, 1, 1]), K * np.array([np.inf, 1, 1, 1])]
    for kw in (dict(M=-1), dict(K=None), dict(xyz=None), dict(uv=None), dict(pose=None), dict(n=None), dict(found=None), dict(H=0), dict(H=-5),
               dict(H=loop.PNP_MAX_ITERS + 1), dict(K=bad_K[0]), dict(K=bad_K[1]), dict(thr=float("nan")), dict(thr=-1.0)):
        assert ransac(**kw) == SSX_ERR_INVALID_ARG, kw
    for M in (0, 1, 2):                                                     # no triple to draw: not an error
        assert ransac(M=M) == 0 and found.value == 0 and n.value == 0
    assert lib.ssx_pnp_ransac(ctx.handle, ptr(K, dbl_p), 0, None, None, lc.H, lc.THR, 1, ptr(pose, dbl_p), None, C.byref(n), None, C.byref(found)) == 0
    assert ransac(H=loop.PNP_MAX_ITERS) == 0 and found.value == 1          # the cap itself is allowed
    for kw in (dict(pose=None), dict(K=None), dict(M=-1), dict(xyz=None), dict(uv=None), dict(K=bad_K[0])):
        a = dict(pose=pose, K=K, M=64, xyz=xyz, uv=uv)
        a.update(kw)
        assert lib.ssx_loop_pose_opt(ctx.handle, ptr(a["pose"], dbl_p), ptr(a["K"], dbl_p), a["M"], ptr(a["xyz"], dbl_p), ptr(a["uv"], dbl_p), 5.991, 1.0,
                                     None, None) == SSX_ERR_INVALID_ARG, kw
    res, kept, has = loop.LoopPoseResult(), np.zeros(64, np.uint8), np.ones(64, np.uint8)
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    for kw in (dict(n=-1), dict(xyz=None), dict(has=None), dict(uv=None), dict(Tc=None), dict(Tl=None), dict(K=None), dict(K=bad_K[1]), dict(H=0),
               dict(H=loop.PNP_MAX_ITERS + 1), dict(kept=None), dict(res=None)):
        a = dict(n=64, xyz=xyz, has=has, uv=uv, Tc=ident, Tl=ident, K=K, H=lc.H, kept=kept, res=C.byref(res))
        a.update(kw)
        assert lib.ssx_loop_compute_pose(ctx.handle, a["n"], ptr(a["xyz"], dbl_p), ptr(a["has"], u8_p), ptr(a["uv"], dbl_p), ptr(a["Tc"], dbl_p),
                                         ptr(a["Tl"], dbl_p), ptr(a["K"], dbl_p), a["H"], 1, ptr(a["kept"], u8_p), a["res"]) == SSX_ERR_INVALID_ARG, kw
    assert lib.ssx_pnp_debug_samples(ctx.handle, 1, 2, 10, ptr(np.zeros(30, np.int32), i32_p)) == SSX_ERR_INVALID_ARG
    # a correct call afterwards still answers
    g = loop.pnp_ransac(ctx, K, xyz, uv, lc.H, lc.THR, seed=lc.CASES["out30-64"][4])
    np.testing.assert_array_equal(g["inliers"], p["inlier"])
    e = loop.compute_correct_pose(ctx, xyz[:0], has[:0], uv[:0], ident, ident, K)
    assert e["verdict"] == loop.LOOP_FEW_MAP_POINTS and len(e["kept"]) == 0
