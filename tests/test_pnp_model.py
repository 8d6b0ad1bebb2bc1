"""CPU: tools/pnp_model.py, the contract of ssx_pnp_ransac (cv::solvePnPRansac itself cannot be pinned: SURVEY.md section 0, item 4),
checked against inputs with ground truth; the refinement of OptimizeCurrentPose as a composition of the pinned pose-only oracle;
and the conditions on the inputs that tests/test_loop_pose_gpu.py relies on."""
import numpy as np
import pytest

from tools import pnp_model as pm

import loop_pose_cases as lc

CLEAN = [n for n in lc.CASES if not n.startswith("noisy")]


@pytest.mark.parametrize("M", [3, 4, 5, 64, 65, 1000])
def test_samples_are_distinct_in_range_and_reproducible(M):
    t = pm.sample_triples(7, M, 257)
    assert t.shape == (257, 3) and t.min() >= 0 and t.max() < M
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    assert np.array_equal(t, pm.sample_triples(7, M, 257))
    assert np.array_equal(t[:100], pm.sample_triples(7, M, 100))          # hypothesis h does not depend on H
    if M > 3:
        assert not np.array_equal(t, pm.sample_triples(8, M, 257))
    else:                                                                 # three points: every triple is a permutation of all of them
        assert (np.sort(t, axis=1) == np.arange(3)).all()
    if M >= 64:                                                           # every index is reached, in every position
        for k in range(3):
            assert len(np.unique(pm.sample_triples(7, M, 4096)[:, k])) > min(M, 4096) * 0.6


def test_p3p_returns_the_true_pose_among_its_solutions():
    p = lc.problem("clean-64")
    from tools.synth import quat_rot
    hit = 0
    for h in range(40):
        tri = list(pm.sample_triple(11, h, 64))
        valid, Rs, ts = pm.p3p(p["K"], p["xyz"][tri], p["uv"][tri])
        assert valid.any(), h
        err = []
        for s in np.nonzero(valid)[0]:
            Rt = np.stack([quat_rot(p["gt_pose"][:4], e) for e in np.eye(3)], 1)
            err.append(max(np.abs(Rs[s] - Rt).max(), np.abs(ts[s] - p["gt_pose"][4:]).max()))
            assert np.abs(Rs[s] @ Rs[s].T - np.eye(3)).max() < 1e-6       # a rotation
        hit += min(err) < 1e-3                                            # (float32 pixels: ~1e-5 px of "noise")
    assert hit == 40


def test_degenerate_triples_give_no_solution_and_no_nan():
    K = lc.problem("clean-10")["K"]
    X = np.array([[0.0, 0, 10], [1, 0, 10], [2, 0, 10]])
    uv = np.array([[600.0, 180], [670, 180], [740, 180]])
    for Xd, uvd in ((X, uv),                                             # collinear points
                    (X[[0, 0, 1]], uv[[0, 0, 1]]),                       # a repeated point
                    (np.array([[0.0, 0, 10], [1, 1, 10], [0, 2, 12]]), uv[[0, 0, 0]]),   # one bearing three times
                    (X * np.nan, uv)):
        valid, Rs, ts = pm.p3p(K, Xd, uvd)
        assert not valid.any() and np.isfinite(Rs).all() and np.isfinite(ts).all()
    r = pm.pnp_ransac(K, X, uv, 20, lc.THR, seed=0)
    assert not r["found"] and r["n_inliers"] == 0 and (r["counts"] == 0).all()
    assert not pm.pnp_ransac(K, X[:2], uv[:2], 20, lc.THR)["found"]       # M < 3


@pytest.mark.parametrize("name", CLEAN)
def test_model_recovers_the_ground_truth_mask(name):
    p, m = lc.problem(name), lc.model(name)
    n_in = int(p["inlier"].sum())
    if name.startswith("out"):
        assert n_in < p["M"]                                              # the case has outliers
    assert m["found"] and m["n_inliers"] == n_in
    np.testing.assert_array_equal(m["inliers"], p["inlier"])
    h = m["best"] >> 2
    assert p["inlier"][m["triples"][h]].all()                             # the winner was drawn from inliers
    assert not (m["counts"][:h] == n_in).any() and m["counts"][h] == n_in   # ... and is the FIRST hypothesis with that many
    assert max(lc.pose_err(m["pose"], p["gt_pose"])) < 1e-3
    if name in lc.MODEL_GT_ERR:                                           # the numbers the GPU test's bar is made of
        assert all(e <= b for e, b in zip(lc.pose_err(m["pose"], p["gt_pose"]), lc.MODEL_GT_ERR[name]))
    assert abs(np.linalg.norm(m["pose"][:4]) - 1) < 1e-15 and m["pose"][3] >= 0


def _decisions(p, m):
    """per valid (hypothesis, solution): (h, s, count, every gt inlier under thr / 2, gt inliers lost, smallest relative distance of
    any point's error to the threshold)"""
    gt = p["inlier"].astype(bool)
    for h, (valid, Rs, ts) in enumerate(m["sols"]):
        for s in np.nonzero(valid)[0]:
            pz, e2 = pm.reproj_sq(p["K"], Rs[s], ts[s], p["xyz"], p["uv"])
            with np.errstate(all="ignore"):
                ok = (pz > 0) & (e2 <= lc.THR ** 2)
                half = (pz > 0) & (e2 <= (lc.THR / 2) ** 2)
                edge = min(np.abs(e2 / lc.THR ** 2 - 1).min(), np.abs(pz).min())
            yield h, s, int(ok.sum()), bool(half[gt].all()), int((~ok)[gt].sum()), edge


@pytest.mark.parametrize("name", list(lc.CASES))
def test_gpu_test_inputs_are_not_marginal(name):
    """What tests/test_loop_pose_gpu.py relies on.  Noise-free inputs: every solution of every hypothesis either keeps every
    ground-truth inlier under half the threshold or loses at least three of them, so that the winner and its mask are the ground
    truth whatever the last bit of a reprojection error is.  The case with 0.5 px of noise cannot meet that condition at 100
    hypotheses: a pose from three noisy points whose worst inlier error lies between thr / 2 and thr breaks it by definition, and of
    750 (size, seed) combinations tried none had fewer than one such hypothesis.  Its GPU check is against the model's own mask and
    counts, so what it relies on is asserted instead: no single inlier decision of any solution is within 1e-9 (relative) of the
    threshold, nor any depth within 1e-9 of zero -- the kernel's and the model's operations are the same IEEE operations, and even a
    difference of a few ulp could not flip a decision.  That per-decision margin is asserted for every case."""
    p, m = lc.problem(name), lc.model(name)
    n = 0
    for h, s, count, all_half, lost, edge in _decisions(p, m):
        n += 1
        assert edge > 1e-9, (h, s, edge)
        if not name.startswith("noisy"):
            assert all_half or lost >= 3, (h, s, count, lost)
    assert n >= lc.H // 4                                                 # (the condition was looked at: most triples have solutions)
    assert m["found"]
    if name.startswith("noisy"):
        runner_up = max(c for h, c in enumerate(m["counts"]) if h != (m["best"] >> 2))
        assert runner_up <= m["n_inliers"]
        assert p["inlier"][m["triples"][m["best"] >> 2]].all()


def _compose(po, pr, pose0, which):
    """OptimizeCurrentPose = optimize(10) over all edges, its classification discarded, then the four classified rounds: g2o resets
    lambda and ni at iteration 0 of every optimize() (optimization_algorithm_levenberg.cpp:88-90)"""
    a = po.pose_only(dict(pr, pose=pose0), which=which, rounds=1)
    return po.pose_only(dict(pr, pose=a["pose"]), which=which, rounds=4)


@pytest.mark.parametrize("name", ["out30-64", "out60-257", "noisy-257", "out30-1000"])
def test_refine_composition_oracle_agrees_with_reference(po, ref_available, name):
    p, m = lc.problem(name), lc.model(name)
    o = _compose(po, p, m["pose"], "oracle")
    assert o["n_inliers"] == int(o["inliers"].sum()) >= 10
    if not name.startswith("noisy"):
        np.testing.assert_array_equal(o["inliers"], p["inlier"])
        assert np.abs(o["pose"] - p["gt_pose"]).max() < 1e-4
    if not ref_available:
        pytest.skip("oracle/_ref/libssvio_ref.so not available")
    r = _compose(po, p, m["pose"], "ref")
    assert r["n_inliers"] == o["n_inliers"]
    np.testing.assert_array_equal(r["inliers"], o["inliers"])
    np.testing.assert_allclose(r["pose"], o["pose"], rtol=0, atol=1e-9)   # the bar of test_oracle_ba.py::test_pose_only_known_answers


@pytest.mark.parametrize("M,pose", lc.REFINE_PARAMS, ids=lc.REFINE_IDS)
def test_refine_inputs_are_well_conditioned(po, ref_available, M, pose):
    """What test_loop_pose_gpu.py::test_loop_pose_opt_matches_oracle_composition relies on: the result of the composition does not hang
    on the last bits of its arithmetic.  The kernel sums in another order than the oracle (relative differences of ~1e-16 per sum); a
    start moved by 1e-13, a thousand times that, must not move the result by more than a tenth of the GPU test's bar of 2e-9 (3 km from
    the origin, where 1e-13 is an ulp or two of t: a tenth of that case's bar, lc.refine_bar)."""
    p = lc.refine_problem(M, pose)
    tenth = max(2e-10, lc.refine_bar(M, pose) / 10)
    m = pm.pnp_ransac(p["K"], p["xyz"], p["uv"], lc.H, lc.THR, seed=lc.REFINE_SEED)
    assert m["found"]
    o = _compose(po, p, m["pose"], "oracle")
    assert o["n_inliers"] >= 8
    for k in range(4):
        q = m["pose"].copy()
        q[4:] += 1e-13 * (k + 1) * (-1) ** k
        o2 = _compose(po, p, q, "oracle")
        np.testing.assert_array_equal(o2["inliers"], o["inliers"])
        assert np.abs(o2["pose"] - o["pose"]).max() < tenth, k
    if not ref_available:
        pytest.skip("oracle/_ref/libssvio_ref.so not available")
    r = _compose(po, p, m["pose"], "ref")
    np.testing.assert_array_equal(r["inliers"], o["inliers"])
    np.testing.assert_allclose(r["pose"], o["pose"], rtol=0, atol=max(1e-9, lc.REFINE_ORACLE_VS_REF.get(pose, 0.0)))


# sha256 (first 16 hex digits) over gt_pose, K, xyz, uv, inlier of every scene the suite had before make_loop_pose_problem took gt_pose
_SCENES = {'clean-10': 'db4b14fe71782c09', 'out30-10': 'acc260e72eb5c5ad', 'out60-10': 'b79ca849165b4ff6', 'clean-64': '3d26d300d31e3048',
           'out30-64': '3c799069f59b539c', 'out60-64': '22ee3141aee033b1', 'clean-65': '62a7cd56482e2be6', 'out30-65': '300a8719e40a2946',
           'out60-65': 'b981c75b706ee6c0', 'clean-257': '8304e131d55077b9', 'out30-257': 'ef49b3d809ccd0a6', 'out60-257': 'f19bde0707d7cbde',
           'clean-1000': '1bead8238b2bd3ae', 'out30-1000': 'e3441b9926aacddd', 'out60-1000': '6a77bd927a43a6be', 'noisy-257': 'f2125beb8695e321',
           'refine-10': 'a1789bc2c678ab07', 'refine-256': '8dcad4d9eb3e1040', 'refine-257': 'f252cf8ddce772fc', 'refine-513': 'e7456c2501870e01',
           'refine-1536': 'bb6e73adf33822cb', 'refine-1537': '5edcb5ec2e08a67a'}


def test_scenes_near_identity_kept_their_bytes_and_gt_pose_replaces_only_the_pose():
    import hashlib

    def digest(p):
        h = hashlib.sha256()
        for k in ("gt_pose", "K", "xyz", "uv", "inlier"):
            h.update(np.ascontiguousarray(p[k]).tobytes())
        return h.hexdigest()[:16]
    assert set(_SCENES) == {n for n in lc.CASES if n not in lc.POSE_OF} | {f"refine-{M}" for M in lc.REFINE}
    for name, want in _SCENES.items():
        p = lc.refine_problem(int(name[7:])) if name.startswith("refine") else lc.problem(name)
        assert digest(p) == want, name
    # the same seed with a pose handed in: the pixels before the wrong matches, the depths and the mask are the same draws
    a, b = lc.problem("out30-64"), lc.problem("yaw170-64")
    from tools.synth import make_loop_pose_problem, quat_rot
    c = make_loop_pose_problem(M=64, seed=lc.CASES["yaw170-64"][3], frac_gross=0.3)
    assert np.array_equal(b["uv"], c["uv"]) and np.array_equal(b["inlier"], c["inlier"]) and not np.array_equal(b["xyz"], c["xyz"])
    assert np.array_equal(b["gt_pose"], lc.POSES["yaw170"]) and a["M"] == b["M"]
    for name in lc.POSE_OF:                                               # ... and the points are where that pose sees them
        p = lc.problem(name)
        i = np.nonzero(p["inlier"])[0][:5]
        pc = np.stack([quat_rot(p["gt_pose"][:4], x) + p["gt_pose"][4:] for x in p["xyz"][i]])
        uv = np.stack([p["K"][0] * pc[:, 0] / pc[:, 2] + p["K"][2], p["K"][1] * pc[:, 1] / pc[:, 2] + p["K"][3]], 1)
        assert (pc[:, 2] > 5).all() and np.abs(uv - p["uv"][i]).max() < 1e-3 * lc.x_scale(p)
