"""The inputs of tests/test_pose_only_cases.py (CPU) and tests/test_pose_only_edges_gpu.py: pose-only problems away from the one family
the suite had (tools.synth.make_pose_only_problem: start at identity, truth within 0.02 rad and 0.3 m, every point 5-45 m ahead).

Plain functions, deterministic seeds, KITTI intrinsics; pixels are float32 values (cv::KeyPoint::pt) unless a family says otherwise.
Every input is finite, and no point lies exactly at the camera centre (0 / 0): see include/ssx.h.

A case is (family, M, seed); CASES maps its name to that, CLAIMS to what the case is there for -- a property of the REFERENCE's record
that tests/test_pose_only_cases.py asserts on tests/golden/ref_po_trace.npz (written by tests/golden/make_po_trace.py), so a case
cannot silently stop exercising its path.  Sizes: 1, 3, 6, 60, 200 (one edge per thread), 257 (two) -> k_pose_only<2>; 513 ->
k_pose_only<6>; 1537 -> k_pose_only_generic.  One workgroup solves one problem: nothing larger is needed."""
import functools

import numpy as np

from tools.synth import IDENT_POSE, KITTI_K, pose_inv, quat_rot, small_rot_quat

SIZES = (1, 3, 6, 60, 200, 257, 513, 1537)
FULL = (4, 10)                          # (rounds, iters) of FrontEnd::EstimateCurrentPose
TRUNCATED = ((1, 1), (1, 3), (2, 2))    # ... and runs cut short, which expose the pose in mid-flight


def kernel_of(M):
    return "k2" if M <= 512 else "k6" if M <= 1536 else "generic"


def _quat(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def _project(gt, xyz):
    fx, fy, cx, cy = KITTI_K
    pc = np.stack([quat_rot(gt[:4], p) + gt[4:] for p in xyz])
    return np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1)


def _world(gt, pc):
    """the map points whose camera-frame coordinates under the pose gt (T_cw) are pc"""
    gi = pose_inv(gt)
    return np.stack([quat_rot(gi[:4], p) + gi[4:] for p in pc])


def _ahead(rng, M, zlo=5.0, zhi=45.0):
    return np.stack([rng.uniform(-12, 12, M), rng.uniform(-3, 3, M), rng.uniform(zlo, zhi, M)], 1)


def _near_gt(rng):
    dq = small_rot_quat(rng.uniform(-0.02, 0.02, 3))
    return np.concatenate([dq / np.linalg.norm(dq), rng.uniform(-0.3, 0.3, 3)])


def _finish(M, gt, xyz, uv, pose=None, f32=True):
    if f32:
        uv = uv.astype(np.float32).astype(np.float64)
    assert np.isfinite(xyz).all() and np.isfinite(uv).all()
    return dict(M=M, pose=(IDENT_POSE if pose is None else np.asarray(pose, dtype=np.float64)).copy(), gt_pose=gt, K=np.array(KITTI_K),
                xyz=np.ascontiguousarray(xyz), uv=np.ascontiguousarray(uv))


def _noisy(rng, uv, frac_gross=0.1, sigma=0.5):
    uv = uv + rng.normal(0, sigma, uv.shape)
    gross = rng.random(len(uv)) < frac_gross
    uv[gross] += rng.normal(0, 25.0, (int(gross.sum()), 2))
    return uv


# ---- the families: (M, rng, arg) -> problem -----------------------------------------------------------------------------------------
def base(M, rng, arg=None):
    """the suite's own family, at sizes it did not have"""
    gt = _near_gt(rng)
    xyz = _ahead(rng, M)
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz)))


def far(M, rng, angle):
    """the start (identity) is `angle` rad and a few metres from the truth; the points lie 5-45 m ahead of the TRUE camera"""
    gt = np.concatenate([_quat([0.3, 1.0, 0.2], angle), np.array([0.5, -0.2, 1.0]) * min(angle, 1.5)])
    pc = _ahead(rng, M)
    xyz = _world(gt, pc)
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz)))


def behind(M, rng, arg=None):
    """a fifth of the points (at least one; 40 of 200) lies 5-45 m BEHIND the camera: map points a forward drive has passed"""
    gt = _near_gt(rng)
    pc = _ahead(rng, M)
    k = max(1, M // 5)
    pc[:k, 2] = -rng.uniform(5, 45, k)
    xyz = _world(gt, pc)
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz)))


def plane(M, rng, arg=None):
    """a tenth of the points (at least one) within +-0.02 m of the camera plane z = 0 of the true pose, another tenth behind the camera"""
    gt = _near_gt(rng)
    pc = _ahead(rng, M)
    k = max(1, M // 10)
    z = rng.uniform(0.002, 0.02, k) * rng.choice([-1.0, 1.0], k)
    pc[:k] = np.stack([rng.uniform(-0.5, 0.5, k), rng.uniform(-0.2, 0.2, k), z], 1)
    if M >= 10:
        pc[k:2 * k, 2] = -rng.uniform(5, 45, k)
    xyz = _world(gt, pc)
    uv = _noisy(rng, _project(gt, xyz))
    return _finish(M, gt, xyz, np.clip(uv, -1e6, 1e6))


def tinyz(M, rng, arg=None):
    """three points at |z| <= 1e-6 of the START camera (identity), off its centre"""
    gt = _near_gt(rng)
    xyz = _ahead(rng, M)
    uv = _noisy(rng, _project(gt, xyz))
    xyz[:3] = np.array([[0.4, -0.1, 1e-6], [-0.3, 0.2, -1e-6], [0.2, 0.1, 3e-7]])
    uv[:3] = np.array([[900.0, 100.0], [300.0, 250.0], [700.0, 200.0]])
    return _finish(M, gt, xyz, uv)


def gross(M, rng, frac):
    """a share `frac` of the pixels is grossly wrong (1.0: all of them)"""
    gt = _near_gt(rng)
    xyz = _ahead(rng, M)
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz), frac_gross=frac if frac < 1.0 else 2.0))


def clean(M, rng, start):
    """noise-free pixels (float32 values), from identity.  The start AT the solution is not a case: with exact pixels chi2 is the square
    of the projection's rounding error and no decision of the run is more than rounding -- whether a trial ends by rho == 0 after
    seven trials or by the tenth hangs on whether the norm of the start quaternion rounds to exactly 1 (the reference and both oracle
    builds flip between the two when the start moves by one ulp), so there is no reference record to hold a kernel to; the truncated
    runs of clean-id, which end ON the solution, cover a noise-free problem at its optimum."""
    gt = _near_gt(rng)
    xyz = _ahead(rng, M)
    return _finish(M, gt, xyz, _project(gt, xyz))


def coincident(M, rng, arg=None):
    """every map point is met twice (and thrice where M is odd): H is the sum of a few rank-2 terms repeated"""
    gt = _near_gt(rng)
    half = _ahead(rng, (M + 1) // 2)
    xyz = np.concatenate([half, half])[:M]
    if M % 2:
        xyz[-1] = xyz[0]
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz), frac_gross=0.0))


def axis(M, rng, arg=None):
    """every point on the optical axis of the start camera: the rotation about it is not observable"""
    gt = _near_gt(rng)
    xyz = np.stack([np.zeros(M), np.zeros(M), rng.uniform(5, 45, M)], 1)
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz), frac_gross=0.0))


def deep(M, rng, arg=None):
    """a scene 3 km deep: x, y and z a hundred times the base family's, the same pixels"""
    gt = _near_gt(rng)
    xyz = _ahead(rng, M) * 100.0
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz)))


def small(M, rng, arg=None):
    """M = 3 (6: coincident-6, farsmall1.5-6; 1: farsmall1.5-1 -- a single point near the start is met exactly within two iterations, and
    everything after is rounding): fewer edges than unknowns allow, and every thread but a few idle"""
    gt = _near_gt(rng)
    xyz = _ahead(rng, M)
    return _finish(M, gt, xyz, _noisy(rng, _project(gt, xyz), frac_gross=0.0))


FAMILIES = dict(base=base, far=far, behind=behind, plane=plane, tinyz=tinyz, gross=gross, clean=clean, coincident=coincident, axis=axis,
                deep=deep, small=small)

# name -> (family, argument, M, seed).  Seeds are chosen by tests/golden/make_po_trace.py's conditions (the reference and both builds
# of the oracle take the same Levenberg decisions through the first five iterations of every case, and through 90 % of all recorded
# iterations): a case that breaks them gets another seed here, it is not excused there.
CASES = {
    # k_pose_only<2>
    "base-200": ("base", None, 200, 212),
    "far0.2-200": ("far", 0.2, 200, 1821), "far0.6-200": ("far", 0.6, 200, 22), "far1.5-200": ("far", 1.5, 200, 23), "far3.0-60": ("far", 3.0, 60, 24),
   
    "behind-200": ("behind", None, 200, 731), "plane-257": ("plane", None, 257, 1332), "tinyz-60": ("tinyz", None, 60, 34),
    "gross70-200": ("gross", 0.7, 200, 141), "gross100-60": ("gross", 1.0, 60, 42),
    "clean-id-200": ("clean", "id", 200, 751),
    "coincident-6": ("coincident", None, 6, 261), "axis-60": ("axis", None, 60, 63), "axis-257": ("axis", None, 257, 1565),
    "deep-200": ("deep", None, 200, 64),
    "farsmall1.5-1": ("far", 1.5, 1, 92), "small-3": ("small", None, 3, 172),
    "deep-60": ("deep", None, 60, 81), "deep-257": ("deep", None, 257, 82), "far1.5-60": ("far", 1.5, 60, 84),
    "far1.5-257": ("far", 1.5, 257, 85), "far3.0-200": ("far", 3.0, 200, 86), "far3.0-257": ("far", 3.0, 257, 87), "tinyz-200": ("tinyz", None, 200, 88),
    "far0.6-60": ("far", 0.6, 60, 91),
    # a far start with barely as many edges as unknowns
    "farsmall1.5-6": ("far", 1.5, 6, 94),
   
    # k_pose_only<6>
    "far0.6-513": ("far", 0.6, 513, 26), "far1.5-513": ("far", 1.5, 513, 27), "plane-513": ("plane", None, 513, 35),
    "clean-id-513": ("clean", "id", 513, 353), "deep-513": ("deep", None, 513, 66), "tinyz-513": ("tinyz", None, 513, 37),
   
    # k_pose_only_generic
    "far0.6-1537": ("far", 0.6, 1537, 28), "far1.5-1537": ("far", 1.5, 1537, 29), "plane-1537": ("plane", None, 1537, 36),
    "clean-id-1537": ("clean", "id", 1537, 755), "tinyz-1537": ("tinyz", None, 1537, 38), "far3.0-1537": ("far", 3.0, 1537, 19),
    "gross100-1537": ("gross", 1.0, 1537, 44),
}
assert all(M in SIZES for _, _, M, _ in CASES.values())

# what a case is there for: a predicate on the reference's record at FULL (see claim_holds)
CLAIMS = {name: "none" for name in CASES}
for _n in CASES:
    if _n.startswith(("far0.6", "far3.0-1537")):
        CLAIMS[_n] = "lost"                      # too far for Levenberg from identity: (almost) every edge ends as outlier
    elif _n.startswith(("far1.5", "far3.0-60", "far3.0-2", "tinyz")):
        CLAIMS[_n] = "no_active_round"           # a round that starts with no active edge (g2o: "0 vertices to optimize")
    elif _n.startswith(("far0.2", "clean-id", "deep")):
        CLAIMS[_n] = "converges"                 # the run gets from its start to the truth
    elif _n.startswith(("behind", "plane")):
        CLAIMS[_n] = "mixed"                     # some edges end as outliers (the points no camera can see among them), others stay active
    elif _n.startswith("gross100"):
        CLAIMS[_n] = "few_inliers"

NI_CASE = "plane-257"
# The case in which `ni = 2` on an accepted trial matters: inside ONE optimize() an iteration with a rejected trial followed by an
# accepted one (trials >= 2 and another iteration follows: a rejected LAST trial would have terminated), and a rejected trial in a
# later iteration (trials >= 2 again) -- without the reset the later rejection multiplies lambda by 4 or more instead of 2.  Found with
# the oracle's record; the CPU test asserts it on the STABLE part of the reference's.
CLAIMS[NI_CASE] = "ni_reset"


def settings(name):
    return (FULL,) + TRUNCATED


RUNS = [(name, r, i) for name in CASES for (r, i) in settings(name)]


def run_key(name, rounds, iters):
    return f"{name}_r{rounds}i{iters}"


@functools.lru_cache(maxsize=None)
def problem(name):
    fam, arg, M, seed = CASES[name]
    return FAMILIES[fam](M, np.random.default_rng(seed), arg)


def ni_property(trials, iters_run, stable=None):
    """-> True when some optimize() of the record holds a rejected-then-accepted iteration and a rejection in a later one (stable: look
    at the stable prefix of each optimize() only)"""
    for r in range(len(iters_run)):
        t = trials[r, :iters_run[r] if stable is None else min(iters_run[r], stable[r])]
        multi = np.nonzero(t >= 2)[0]
        if len(multi) >= 2 and multi[0] < iters_run[r] - 1:
            return True
    return False


def claim_holds(name, rec, gt_pose):
    """rec: the reference's record at FULL: dict(pose, n_inliers, trials, active, iters_run, terminated, outliers)"""
    c = CLAIMS[name]
    M = CASES[name][2]
    err = min(np.abs(rec["pose"][:4] - gt_pose[:4]).max(), np.abs(rec["pose"][:4] + gt_pose[:4]).max()) + np.abs(rec["pose"][4:] - gt_pose[4:]).max()
    if c == "no_active_round":
        return bool((rec["active"][1:] == 0).any()) and rec["n_inliers"] == 0
    if c == "lost":
        return rec["n_inliers"] <= M // 20
    if c == "converges":
        return err < 5e-2 * (100.0 if name.startswith("deep") else 1.0) and rec["n_inliers"] > M // 2
    if c == "mixed":
        return 0 < rec["n_inliers"] < M and bool((rec["outliers"] > 0).all())
    if c == "few_inliers":
        return rec["n_inliers"] < M // 4
    if c == "ni_reset":
        return ni_property(rec["trials"], rec["iters_run"], rec.get("stable"))
    return True


def pose_floor(M):
    """today's bars of the pose-only tests (tests/test_ba_gpu.py, tests/loop_pose_cases.refine_bar)"""
    return 1e-8 if M < 8 else 2e-9


@functools.lru_cache(maxsize=None)
def load_fixture():
    """tests/golden/ref_po_trace.npz unpacked: (dict run_key -> dict(rounds, iters, M, pose, inliers, n_inliers, chi2, lam, trials, d_lam, d_chi2
    [rounds, iters], active, iters_run, terminated, outliers, stable, round_stable [rounds], d_pose), dict of the global entries)"""
    import os
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_po_trace.npz"))
    runs = {}
    o_it = o_rd = o_mask = 0
    for k, key in enumerate(G["runs"]):
        R, I, M = int(G["rounds"][k]), int(G["iters"][k]), int(G["M"][k])
        nb = (M + 7) // 8
        it = lambda f: G[f][o_it:o_it + R * I].reshape(R, I)        # noqa: E731
        rr = G["round"][4 * o_rd:4 * (o_rd + R)].reshape(R, 4)
        runs[str(key)] = dict(rounds=R, iters=I, M=M, pose=G["pose"][7 * k:7 * k + 7], inliers=np.unpackbits(G["mask"][o_mask:o_mask + nb])[:M],
                              n_inliers=int(G["n"][k]), chi2=it("chi2"), lam=it("lam"), trials=it("trials").astype(np.int32),
                              d_lam=it("d_lam").astype(np.float64), d_chi2=it("d_chi2").astype(np.float64), active=rr[:, 0], iters_run=rr[:, 1],
                              terminated=rr[:, 2], outliers=rr[:, 3], stable=G["stable"][o_rd:o_rd + R].astype(np.int32),
                              round_stable=G["round_stable"][o_rd:o_rd + R], d_pose=float(G["d_pose"][k]))
        o_it += R * I; o_rd += R; o_mask += nb
    glob = {k: float(G[k]) for k in ("floor_lam", "floor_chi2", "K", "chi2_abs", "n_recorded", "n_stable")}
    return runs, glob


def rel_chi2(a, ref, first, chi2_abs):
    """the relative chi2 distance of the fixture (tests/golden/make_po_trace.py)"""
    return np.abs(a - ref) / (np.abs(ref) + 1e-7 * first + chi2_abs)


def compare_with_fixture(got, fx, glob, check_pose=True):
    """Hold a record (dict as oracle.pyoracle.pose_only_trace / ssvio_amd.ba.pose_only_trace return it) to a run of the fixture.  Asserts
    every count and flag; -> dict(pose, lam, chi2 = the worst distance / its bar as (distance, bar) at the worst ratio)."""
    R = fx["rounds"]
    assert got["n_inliers"] == fx["n_inliers"] and np.array_equal(got["inliers"], fx["inliers"]), "mask / inlier count"
    assert np.array_equal(got["active"], fx["active"]), ("active edges per round", got["active"], fx["active"])
    assert np.array_equal(got["outliers"], fx["outliers"]), ("outliers per round", got["outliers"], fx["outliers"])
    worst = dict(lam=(0.0, glob["floor_lam"]), chi2=(0.0, glob["floor_chi2"]))
    first = fx["chi2"][0, 0]
    for r in range(R):
        k = int(fx["stable"][r])
        assert got["iters_run"][r] >= k, ("iterations run", r, got["iters_run"][r], k)
        assert np.array_equal(got["trials"][r, :k], fx["trials"][r, :k]), ("trials", r, got["trials"][r], fx["trials"][r])
        if fx["round_stable"][r]:
            assert got["iters_run"][r] == fx["iters_run"][r] and got["terminated"][r] == fx["terminated"][r], ("iterations / terminated", r)
        for f, d, floor in (("lam", np.abs(got["lam"][r, :k] - fx["lam"][r, :k]) / np.abs(fx["lam"][r, :k]), glob["floor_lam"]),
                            ("chi2", rel_chi2(got["chi2"][r, :k], fx["chi2"][r, :k], first, glob["chi2_abs"]), glob["floor_chi2"])):
            bar = np.maximum(floor, glob["K"] * fx["d_" + f][r, :k])
            assert (d <= bar).all(), (f, r, d.tolist(), bar.tolist())
            if k and (d / bar).max() > worst[f][0] / worst[f][1]:
                j = int(np.argmax(d / bar))
                worst[f] = (float(d[j]), float(bar[j]))
    bar = max(pose_floor(fx["M"]), glob["K"] * fx["d_pose"])
    d = float(np.abs(got["pose"] - fx["pose"]).max())
    if check_pose:
        assert d <= bar, ("pose", d, bar)
    worst["pose"] = (d, bar)
    return worst
