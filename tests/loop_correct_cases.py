"""Deterministic problems for ssx_loop_correct / tools/loop_correct_model.py, shared by tests/golden/make_loop_correct_hp.py,
tests/test_loop_correct_model.py and tests/test_loop_correct_gpu.py.

A case is the pose graph of tools.synth.make_pose_graph_problem with what LoopClosing::LoopCorrect needs beside it: the active
window (the newest n_active keyframes, drifted rigidly away from where `corrected_pose` puts them), the current, loop, initial and
kept keyframes, and map points.  Every case with enough points mixes, by the point's index modulo 10:
    0 1 2  active point anchored to an active keyframe (2: to the current keyframe)       moved by stage 1
    3      active point anchored to a keyframe that is not active                         left alone (:413-415)
    4      active point, anchor -1                                                        left alone
    5 6 7  non-active point anchored to a keyframe (5, 6: mostly free ones)               moved by stage 3
    8      non-active point anchored to a fixed keyframe (loop / active / kept in turn)   moved by stage 3 (by rounding)
    9      non-active point, anchor -1                                                    left alone (:556-561)
The point counts 0, 1, 63, 64, 65, 255, 257 are the tails of a 64-wide wave and of a 256-thread workgroup."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import synth  # noqa: E402

# name -> (pose graph arguments, points, options)
SPECS = {
    "lc12": (dict(P=12, n_loops=1, seed=13, meas_noise=0.03, drift=0.05, n_active=2), 65, dict()),
    "lc60": (dict(P=60, n_loops=2, seed=11, meas_noise=0.02, drift=0.05, n_active=7), 257, dict(loop_pick=1, keep="free")),
    "lc200": (dict(P=200, n_loops=3, seed=12, meas_noise=0.01, drift=0.03, n_active=7), 1000, dict(loop_pick=2, initial=-1, keep="cur")),
    "only_cur": (dict(P=12, n_loops=1, seed=14, meas_noise=0.03, drift=0.05, n_active=1), 63, dict(keep="cur")),
    "all_fixed": (dict(P=12, n_loops=1, seed=15, meas_noise=0.03, drift=0.05, n_active=12), 64, dict()),
    "no_edges": (dict(P=12, n_loops=1, seed=16, meas_noise=0.03, drift=0.05, n_active=3), 255, dict(no_edges=True, keep=-1)),
    "far": (dict(P=24, n_loops=1, seed=17, meas_noise=0.02, drift=0.05, n_active=4), 130, dict(far=3000.0)),
    "half_turn": (dict(P=24, n_loops=1, seed=18, meas_noise=0.02, drift=0.05, n_active=4), 129, dict(half_turn=True)),
    "no_change": (dict(P=24, n_loops=1, seed=19, meas_noise=0.02, drift=0.05, n_active=4), 66, dict(no_change=True)),
    "lc12_n0": (dict(P=12, n_loops=1, seed=13, meas_noise=0.03, drift=0.05, n_active=2), 0, dict()),
    "lc12_n1": (dict(P=12, n_loops=1, seed=13, meas_noise=0.03, drift=0.05, n_active=2), 1, dict()),
}
NAMES = list(SPECS)


def _world(T, G):
    """the poses T_cw after the world is moved by G^-1 (p -> G^-1 p): T * G"""
    return np.array([synth.pose_mul(t, G) for t in np.atleast_2d(T)])


def make(name):
    pg_args, N, opt = SPECS[name]
    pg = synth.make_pose_graph_problem(**pg_args)
    P, n_active = pg["P"], pg_args["n_active"]
    rng = np.random.default_rng(1000 + pg_args["seed"])
    gt = pg["gt_poses"]
    cur = P - 1
    active = np.zeros(P, np.uint8)
    active[P - n_active:] = 1
    loops = [int(j) for j in pg["ej"][P - 1:]]                  # the loop edges' targets
    loop_kf = loops[opt.get("loop_pick", 0)]
    initial_kf = opt.get("initial", 0)
    # the window as the odometry left it: rigidly off by D from where the corrected current pose puts it
    D = np.concatenate([synth.small_rot_quat(np.array([0.01, -0.04, 0.02])), [0.8, -0.1, 1.5]])
    D[:4] /= np.linalg.norm(D[:4])
    corrected = gt[cur].copy()
    poses = pg["poses"].copy()
    T_cur_in = synth.pose_mul(D, gt[cur])
    for a in np.nonzero(active)[0]:
        poses[a] = synth.pose_mul(synth.pose_mul(gt[a], synth.pose_inv(gt[cur])), T_cur_in)
    poses[cur] = T_cur_in
    if opt.get("no_change"):
        corrected = poses[cur].copy()
    keep = opt.get("keep", "active")
    fixed = active.copy(); fixed[loop_kf] = 1
    if initial_kf >= 0:
        fixed[initial_kf] = 1
    free = np.nonzero(fixed == 0)[0]
    if keep == "free":
        keep_kf = int(free[len(free) // 2])
    elif keep == "cur":
        keep_kf = cur
    elif keep == "active":
        keep_kf = int(np.nonzero(active)[0][0])
    else:
        keep_kf = -1
    # ---- points: a position in the anchor's camera frame, carried to the world with the input pose ----
    act_idx = np.nonzero(active)[0]
    non_act = np.nonzero(active == 0)[0]
    fixed_cycle = [loop_kf, int(act_idx[0]), keep_kf if keep_kf >= 0 else cur]
    anchor = np.full(N, -1, np.int32)
    pact = np.zeros(N, np.uint8)
    pts = np.zeros((N, 3))
    for i in range(N):
        m = i % 10
        pact[i] = m < 5
        if m in (0, 1):
            a = int(act_idx[(i // 10 + m) % len(act_idx)])
        elif m == 2:
            a = cur
        elif m == 3:
            a = int(non_act[(7 * i) % len(non_act)]) if len(non_act) else -1
        elif m in (5, 6):
            a = int(free[(3 * i + m) % len(free)]) if len(free) else int(act_idx[i % len(act_idx)])
        elif m == 7:
            a = (5 * i + 1) % P
        elif m == 8:
            a = fixed_cycle[(i // 10) % 3]
        else:
            a = -1
        anchor[i] = a
        pc = np.array([rng.uniform(-10, 10), rng.uniform(-2, 2), rng.uniform(3, 40)])
        T = poses[a] if a >= 0 else poses[i % P]
        pts[i] = synth.quat_rot(synth.pose_inv(T)[:4], pc - T[4:])
    ei, ej, meas = pg["ei"], pg["ej"], pg["meas"]
    if opt.get("no_edges"):
        ei, ej, meas = ei[:0], ej[:0], meas[:0]
    G = None
    if opt.get("far"):
        G = np.array([0, 0, 0, 1.0, -opt["far"], -0.25 * opt["far"], 0.5 * opt["far"]])
    if opt.get("half_turn"):
        # turn the world so that the corrected pose's quaternion has w = 0
        qc = corrected[:4]
        qg = synth.quat_mul(np.array([-qc[0], -qc[1], -qc[2], qc[3]]), np.array([0.6, 0.0, 0.8, 0.0]))
        G = np.concatenate([qg / np.linalg.norm(qg), [1.0, -2.0, 0.5]])
    if G is not None:
        Gi = synth.pose_inv(G)
        poses, corrected = _world(poses, G), _world(corrected, G)[0]
        pts = np.array([synth.quat_rot(Gi[:4], p) + Gi[4:] for p in pts]).reshape(-1, 3)
    if opt.get("half_turn"):
        corrected[3] = 0.0
        corrected[:4] /= np.linalg.norm(corrected[:4])
        assert corrected[3] == 0.0
    return dict(name=name, P=P, E=len(ei), N=N, poses=np.ascontiguousarray(poses), kf_active=active, cur_kf=cur, loop_kf=loop_kf,
                initial_kf=initial_kf, keep_kf=keep_kf, corrected_pose=np.ascontiguousarray(corrected), ei=np.ascontiguousarray(ei, dtype=np.int32),
                ej=np.ascontiguousarray(ej, dtype=np.int32), meas=np.ascontiguousarray(meas).reshape(-1, 7), points=np.ascontiguousarray(pts),
                point_anchor=anchor, point_active=pact)


def stated_opt_poses(pr, s1_poses):
    """a stated set of "optimised" poses for stage 3's truth, independent of any optimiser: the free keyframes of the stage-1 poses
    moved by a smooth, index-dependent small motion (a few centimetres, a few milliradians); fixed keyframes keep their bits"""
    from tools import loop_correct_model as lcm
    fixed = lcm.fixed_set(pr)
    out = np.array(s1_poses, dtype=np.float64).copy()
    for i in np.nonzero(fixed == 0)[0]:
        w = 0.004 * np.array([np.sin(0.7 * i), np.cos(0.3 * i), np.sin(0.2 * i + 1.0)])
        d = np.concatenate([synth.small_rot_quat(w), 0.05 * np.array([np.cos(0.5 * i), np.sin(0.9 * i), np.cos(0.1 * i)])])
        d[:4] /= np.linalg.norm(d[:4])
        out[i] = synth.pose_mul(d, out[i])
    return out


def fix_sign(q_poses, ref_poses):
    """q and -q are one rotation: the poses with the sign of each quaternion chosen as in ref_poses"""
    out = np.array(q_poses, dtype=np.float64).copy()
    flip = (out[:, :4] * ref_poses[:, :4]).sum(1) < 0
    out[flip, :4] *= -1.0
    return out


def pose_distance(a, b):
    """largest difference of an entry, quaternion signs fixed"""
    return float(np.abs(fix_sign(a, b) - b).max()) if len(a) else 0.0


def point_distance(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) if len(a) else 0.0


def magnitude(pr, *more):
    """the largest number of the case: the size every rounding error of it scales with"""
    m = max(float(np.abs(pr["poses"]).max()), float(np.abs(pr["corrected_pose"]).max()), float(np.abs(pr["points"]).max()) if pr["N"] else 0.0)
    for a in more:
        if len(a):
            m = max(m, float(np.abs(a).max()))
    return m


def expected_counts(pr):
    act, anc, pact = pr["kf_active"] != 0, pr["point_anchor"], pr["point_active"] != 0
    m1 = int((pact & (anc >= 0) & act[np.maximum(anc, 0)]).sum())
    m3 = int((~pact & (anc >= 0)).sum())
    return dict(n_active_kf=int(act.sum()), n_active_points_moved=m1, n_other_points_moved=m3, n_points_skipped=pr["N"] - m1 - m3)


def check_invariants(pr, s1_poses, opt_poses, out_poses, out_points, s1_points=None):
    """what LoopCorrect conserves, on any implementation's output.  opt_poses = the vertex estimates (out_poses with keep_kf's estimate
    instead of its kept pose).  Tolerance: every quantity below is two or three SE3 operations on numbers up to M = magnitude(pr), each a
    dozen roundings of terms up to 2 M, compared with another such chain: 64 spacing(M) on lengths; 1e-12 on unit quaternions."""
    from tools import loop_correct_model as lcm
    tol = 64 * np.spacing(magnitude(pr, s1_poses, opt_poses))
    act, anc, pact = pr["kf_active"] != 0, pr["point_anchor"], pr["point_active"] != 0
    cur, keep = pr["cur_kf"], pr["keep_kf"]
    T0, p0 = pr["poses"], pr["points"]
    for T in (s1_poses, opt_poses, out_poses):
        assert np.isfinite(T).all() and np.abs(np.linalg.norm(T[:, :4], axis=1) - 1.0).max() <= 1e-12
    # stage 1: the window moves rigidly -- T'_a T'_cur^-1 == T_a T_cur^-1 -- and with `corrected`; other keyframes keep their bits
    assert np.array_equal(s1_poses[~act], T0[~act])
    assert np.array_equal(s1_poses[cur], pr["corrected_pose"])
    rel_new = lcm.se3_mul(s1_poses[act], lcm.se3_inverse(s1_poses[cur])[None, :])
    rel_old = lcm.se3_mul(T0[act], lcm.se3_inverse(T0[cur])[None, :])
    d = fix_sign(rel_new, rel_old) - rel_old
    assert np.abs(d[:, :4]).max() <= 1e-12 and np.abs(d[:, 4:]).max() <= tol, np.abs(d).max(0)
    # the points: the position in the anchor's camera is conserved, stage by stage; everything else keeps its bits
    m1 = pact & (anc >= 0) & act[np.maximum(anc, 0)]
    m3 = ~pact & (anc >= 0)
    assert np.array_equal(out_points[~(m1 | m3)], p0[~(m1 | m3)])
    if m1.any():
        a = anc[m1]
        assert np.abs(lcm.se3_act(s1_poses[a], out_points[m1]) - lcm.se3_act(T0[a], p0[m1])).max() <= tol
    if m3.any():
        a = anc[m3]
        assert np.abs(lcm.se3_act(opt_poses[a], out_points[m3]) - lcm.se3_act(s1_poses[a], p0[m3])).max() <= tol
    if s1_points is not None:
        assert np.array_equal(s1_points[~m1], p0[~m1]) and np.array_equal(s1_points[m1], out_points[m1])
    # the poses returned: the estimates, except the kept keyframe's stage-1 pose
    others = np.arange(pr["P"]) != keep
    assert np.array_equal(out_poses[others], opt_poses[others])
    if keep >= 0:
        assert np.array_equal(out_poses[keep], s1_poses[keep])
