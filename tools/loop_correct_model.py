"""Executable model of ssx_loop_correct (ssvio_amd/csrc/loop_correct.inc), the library's restatement of the geometry of
LoopClosing::LoopCorrect (reference: src/ssvio/loopclosing.cpp:353-594).  The contract of that call is this file, in the role
tools/pnp_model.py has for the RANSAC.

stage 1   CorrectActivateKeyframeAndMappoint (:378-425): an active keyframe a != cur gets T'_a = (T_a * T_cur^-1) * corrected, the
          current keyframe gets `corrected`; an active point whose anchor is an active keyframe gets p' = T'_a^-1 * (T_a * p)
stage 2   PoseGraphOptimization (:458-533): NOT restated -- the optimiser is passed in as a callable on a flat problem
          dict(poses, fixed, ei, ej, meas) with fixed = active | loop | initial, and returns a dict with "poses"
stage 3   :537-591: a non-active point with an anchor gets p' = T_opt^-1 * (T_stage1 * p), also where the vertex was fixed; keep_kf (the
          front-end's reference keyframe) keeps its stage-1 pose while its points are re-anchored with the estimate

Every operation is written in the order of ssvio_amd/csrc/se3.hpp -- the normalising se3_inverse, the normalising se3_mul, the
quat_rotate form p + w u + q x u with u = 2 q x p -- as one IEEE double operation each (numpy arrays, no fused multiply-add).  The
kernel is compiled with contraction on, so it differs from this file by FMA rounding only; tests/golden/make_loop_correct_hp.py measures
this file against 60 digits and tests/test_loop_correct_gpu.py holds the kernel to four times that.  (tools/synth.py's pose_inv does
not re-normalise and is therefore not used here.)

A problem is a dict: poses [P, 7] (qx qy qz qw tx ty tz, T_cw), kf_active [P], cur_kf, loop_kf, initial_kf (-1: none), keep_kf
(-1: none), corrected_pose [7], ei / ej [E], meas [E, 7], points [N, 3], point_anchor [N] (-1: leave alone), point_active [N]."""
import numpy as np


def quat_rotate(q, p):
    """q [..., 4] (x y z w), p [..., 3]"""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    p0, p1, p2 = p[..., 0], p[..., 1], p[..., 2]
    ux = y * p2 - z * p1
    uy = z * p0 - x * p2
    uz = x * p1 - y * p0
    ux = ux + ux; uy = uy + uy; uz = uz + uz
    return np.stack([p0 + w * ux + (y * uz - z * uy), p1 + w * uy + (z * ux - x * uz), p2 + w * uz + (x * uy - y * ux)], -1)


def se3_act(T, p):
    return quat_rotate(T[..., :4], p) + T[..., 4:]


def se3_mul(A, B):
    ax, ay, az, aw = A[..., 0], A[..., 1], A[..., 2], A[..., 3]
    bx, by, bz, bw = B[..., 0], B[..., 1], B[..., 2], B[..., 3]
    w = aw * bw - ax * bx - ay * by - az * bz
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    n = np.sqrt(x * x + y * y + z * z + w * w)
    r = quat_rotate(A[..., :4], B[..., 4:])
    return np.concatenate([np.stack([x / n, y / n, z / n, w / n], -1), A[..., 4:] + r], -1)


def se3_inverse(T):
    q = np.stack([-T[..., 0], -T[..., 1], -T[..., 2], T[..., 3]], -1)
    n = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])
    q = q / n[..., None]
    return np.concatenate([q, quat_rotate(q, T[..., 4:] * -1.0)], -1)


def _arrays(pr):
    poses = np.ascontiguousarray(pr["poses"], dtype=np.float64).reshape(-1, 7)
    act = np.ascontiguousarray(pr["kf_active"]).reshape(-1) != 0
    pts = np.ascontiguousarray(pr["points"], dtype=np.float64).reshape(-1, 3)
    anc = np.ascontiguousarray(pr["point_anchor"], dtype=np.int64).reshape(-1)
    pact = np.ascontiguousarray(pr["point_active"]).reshape(-1) != 0
    return poses, act, pts, anc, pact


def fixed_set(pr):
    """pose_fixed of stage 2 (:482-486)"""
    f = (np.ascontiguousarray(pr["kf_active"]).reshape(-1) != 0).astype(np.uint8)
    f[pr["loop_kf"]] = 1
    if pr["initial_kf"] >= 0:
        f[pr["initial_kf"]] = 1
    return f


def reanchor(old_poses, inv_new_poses, pts, anc, sel):
    """p' = inv_new[a] * (old[a] * p) for the selected points; the others keep their bits"""
    out = pts.copy()
    if sel.any():
        a = anc[sel]
        out[sel] = se3_act(inv_new_poses[a], se3_act(old_poses[a], pts[sel]))
    return out


def stage1(pr):
    """-> (stage-1 poses [P, 7], points after stage 1 [N, 3], moved [N] bool)"""
    poses, act, pts, anc, pact = _arrays(pr)
    cur = int(pr["cur_kf"])
    if not act[cur]:
        raise ValueError("the current keyframe is not active")
    corrected = np.ascontiguousarray(pr["corrected_pose"], dtype=np.float64)
    s1 = poses.copy()
    others = act.copy(); others[cur] = False
    if others.any():
        rel = se3_mul(poses[others], se3_inverse(poses[cur])[None, :])           # T_kn_k = T_a * T_cur^-1       (:394)
        s1[others] = se3_mul(rel, corrected[None, :])                            # T_kn_true = T_kn_k * corrected (:397)
    s1[cur] = corrected
    moved = pact & (anc >= 0) & act[np.maximum(anc, 0)]
    return s1, reanchor(poses, se3_inverse(s1), pts, anc, moved), moved


def stage3(pr, s1_poses, opt_poses, pts):
    """-> (poses returned [P, 7], points after stage 3 [N, 3], moved [N] bool)"""
    _, _, _, anc, pact = _arrays(pr)
    moved = ~pact & (anc >= 0)
    out_pts = reanchor(s1_poses, se3_inverse(opt_poses), pts, anc, moved)
    out = opt_poses.copy()
    if pr["keep_kf"] >= 0:
        out[pr["keep_kf"]] = s1_poses[pr["keep_kf"]]                             # :572-587
    return out, out_pts, moved


def loop_correct(pr, optimiser, iters=20):
    """the whole call.  optimiser(flat problem, iters) -> dict with "poses" (more keys are passed through under "pg"); it is not called
    when nothing can be optimised (no free keyframe, no edge, iters <= 0)"""
    s1, p1, moved1 = stage1(pr)
    fixed = fixed_set(pr)
    ei = np.ascontiguousarray(pr["ei"], dtype=np.int32); ej = np.ascontiguousarray(pr["ej"], dtype=np.int32)
    pg = None
    opt = s1
    if (fixed == 0).any() and len(ei) > 0 and iters > 0:
        pg = optimiser(dict(P=len(s1), E=len(ei), poses=s1.copy(), fixed=fixed, ei=ei, ej=ej, meas=np.ascontiguousarray(pr["meas"], dtype=np.float64)), iters)
        opt = np.ascontiguousarray(pg["poses"], dtype=np.float64)
    poses, p3, moved3 = stage3(pr, s1, opt, p1)
    act = np.ascontiguousarray(pr["kf_active"]).reshape(-1) != 0
    return dict(poses=poses, points=p3, stage1_poses=s1, stage1_points=p1, opt_poses=opt, pg=pg, n_active_kf=int(act.sum()),
                n_active_points_moved=int(moved1.sum()), n_other_points_moved=int(moved3.sum()),
                n_points_skipped=int(len(p3) - moved1.sum() - moved3.sum()))


def host_loops(pr, s1_then_opt):
    """the path without ssx_loop_correct, for tools/loop_correct_time.py: stage 1 here, the optimiser through s1_then_opt(flat problem)
    (a library call: the poses go down and come up again), stage 3 here"""
    return loop_correct(pr, lambda flat, iters: s1_then_opt(flat), iters=1)
