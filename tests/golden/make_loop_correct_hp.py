"""tests/golden/loop_correct_hp.npz: stages 1 and 3 of LoopClosing::LoopCorrect to 60 digits -- the yardstick of
tools/loop_correct_model.py and, through it, of ssx_loop_correct (ssvio_amd/csrc/loop_correct.inc).

Every pose is the rigid motion its seven stored doubles name: rotation by the quaternion DIVIDED BY ITS NORM (what Sophus holds after
its constructor), then the translation.  With mpmath at 60 digits, from the exact values of the doubles of tests/loop_correct_cases.py:

  s1_poses    T'_a = (T_a T_cur^-1) corrected for the active keyframes, `corrected` for the current one, the input elsewhere
  s1_points   p' = T'_a^-1 (T_a p) for the active points anchored to an active keyframe, the input elsewhere
  stage 3 is held to two truths, neither of which needs an optimiser:
  identity    with the optimiser bypassed the new pose IS the old pose, and T^-1 (T p) = p whatever T is: the non-active points of an
              iterations = 0 call are exactly the points stage 1 left (s1_points); no array is stored for it
  s3_*        for the model's f64 stage-1 poses (s3_s1_poses), the model's f64 stage-1 points (s3_in_points) and the stated f64
              "optimised" poses of loop_correct_cases.stated_opt_poses (s3_opt_poses), all stored: s3_points = T_opt^-1 (T_s1 p) for the
              non-active points with an anchor, the input elsewhere

Every number is rounded to double at the very end; quaternions are stored with the sign of the input pose's (s1_poses).

model_<quantity>[case] is the model's own largest distance from that truth (loop_correct_cases.pose_distance / point_distance: largest
difference of an entry, quaternion sign fixed first), for the quantities s1_poses, s1_points, identity, s3_points; factor = 4 is the
margin a differently contracted build of the same operations is given (the project's factor for an equivalent evaluation order, as in
p3p_hp.npz and the loop-pose refinement).  No number here comes from the kernel.

    python tests/golden/make_loop_correct_hp.py        (needs mpmath; under a minute)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import loop_correct_cases as lcc  # noqa: E402
from tools import loop_correct_model as lcm  # noqa: E402

OUT = os.path.join(HERE, "loop_correct_hp.npz")
DPS = 60
FACTOR = 4.0
QUANTITIES = ("s1_poses", "s1_points", "identity", "s3_points")


def _hp():
    import mpmath as mp
    mp.mp.dps = DPS
    f = mp.mpf

    def pose(T):
        q = [f(float(v)) for v in T[:4]]
        n = mp.sqrt(sum(v * v for v in q))
        return [v / n for v in q], [f(float(v)) for v in T[4:]]

    def qmul(a, b):
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                aw * bw - ax * bx - ay * by - az * bz]

    def rot(q, p):
        # R(q) p by the rotation matrix of a unit quaternion: another route than the model's p + w u + q x u
        x, y, z, w = q
        R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
             [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
             [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        return [sum(R[r][c] * p[c] for c in range(3)) for r in range(3)]

    def mul(A, B):
        q = qmul(A[0], B[0])
        r = rot(A[0], B[1])
        return q, [A[1][k] + r[k] for k in range(3)]

    def inv(A):
        q = [-A[0][0], -A[0][1], -A[0][2], A[0][3]]
        r = rot(q, A[1])
        return q, [-r[k] for k in range(3)]

    def act(A, p):
        r = rot(A[0], p)
        return [r[k] + A[1][k] for k in range(3)]

    def out_pose(A, like):
        v = np.array([float(x) for x in A[0]] + [float(x) for x in A[1]])
        if np.dot(v[:4], like[:4]) < 0:
            v[:4] *= -1.0
        return v

    return f, pose, mul, inv, act, out_pose


def truth(pr, s3_s1, s3_opt, s3_in):
    f, pose, mul, inv, act, out_pose = _hp()
    P, N = pr["P"], pr["N"]
    T = [pose(pr["poses"][i]) for i in range(P)]
    C = pose(pr["corrected_pose"])
    cur = pr["cur_kf"]
    Tci = inv(T[cur])
    S1 = []
    for a in range(P):
        if not pr["kf_active"][a]:
            S1.append(T[a])
        elif a == cur:
            S1.append(C)
        else:
            S1.append(mul(mul(T[a], Tci), C))
    s1_poses = np.array([pr["poses"][a] if not pr["kf_active"][a] else out_pose(S1[a], pr["poses"][a]) for a in range(P)]).reshape(P, 7)
    s1_points = pr["points"].copy()
    for i in range(N):
        a = pr["point_anchor"][i]
        if pr["point_active"][i] and a >= 0 and pr["kf_active"][a]:
            p = [f(float(v)) for v in pr["points"][i]]
            s1_points[i] = [float(v) for v in act(inv(S1[a]), act(T[a], p))]
    s3_points = s3_in.copy()
    for i in range(N):
        a = pr["point_anchor"][i]
        if not pr["point_active"][i] and a >= 0:
            p = [f(float(v)) for v in s3_in[i]]
            s3_points[i] = [float(v) for v in act(inv(pose(s3_opt[a])), act(pose(s3_s1[a]), p))]
    return s1_poses, s1_points, s3_points


def main():
    out = dict(names=np.array(lcc.NAMES), factor=np.float64(FACTOR), quantities=np.array(QUANTITIES))
    worst = {q: np.zeros(len(lcc.NAMES)) for q in QUANTITIES}
    for k, name in enumerate(lcc.NAMES):
        pr = lcc.make(name)
        m_s1, m_p1, _ = lcm.stage1(pr)
        opt = lcc.stated_opt_poses(pr, m_s1)
        _, m_p3, _ = lcm.stage3(pr, m_s1, opt, m_p1)
        m0 = lcm.loop_correct(pr, None, iters=0)                       # the optimiser bypassed
        s1_poses, s1_points, s3_points = truth(pr, m_s1, opt, m_p1)
        worst["s1_poses"][k] = lcc.pose_distance(m_s1, s1_poses)
        worst["s1_points"][k] = lcc.point_distance(m_p1, s1_points)
        other = pr["point_active"] == 0
        worst["identity"][k] = lcc.point_distance(m0["points"][other], s1_points[other])
        worst["s3_points"][k] = lcc.point_distance(m_p3, s3_points)
        out.update({f"{name}_s1_poses": s1_poses, f"{name}_s1_points": s1_points, f"{name}_s3_s1_poses": m_s1, f"{name}_s3_in_points": m_p1,
                    f"{name}_s3_opt_poses": opt, f"{name}_s3_points": s3_points})
        print(f"{name:10s} P {pr['P']:4d} N {pr['N']:5d}  model: " + "  ".join(f"{q} {worst[q][k]:.2e}" for q in QUANTITIES))
    for q in QUANTITIES:
        out[f"model_{q}"] = worst[q]
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
