"""Executable model of the P3P-RANSAC of ssvio_amd/csrc/pnp.hip (ssx_pnp_ransac), the library's restatement of the
cv::solvePnPRansac call of LoopClosing::ComputeCorrectPose (reference: src/ssvio/loopclosing.cpp:205-206).  OpenCV's result
cannot be pinned (its sampler and its early exit belong to one build of one library), so the contract is this file: the
same counter-based sampler, the same minimal solver written operation by operation as the kernel writes it, the same inlier
rule and the same selection.  Every scalar is a numpy float64 and every operation is one IEEE operation (the kernel is built
with -ffp-contract=off), so the kernel and this file agree to the bit: tests/test_p3p_gpu.py asserts it on R, t and the pose of
every slot over tests/golden/p3p_hp.npz.  tests/test_pnp_model.py checks the model against ground truth, tests/test_p3p_cases.py its
minimal solver against a 60-digit reference (complete, accurate, sound), tests/test_loop_pose_gpu.py the kernel against the model.

sample_triple   three distinct indices of [0, M) as a pure function of (seed, h, M)
p3p             up to four (R, t) for three bearings and three points
pnp_ransac      H hypotheses, all scored (no confidence-driven early exit: every hypothesis is independent work of one
                launch), the winner = most inliers, then the lowest hypothesis, then the lowest solution

The minimal solver.  With unit bearings y_i and depths l_i, |l_i y_i - l_j y_j|^2 = |X_i - X_j|^2 are three quadrics
l' M_ij l = a_ij.  Two combinations without constant term, D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23, span a pencil
of cones; a real root g of the cubic det(Da + g Db) = 0 (Newton steps from a start beyond the cubic's turning points) gives a
degenerate member, which splits into two planes through the origin (adjugate and one square root).  On each plane the other
cone leaves a homogeneous quadratic: two depth directions per plane, scaled by the sum of the three quadrics, polished by
three Gauss-Newton steps on the three quadrics, and turned into (R, t) by the frames the two triangles span.  Only
+ - * / and sqrt are used.  (The construction follows Persson & Nordberg, "Lambda Twist: An Accurate Fast Robust
Perspective Three Point (P3P) Solver", ECCV 2018; the splitting of the degenerate cone is the classical one of projective
geometry.)

Where both D1 and D2 are plane pairs themselves (det D1 = det D2 = 0 in double: an equilateral triangle seen on its axis, a12 = a23 and
b12 = b23) there is no cubic to solve: g = 0, the member is Da.  (Before, this returned nothing where the reference has four poses.)

What makes a slot valid.  Finite and positive depths are not enough: a slot is a hypothesis that is scored with R and whose
rot_to_quat(R) is handed to the refinement, so it has to be a pose.  Two conditions, both measured against the 60-digit reference
(tests/golden/make_p3p_hp.py; over its well-posed cases, at the reference's depths rounded to double, in this file's arithmetic):
  RESID_CUT  the three quadrics hold to 5.9e-9 (l1^2 + l2^2 + l3^2) = 2^24 x the reference's worst, 3.52e-16.  Three Gauss-Newton steps
             end at 1e-16 except next to a double root, where they leave a continuum of residuals r whose poses miss their own pixels by
             about 2e3 r px (40 000 random triples: r up to 6e-9); the cut keeps that under 2e-5 px and every hypothesis of
             tests/loop_pose_cases.py (largest 4.6e-12) as it was.
  AREA_CUT   the triangle of the solution has the area of the points' triangle: | |q1 x q2|^2 / |p1 x p2|^2 - 1 | <= 1e-6 = 7.8e5 x the
             reference's worst, 1.28e-12 (a 1 cm triangle at 50 m, where this file's own depths leave 1.6e-8).  The sides of a needle
             (height 1e-6 of its length) hold to rounding while its height is off by percents; the frames then stretch R along the
             normal by that ratio, and R is no rotation (|R R' - I| of 0.02 and 0.06 were returned as valid).  1e-6 is a stretch of 5e-7:
             under 1e-3 px at any bearing the camera has.
"""
import numpy as np

F = np.float64
NEWTON_STEPS = 16      # on the cubic
GN_STEPS = 3           # on the three quadrics
RESID_CUT = 5.9e-9     # on the three quadrics, relative to l1^2 + l2^2 + l3^2
AREA_CUT = 1e-6        # on |q1 x q2|^2 / |p1 x p2|^2 - 1
MIN_INLIERS = 4        # a hypothesis explains its own three points: a pose needs one more
MAX_ITERS = 4096       # SSX_PNP_MAX_ITERS


def mix32(x):
    """a 32-bit integer mixer (two multiplications, three xor-shifts)"""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def sample_triple(seed, h, M):
    """three distinct indices of [0, M), M >= 3: draws from [0, M), [0, M - 1), [0, M - 2) by multiply-high, each lifted past the
    earlier picks in ascending order"""
    r = [mix32((seed & 0xFFFFFFFF) ^ mix32(3 * h + k + 1)) for k in range(3)]
    a = (r[0] * M) >> 32
    b = (r[1] * (M - 1)) >> 32
    c = (r[2] * (M - 2)) >> 32
    b += b >= a
    lo, hi = min(a, b), max(a, b)
    c += c >= lo
    c += c >= hi
    return int(a), int(b), int(c)


def sample_triples(seed, M, H):
    return np.array([sample_triple(seed, h, M) for h in range(H)], dtype=np.int32).reshape(H, 3)


def _adj(m):
    """adjugate of the symmetric (m00 m01 m02 m11 m12 m22), same layout"""
    m00, m01, m02, m11, m12, m22 = m
    return (m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11, m00 * m22 - m02 * m02, m01 * m02 - m00 * m12,
            m00 * m11 - m01 * m01)


def _dot_sym(a, b):
    """trace(A B) of two symmetric matrices"""
    return a[0] * b[0] + a[3] * b[3] + a[5] * b[5] + F(2.0) * (a[1] * b[1] + a[2] * b[2] + a[4] * b[4])


def _quad(q, u, v):
    """u' Q v for the symmetric Q"""
    return (u[0] * (q[0] * v[0] + q[1] * v[1] + q[2] * v[2]) + u[1] * (q[1] * v[0] + q[3] * v[1] + q[4] * v[2])
            + u[2] * (q[2] * v[0] + q[4] * v[1] + q[5] * v[2]))


def _cubic_root(b, c, d):
    """a real root of r^3 + b r^2 + c r + d"""
    disc = b * b - F(3.0) * c
    if not _fin(disc):                              # an overflow is handed back before it is compared: the caller tests the result
        return disc
    if disc > 0:
        v = np.sqrt(disc)
        t1 = (-b - v) / F(3.0)
        k = ((t1 + b) * t1 + c) * t1 + d
        if not _fin(k):
            return k
        if k > 0:                                   # the local maximum is above the axis: the root left of it
            r = t1 - np.sqrt(k / v)
        else:                                       # else the root right of the local minimum
            t2 = (-b + v) / F(3.0)
            k = ((t2 + b) * t2 + c) * t2 + d
            r = t2 + np.sqrt(-k / v)
    else:                                           # monotone: from the inflection
        r = -b / F(3.0)
        if abs((F(3.0) * r + F(2.0) * b) * r + c) < 1e-4:
            r = r + F(1.0)
    for _ in range(NEWTON_STEPS):
        fx = ((r + b) * r + c) * r + d
        fp = (F(3.0) * r + F(2.0) * b) * r + c
        r = r - fx / fp
    return r


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _fin(*v):
    return all(np.isfinite(x) for x in v)


def p3p(K, X, uv, trace=None):
    """X [3, 3] points, uv [3, 2] pixels -> (valid [4] bool, R [4, 3, 3], t [4, 3]).  Solution 2 p + r is root r of plane p.
    trace: a list that receives (slot, largest |quadric residual| / (l1^2 + l2^2 + l3^2)) of every candidate that reaches that cut-off, and (4 + slot, the relative
    difference of the two squared areas) of every one that reaches the second."""
    with np.errstate(all="ignore"):
        return _p3p(K, X, uv, trace)


def _p3p(K, X, uv, trace=None):
    fx, fy, cx, cy = (F(v) for v in K)
    valid = np.zeros(4, bool)
    Rs = np.zeros((4, 3, 3))
    ts = np.zeros((4, 3))
    X = [[F(X[i][k]) for k in range(3)] for i in range(3)]
    y = []
    for i in range(3):
        bx = (F(uv[i][0]) - cx) / fx
        by = (F(uv[i][1]) - cy) / fy
        n = np.sqrt(bx * bx + by * by + F(1.0))
        y.append((bx / n, by / n, F(1.0) / n))

    def d2(p, q):
        dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
        return dx * dx + dy * dy + dz * dz

    def dot(p, q):
        return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]

    A12, A13, A23 = d2(X[0], X[1]), d2(X[0], X[2]), d2(X[1], X[2])
    S = A12 + A13 + A23
    if not (_fin(S) and S > 0):
        return valid, Rs, ts
    a12, a13, a23 = A12 / S, A13 / S, A23 / S
    b12, b13, b23 = F(-2.0) * dot(y[0], y[1]), F(-2.0) * dot(y[0], y[2]), F(-2.0) * dot(y[1], y[2])
    h12, h13, h23 = F(0.5) * b12, F(0.5) * b13, F(0.5) * b23
    Z = F(0.0)
    D1 = (a23, a23 * h12, Z, a23 - a12, -(a12 * h23), -a12)
    D2 = (a23, Z, a23 * h13, -a13, -(a13 * h23), a23 - a13)
    J1, J2 = _adj(D1), _adj(D2)
    det1 = D1[0] * J1[0] + D1[1] * J1[1] + D1[2] * J1[2]
    det2 = D2[0] * J2[0] + D2[1] * J2[1] + D2[2] * J2[2]
    if not _fin(det1, det2):
        return valid, Rs, ts
    if abs(det2) >= abs(det1):
        Da, Db, Ja, Jb, deta, detb = D1, D2, J1, J2, det1, det2
    else:
        Da, Db, Ja, Jb, deta, detb = D2, D1, J2, J1, det2, det1
    g = F(0.0)                                       # detb = 0, hence deta = 0: Da is a plane pair itself (a12 = a23 and b12 = b23, say)
    if abs(detb) > 0:
        cb, cc, cd = _dot_sym(Da, Jb) / detb, _dot_sym(Ja, Db) / detb, deta / detb   # (a tiny detb can make them infinite)
        if not _fin(cb, cc, cd):
            return valid, Rs, ts
        g = _cubic_root(cb, cc, cd)
        if not _fin(g):
            return valid, Rs, ts
    C = tuple(Da[k] + g * Db[k] for k in range(6))
    Q = Db if abs(g) <= 1 else Da                    # on the planes Da = -g Db: the one that is not small there
    # C = l m' + m l' with p = l x m: -adj(C) = p p', and C + [p]x = 2 m l'
    Ja = _adj(C)
    B = tuple(-v for v in Ja)
    if not _fin(*B):
        return valid, Rs, ts
    if B[0] >= B[3] and B[0] >= B[5]:
        bii, p = B[0], (B[0], B[1], B[2])
    elif B[3] >= B[5]:
        bii, p = B[3], (B[1], B[3], B[4])
    else:
        bii, p = B[5], (B[2], B[4], B[5])
    if not bii > 0:
        return valid, Rs, ts
    beta = np.sqrt(bii)
    p = (p[0] / beta, p[1] / beta, p[2] / beta)
    N = ((C[0], C[1] - p[2], C[2] + p[1]), (C[1] + p[2], C[3], C[4] - p[0]), (C[2] - p[1], C[4] + p[0], C[5]))
    if not _fin(*N[0], *N[1], *N[2]):
        return valid, Rs, ts
    best, bj, bk = F(-1.0), 0, 0
    for j in range(3):
        for k in range(3):
            if abs(N[j][k]) > best:
                best, bj, bk = abs(N[j][k]), j, k
    planes = ((N[bj][0], N[bj][1], N[bj][2]), (N[0][bk], N[1][bk], N[2][bk]))
    sqS = np.sqrt(S)
    for pl in range(2):
        n = planes[pl]
        u = (n[1] - n[2], n[2] - n[0], n[0] - n[1])              # n x (1, 1, 1): never zero for a plane that meets the positive octant
        v = _cross(n, u)
        qa, qb, qc = _quad(Q, u, u), _quad(Q, u, v), _quad(Q, v, v)
        disc = qb * qb - qa * qc
        if not (_fin(disc) and disc >= 0):
            continue
        sq = np.sqrt(disc)
        q = -(qb + sq) if qb >= 0 else -(qb - sq)
        for r in range(2):
            s, t = (q, qa) if r == 0 else (qc, q)               # the two roots (s : t) of qa s^2 + 2 qb s t + qc t^2
            l1, l2, l3 = s * u[0] + t * v[0], s * u[1] + t * v[1], s * u[2] + t * v[2]
            w = F(2.0) * (l1 * l1 + l2 * l2 + l3 * l3) + b12 * (l1 * l2) + b13 * (l1 * l3) + b23 * (l2 * l3)   # = a12 + a13 + a23 = 1
            if not (_fin(w) and w > 0):
                continue
            sc = F(1.0) / np.sqrt(w)
            if l1 < 0:
                sc = -sc
            l1, l2, l3 = l1 * sc, l2 * sc, l3 * sc
            for _ in range(GN_STEPS):
                r0 = l1 * l1 + l2 * l2 + b12 * (l1 * l2) - a12
                r1 = l1 * l1 + l3 * l3 + b13 * (l1 * l3) - a13
                r2 = l2 * l2 + l3 * l3 + b23 * (l2 * l3) - a23
                j00, j01 = F(2.0) * l1 + b12 * l2, F(2.0) * l2 + b12 * l1
                j10, j12 = F(2.0) * l1 + b13 * l3, F(2.0) * l3 + b13 * l1
                j21, j22 = F(2.0) * l2 + b23 * l3, F(2.0) * l3 + b23 * l2
                det = -(j00 * (j12 * j21)) - j01 * (j10 * j22)
                # Cramer for [[j00 j01 0] [j10 0 j12] [0 j21 j22]]
                e1 = (r0 * (-(j12 * j21)) - j01 * (r1 * j22 - j12 * r2)) / det
                e2 = (j00 * (r1 * j22 - j12 * r2) - r0 * (j10 * j22)) / det
                e3 = (j00 * (-(r1 * j21)) - j01 * (j10 * r2) + r0 * (j10 * j21)) / det
                l1, l2, l3 = l1 - e1, l2 - e2, l3 - e3
            if not (_fin(l1, l2, l3) and l1 > 0 and l2 > 0 and l3 > 0):
                continue
            # a solution satisfies the three quadrics: where the iteration has not arrived (a plane pair that is none, a multiple root)
            # there is no pose to hand on
            r0 = l1 * l1 + l2 * l2 + b12 * (l1 * l2) - a12
            r1 = l1 * l1 + l3 * l3 + b13 * (l1 * l3) - a13
            r2 = l2 * l2 + l3 * l3 + b23 * (l2 * l3) - a23
            cut = F(RESID_CUT) * (l1 * l1 + l2 * l2 + l3 * l3)
            if trace is not None:
                trace.append((2 * pl + r, max(abs(r0), abs(r1), abs(r2)) / (l1 * l1 + l2 * l2 + l3 * l3)))
            if not (_fin(r0, r1, r2, cut) and abs(r0) <= cut and abs(r1) <= cut and abs(r2) <= cut):
                continue
            l1, l2, l3 = l1 * sqS, l2 * sqS, l3 * sqS
            Y = [(l1 * y[0][0], l1 * y[0][1], l1 * y[0][2]), (l2 * y[1][0], l2 * y[1][1], l2 * y[1][2]), (l3 * y[2][0], l3 * y[2][1], l3 * y[2][2])]
            p1 = (X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2])
            p2 = (X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2])
            p3 = _cross(p1, p2)
            q1 = (Y[1][0] - Y[0][0], Y[1][1] - Y[0][1], Y[1][2] - Y[0][2])
            q2 = (Y[2][0] - Y[0][0], Y[2][1] - Y[0][1], Y[2][2] - Y[0][2])
            q3 = _cross(q1, q2)
            det = p3[0] * p3[0] + p3[1] * p3[1] + p3[2] * p3[2]
            if not (_fin(det) and det > 0):
                continue
            # ... and spans a triangle congruent to the points': a needle's height is lost in the rounding of its sides, and the frames
            # below would stretch R along the normal by the ratio of the two areas
            area = q3[0] * q3[0] + q3[1] * q3[1] + q3[2] * q3[2]
            acut = F(AREA_CUT) * det
            if trace is not None:
                trace.append((4 + 2 * pl + r, abs(area - det) / det))
            if not (_fin(area, acut) and abs(area - det) <= acut):
                continue
            w1, w2 = _cross(p2, p3), _cross(p3, p1)              # rows of the inverse of [p1 p2 p3], times det
            R = [[(q1[a] * w1[c] + q2[a] * w2[c] + q3[a] * p3[c]) / det for c in range(3)] for a in range(3)]
            t = [Y[0][a] - (R[a][0] * X[0][0] + R[a][1] * X[0][1] + R[a][2] * X[0][2]) for a in range(3)]
            if not _fin(*R[0], *R[1], *R[2], *t):
                continue
            k = 2 * pl + r
            valid[k] = True
            Rs[k] = np.array(R, dtype=np.float64)
            ts[k] = np.array(t, dtype=np.float64)
    return valid, Rs, ts


def solution_checks(K, X, uv, l):
    """what _p3p asks of a solution before it hands it on, at the normalised depths l (= depths / sqrt(A12 + A13 + A23)) and in _p3p's
    operations -> (the three quadrics [3], |q1 x q2|^2 / |p1 x p2|^2 - 1: the squared areas of the two triangles)"""
    fx, fy, cx, cy = (F(v) for v in K)
    y = []
    for i in range(3):
        bx = (F(uv[i][0]) - cx) / fx
        by = (F(uv[i][1]) - cy) / fy
        n = np.sqrt(bx * bx + by * by + F(1.0))
        y.append((bx / n, by / n, F(1.0) / n))
    X = [[F(X[i][k]) for k in range(3)] for i in range(3)]

    def d2(p, q):
        dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
        return dx * dx + dy * dy + dz * dz

    def dot(p, q):
        return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]

    A12, A13, A23 = d2(X[0], X[1]), d2(X[0], X[2]), d2(X[1], X[2])
    S = A12 + A13 + A23
    a12, a13, a23 = A12 / S, A13 / S, A23 / S
    b12, b13, b23 = F(-2.0) * dot(y[0], y[1]), F(-2.0) * dot(y[0], y[2]), F(-2.0) * dot(y[1], y[2])
    l1, l2, l3 = (F(v) for v in l)
    res = np.array([l1 * l1 + l2 * l2 + b12 * (l1 * l2) - a12, l1 * l1 + l3 * l3 + b13 * (l1 * l3) - a13,
                    l2 * l2 + l3 * l3 + b23 * (l2 * l3) - a23])
    sqS = np.sqrt(S)
    l1, l2, l3 = l1 * sqS, l2 * sqS, l3 * sqS
    Y = [(l1 * y[0][0], l1 * y[0][1], l1 * y[0][2]), (l2 * y[1][0], l2 * y[1][1], l2 * y[1][2]), (l3 * y[2][0], l3 * y[2][1], l3 * y[2][2])]
    p3 = _cross([X[1][k] - X[0][k] for k in range(3)], [X[2][k] - X[0][k] for k in range(3)])
    q3 = _cross([Y[1][k] - Y[0][k] for k in range(3)], [Y[2][k] - Y[0][k] for k in range(3)])
    return res, dot(q3, q3) / dot(p3, p3) - F(1.0)


def reproj_sq(K, R, t, xyz, uv):
    """-> (depth, ex^2 + ey^2) per point, in the kernel's order of operations"""
    fx, fy, cx, cy = (F(v) for v in K)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        px = R[0, 0] * x + R[0, 1] * y + R[0, 2] * z + t[0]
        py = R[1, 0] * x + R[1, 1] * y + R[1, 2] * z + t[1]
        pz = R[2, 0] * x + R[2, 1] * y + R[2, 2] * z + t[2]
        ex = fx * (px / pz) + cx - uv[:, 0]
        ey = fy * (py / pz) + cy - uv[:, 1]
        return pz, ex * ex + ey * ey


def inlier_mask(K, R, t, xyz, uv, thr_px):
    pz, e2 = reproj_sq(K, R, t, xyz, uv)
    thr2 = F(thr_px) * F(thr_px)
    with np.errstate(all="ignore"):
        return (pz > 0) & (e2 <= thr2)


def rot_to_quat(R):
    """(qx qy qz qw), normalised, qw >= 0"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2.0
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2.0
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2.0
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2.0
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q, dtype=np.float64)
    q /= np.sqrt((q * q).sum())
    return -q if q[3] < 0 else q


def pnp_ransac(K, xyz, uv, max_iters=100, reproj_px=5.991, seed=0, detail=False):
    """-> dict(found, pose (qx qy qz qw tx ty tz), inliers uint8 [M], n_inliers, best (= 4 h + s), counts int32 [H]: the best
    count of each hypothesis[, sols: per hypothesis (valid, R, t)])"""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
    uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
    M, H = len(xyz), int(max_iters)
    counts = np.zeros(H, np.int32)
    out = dict(found=False, pose=np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64), inliers=np.zeros(M, np.uint8), n_inliers=0, best=-1,
               counts=counts, triples=None)
    if detail:
        out["sols"] = []
    if M < 3:
        return out
    out["triples"] = sample_triples(seed, M, H)
    best_key, best = None, None
    for h in range(H):
        tri = out["triples"][h]
        valid, Rs, ts = p3p(K, xyz[tri], uv[tri])
        if detail:
            out["sols"].append((valid, Rs, ts))
        for s in range(4):
            n = int(inlier_mask(K, Rs[s], ts[s], xyz, uv, reproj_px).sum()) if valid[s] else 0
            counts[h] = max(counts[h], n)
            if best_key is None or n > best_key:          # strictly more: the lowest hypothesis, then the lowest solution, keeps a tie
                best_key, best = n, (h, s, Rs[s].copy(), ts[s].copy())
    h, s, R, t = best
    out["n_inliers"] = best_key if best_key >= MIN_INLIERS else 0
    if best_key >= MIN_INLIERS:
        out.update(found=True, best=4 * h + s, pose=np.concatenate([rot_to_quat(R), t]),
                   inliers=inlier_mask(K, R, t, xyz, uv, reproj_px).astype(np.uint8))
    return out
