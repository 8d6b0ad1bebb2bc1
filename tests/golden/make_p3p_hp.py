"""tests/golden/p3p_hp.npz: the perspective-three-point problem to 60 digits -- the yardstick of the minimal solver of
ssvio_amd/csrc/pnp.hip (p3p_solve) and of its model tools/pnp_model.py::p3p, which are otherwise only compared with each other.

The route shares nothing with the solver's (a pencil of cones, a cubic, a plane split).  From the exact values of the stored doubles
(K, X, uv): unit bearings and their cosines; with depths s1, s2 = u s1, s3 = v s1 the three distance equations lose s1 and leave two
quadratics in u whose difference is linear in u -- u = N(v) / D(v) -- and substituting gives the classical quartic in the depth ratio v
(Grunert 1841; Fischler & Bolles 1981).  mpmath.polyroots solves it at 2 x DPS digits; real roots give (s1, s2, s3), mpmath.findroot
polishes them on the three distance equations, duplicates are merged, triples with a depth <= 0 dropped, and (R, t) is built from the
frames of the two triangles.  Every number is rounded to double at the very end.

Per case: n (solutions), q (the quaternion of R, qw >= 0, computed at 60 digits without a branch on the trace; the file holds it in
place of R to stay small, and p3p_cases.load turns it back), t, sigma_min = the smallest singular value of the 3x3 Jacobian of the three quadrics at the solution in the
solver's normalisation (a_ij / (a12 + a13 + a23), depths / its square root), min_sep = the smallest pairwise distance of the solutions
in normalised depth space (inf with fewer than two), gen = which solution is the generating pose of tests/p3p_cases.py (R within 1e-6,
t within 1e-6 max(1, |X|max)) or -1, stable = the number of solutions survives every one of PERTURB perturbations of the inputs by
1e-6 relative (points by 1e-6 of the longest side, bearings by 1e-6 rad).

    well = n >= 1 and every sigma_min >= 1e-4 and min_sep >= 1e-3 and stable

is a condition on the inputs, read off the reference alone; everything else is treated as ill-posed whatever class it was built for.

The model's own error against the reference is measured here, per class over the well-posed cases, and stored (model_worst; err =
max(max |R - R_ref|, |t - t_ref| / max(1, |X|max)) of the matched solution), with the bar max(1e-9, 4 x worst) the kernel is held to
(4: the project's margin for an equivalent summation order, as in tri_hp.npz -- the kernel is meant to have none).  So are, at the
reference depths ROUNDED TO DOUBLE and in the solver's own double arithmetic, the largest residual of the three quadrics relative to
l1^2 + l2^2 + l3^2 (ref_resid_worst) and the relative difference of the squared areas of the two triangles (ref_area_worst): the
solver's two validity cut-offs are stated against them (tools/pnp_model.py: RESID_CUT, AREA_CUT; model_resid_worst and model_area_worst are
what the model's own valid solutions leave).  No number here
comes from the kernel.

    python tests/golden/make_p3p_hp.py        (needs mpmath; about a minute)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import p3p_cases as pc  # noqa: E402
from tools import pnp_model as pm  # noqa: E402

OUT = os.path.join(HERE, "p3p_hp.npz")
DPS = 60
PERTURB = 4
SIGMA_MIN, MIN_SEP = 1e-4, 1e-3
GEN_TOL = 1e-6


def _poly_mul(a, b):
    """coefficient lists, lowest degree first"""
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = out[i + j] + x * y
    return out


def _poly_add(a, b):
    n = max(len(a), len(b))
    return [(a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0) for i in range(n)]


def depths_hp(mp, y, A, polish=True):
    """unit bearings y [3][3] and squared sides A = (A12, A13, A23) -> list of (s1, s2, s3), every real solution with positive depths"""
    f = mp.mpf
    c12 = sum(y[0][k] * y[1][k] for k in range(3))
    c13 = sum(y[0][k] * y[2][k] for k in range(3))
    c23 = sum(y[1][k] * y[2][k] for k in range(3))
    A12, A13, A23 = A
    # s1^2 (1 + u^2 - 2 u c12) = A12,  s1^2 (1 + v^2 - 2 v c13) = A13,  s1^2 (u^2 + v^2 - 2 u v c23) = A23;  q(v) = 1 + v^2 - 2 v c13
    q = [f(1), -2 * c13, f(1)]
    # A13 (u^2 + v^2 - 2 u v c23) - A23 q = 0  and  A13 (1 + u^2 - 2 u c12) - A12 q = 0;  their difference is linear in u:  u D = N
    N = _poly_add([-A13, f(0), A13], [(A12 - A23) * t for t in q])
    D = [-2 * A13 * c12, 2 * A13 * c23]
    # substitute into the second, times D^2:  A13 N^2 - 2 A13 c12 N D + (A13 - A12 q) D^2 = 0
    DD = _poly_mul(D, D)
    quartic = _poly_add(_poly_add([A13 * t for t in _poly_mul(N, N)], [-2 * A13 * c12 * t for t in _poly_mul(N, D)]),
                        _poly_mul(_poly_add([A13], [-A12 * t for t in q]), DD))
    scale = max(abs(t) for t in quartic)
    if not scale > 0:
        return []
    coeffs = [t / scale for t in reversed(quartic)]
    while coeffs and abs(coeffs[0]) < f(10) ** (-DPS):                 # (a vanishing leading coefficient: a root at infinity)
        coeffs = coeffs[1:]
    if len(coeffs) < 2:
        return []
    with mp.workdps(2 * DPS):
        try:
            roots = mp.polyroots(coeffs, maxsteps=500, extraprec=8 * DPS)
        except mp.libmp.libhyper.NoConvergence:
            return []
    sols = []
    for r in roots:
        if abs(mp.im(r)) > f(10) ** (-DPS // 2) * max(1, abs(r)):
            continue
        v = mp.re(r)
        den = D[0] + D[1] * v
        qv = q[0] + q[1] * v + q[2] * v * v
        if not qv > 0:
            continue
        us = []
        if abs(den) > f(10) ** (-DPS // 2) * A13:
            us.append((N[0] + N[1] * v + N[2] * v * v) / den)
        else:                                                          # both quadratics share the root: take it from the second one
            disc = c12 * c12 - (1 - A12 * qv / A13)
            if disc >= 0:
                us += [c12 + mp.sqrt(disc), c12 - mp.sqrt(disc)]
        for u in us:
            s1 = mp.sqrt(A13 / qv)
            s = [s1, u * s1, v * s1]
            if polish:
                def eqs(a, b, c):
                    return (a * a + b * b - 2 * a * b * c12 - A12, a * a + c * c - 2 * a * c * c13 - A13, b * b + c * c - 2 * b * c * c23 - A23)
                try:
                    z = mp.findroot(eqs, s, tol=f(10) ** (-2 * DPS + 10), maxsteps=50)
                    z = [z[0], z[1], z[2]]
                    if max(abs(z[k] - s[k]) for k in range(3)) < f(10) ** (-DPS // 3) * max(abs(t) for t in s):
                        s = z
                except (ValueError, ZeroDivisionError):
                    pass                                               # a singular Jacobian (a multiple root): the unpolished root stands
            res = max(abs(s[0] ** 2 + s[1] ** 2 - 2 * s[0] * s[1] * c12 - A12), abs(s[0] ** 2 + s[2] ** 2 - 2 * s[0] * s[2] * c13 - A13),
                      abs(s[1] ** 2 + s[2] ** 2 - 2 * s[1] * s[2] * c23 - A23))
            if res > f(10) ** (-DPS // 3) * (A12 + A13 + A23):
                continue
            if not (s[0] > 0 and s[1] > 0 and s[2] > 0):
                continue
            if any(max(abs(s[k] - o[k]) for k in range(3)) < f(10) ** (-DPS // 3) * max(s) for o in sols):
                continue
            sols.append(s)
    return sols


def _bearings(mp, K, uv):
    f = mp.mpf
    y = []
    for i in range(3):
        bx, by = (f(float(uv[i][0])) - f(float(K[2]))) / f(float(K[0])), (f(float(uv[i][1])) - f(float(K[3]))) / f(float(K[1]))
        n = mp.sqrt(bx * bx + by * by + 1)
        y.append([bx / n, by / n, 1 / n])
    return y


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _quat(mp, R):
    """(qx qy qz qw) of a rotation, qw >= 0: the column of largest norm of 1/4 of the matrix (1 + R ...) whose columns are all
    multiples of q -- no branch on the trace"""
    M = [[1 + R[0][0] - R[1][1] - R[2][2], R[0][1] + R[1][0], R[0][2] + R[2][0], R[2][1] - R[1][2]],
         [R[0][1] + R[1][0], 1 - R[0][0] + R[1][1] - R[2][2], R[1][2] + R[2][1], R[0][2] - R[2][0]],
         [R[0][2] + R[2][0], R[1][2] + R[2][1], 1 - R[0][0] - R[1][1] + R[2][2], R[1][0] - R[0][1]],
         [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1], 1 + R[0][0] + R[1][1] + R[2][2]]]
    col = max(range(4), key=lambda k: M[k][k])
    q = [M[r][col] for r in range(4)]
    n = mp.sqrt(sum(v * v for v in q))
    if q[3] < 0:
        n = -n
    return [v / n for v in q]


def solve_hp(K, X, uv, seed):
    """one case at 60 digits -> dict(n, R [4, 3, 3], t [4, 3], q [4, 4], sigma_min [4], l [4, 3], min_sep, stable)"""
    import mpmath as mp
    mp.mp.dps = DPS
    f = mp.mpf
    out = dict(n=0, R=np.zeros((4, 3, 3)), t=np.zeros((4, 3)), q=np.zeros((4, 4)), sigma_min=np.zeros(4), l=np.zeros((4, 3)), min_sep=np.inf, stable=False)
    if not (np.isfinite(X).all() and np.isfinite(uv).all()):
        return out
    Xm = [[f(float(X[i][k])) for k in range(3)] for i in range(3)]
    y = _bearings(mp, K, uv)

    def sides(P):
        d2 = lambda a, b: sum((a[k] - b[k]) ** 2 for k in range(3))
        return d2(P[0], P[1]), d2(P[0], P[2]), d2(P[1], P[2])
    A = sides(Xm)
    S = A[0] + A[1] + A[2]
    if not S > 0:
        return out
    sols = depths_hp(mp, y, A)
    assert len(sols) <= 4, len(sols)
    sq = mp.sqrt(S)
    b = [-2 * sum(y[i][k] * y[j][k] for k in range(3)) for i, j in ((0, 1), (0, 2), (1, 2))]
    p1 = [Xm[1][k] - Xm[0][k] for k in range(3)]
    p2 = [Xm[2][k] - Xm[0][k] for k in range(3)]
    p3 = _cross(p1, p2)
    det = sum(t * t for t in p3)
    if not det > 0:                                                    # collinear points: no frame, no pose
        return out
    w1, w2 = _cross(p2, p3), _cross(p3, p1)
    sols.sort(key=lambda s: float(s[0]))
    ls = []
    for n, s in enumerate(sols):
        Y = [[s[i] * y[i][k] for k in range(3)] for i in range(3)]
        q1 = [Y[1][k] - Y[0][k] for k in range(3)]
        q2 = [Y[2][k] - Y[0][k] for k in range(3)]
        q3 = _cross(q1, q2)
        R = [[(q1[a] * w1[c] + q2[a] * w2[c] + q3[a] * p3[c]) / det for c in range(3)] for a in range(3)]
        t = [Y[0][a] - sum(R[a][c] * Xm[0][c] for c in range(3)) for a in range(3)]
        l = [s[k] / sq for k in range(3)]
        J = mp.matrix([[2 * l[0] + b[0] * l[1], 2 * l[1] + b[0] * l[0], 0], [2 * l[0] + b[1] * l[2], 0, 2 * l[2] + b[1] * l[0]],
                       [0, 2 * l[1] + b[2] * l[2], 2 * l[2] + b[2] * l[1]]])
        sv = mp.svd_r(J, compute_uv=False)
        out["R"][n] = [[float(v) for v in row] for row in R]
        out["t"][n] = [float(v) for v in t]
        out["q"][n] = [float(v) for v in _quat(mp, R)]
        out["sigma_min"][n] = float(min(sv[i] for i in range(3)))
        out["l"][n] = [float(v) for v in l]
        ls.append(l)
    out["n"] = len(sols)
    for i in range(len(ls)):
        for j in range(i):
            out["min_sep"] = min(out["min_sep"], float(mp.sqrt(sum((ls[i][k] - ls[j][k]) ** 2 for k in range(3)))))
    # does the number of solutions survive a perturbation of 1e-6?  (the quartic's real roots are then not about to turn complex, nor a depth
    # about to change sign)
    rng = np.random.default_rng(seed)
    side = mp.sqrt(max(A))
    stable = out["n"] >= 1
    for _ in range(PERTURB if stable else 0):
        dX = rng.choice([-1.0, 1.0], (3, 3))
        dy = rng.choice([-1.0, 1.0], (3, 3))
        Xp = [[Xm[i][k] + f("1e-6") * side * f(float(dX[i][k])) for k in range(3)] for i in range(3)]
        yp = []
        for i in range(3):
            v = [y[i][k] + f("1e-6") * f(float(dy[i][k])) for k in range(3)]
            n = mp.sqrt(sum(t * t for t in v))
            yp.append([t / n for t in v])
        if len(depths_hp(mp, yp, sides(Xp), polish=False)) != out["n"]:
            stable = False
            break
    out["stable"] = bool(stable)
    return out


def ref_residual(K, X, uv, l):
    """at the double depths l (normalised), in the solver's own double arithmetic: the largest of the three quadrics relative to
    l1^2 + l2^2 + l3^2, and the relative difference of the squared areas of the two triangles"""
    r, a = pm.solution_checks(K, X, uv, l)
    return float(np.abs(r).max() / (l * l).sum()), float(abs(a))


def main():
    cls, names, X, uv, R_gen, t_gen = pc.arrays()
    N = len(cls)
    n = np.zeros(N, np.int32); R = np.zeros((N, 4, 3, 3)); t = np.zeros((N, 4, 3)); q = np.zeros((N, 4, 4)); sig = np.zeros((N, 4)); ln = np.zeros((N, 4, 3))
    sep = np.full(N, np.inf); stable = np.zeros(N, bool); gen = np.full(N, -1, np.int32)
    for i in range(N):
        o = solve_hp(pc.K, X[i], uv[i], 7000 + i)
        q[i] = o["q"]
        for s in range(o["n"]):
            o["R"][s] = pc.quat_to_rot(o["q"][s])                        # what the fixture's readers see (it stores q, not R)
        n[i], R[i], t[i], sig[i], ln[i], sep[i], stable[i] = o["n"], o["R"], o["t"], o["sigma_min"], o["l"], o["min_sep"], o["stable"]
        xmax = np.abs(X[i]).max() if np.isfinite(X[i]).all() else 1.0
        for s in range(n[i]):
            if np.abs(R[i, s] - R_gen[i]).max() < GEN_TOL and np.linalg.norm(t[i, s] - t_gen[i]) < GEN_TOL * max(1.0, xmax):
                gen[i] = s
    well = np.array([n[i] >= 1 and (sig[i, :n[i]] >= SIGMA_MIN).all() and sep[i] >= MIN_SEP and stable[i] for i in range(N)])
    # the model against the reference, and the residual of the rounded reference solutions
    model_worst = np.zeros(len(pc.CLASSES)); resid_worst = area_worst = 0.0; model_checks = [0.0, 0.0]
    for i in np.nonzero(well)[0]:
        trace = []
        valid, Rs, ts = pm.p3p(pc.K, X[i], uv[i], trace=trace)
        for k, v in trace:                                             # what the model's own solutions leave of the two conditions
            if valid[k % 4]:
                model_checks[k // 4] = max(model_checks[k // 4], float(v))
        pairs, extra, missing = pc.match(valid, Rs, ts, n[i], R[i], t[i], np.abs(X[i]).max())
        if extra or missing:
            print(f"  {names[i]}: model has {len(extra)} extra, {len(missing)} missing of {n[i]}")
        for s, r, e in pairs:
            model_worst[cls[i]] = max(model_worst[cls[i]], e)
        for s in range(n[i]):
            rq, ra = ref_residual(pc.K, X[i], uv[i], ln[i, s])
            resid_worst, area_worst = max(resid_worst, rq), max(area_worst, ra)
    bar = np.maximum(1e-9, 4.0 * model_worst)
    np.savez_compressed(OUT, K=pc.K, cls=cls, classes=np.array(pc.CLASSES), names=names, X=X, uv=uv, n=n, q=q, t=t,
                        sigma_min=sig.astype(np.float32), min_sep=sep.astype(np.float32), stable=stable, gen=gen, well=well, model_worst=model_worst, bar=bar,
                        ref_resid_worst=np.float64(resid_worst), ref_area_worst=np.float64(area_worst),
                        model_resid_worst=np.float64(model_checks[0]), model_area_worst=np.float64(model_checks[1]))
    print(f"{OUT}: {N} cases, {os.path.getsize(OUT)} bytes; reference rounded to double: quadrics {resid_worst:.3e}, areas {area_worst:.3e}; "
          f"the model's own solutions: {model_checks[0]:.3e}, {model_checks[1]:.3e}")
    for k, name in enumerate(pc.CLASSES):
        m = cls == k
        print(f"  {name:11s} {m.sum():4d} cases, {int((m & well).sum()):4d} well-posed, solutions {np.bincount(n[m], minlength=5).tolist()}, "
              f"generating pose found in {int((gen[m] >= 0).sum())}; model worst {model_worst[k]:.2e}  bar {bar[k]:.2e}")


if __name__ == "__main__":
    main()
