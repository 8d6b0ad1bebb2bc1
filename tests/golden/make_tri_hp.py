"""tests/golden/tri_hp.npz: stereo triangulation to 60 digits -- the yardstick of ssx_triangulate that is more precise than double.

The device routine (k_triangulate_*, ssvio_amd/csrc/stereo.hip) and the CPU oracle (orc_triangulate) are two different Jacobi
iterations in double; comparing them with each other says nothing about either once the null vector of the DLT matrix becomes
ill-conditioned (small disparity).  Here the 4x4 DLT matrix of ssvio::triangulation (algorithm.hpp:23-45) is formed with mpmath at
mp.dps = 60 from the exact values of the double inputs, the eigenvector of the smallest eigenvalue of A^T A (mp.eigsy) is divided
by w, and sigma3 / sigma2 is the square root of the ratio of the two smallest eigenvalues.

Inputs: three rigs, pixels in and out of the image, disparity log-spaced over 1e-6 .. 1e3 px (SAMPLES per decade) plus exactly 0 and
negative, vertical offsets 0, +-0.3, +-0.7 and a sweep 0 .. 20 px that crosses the sigma3 / sigma2 < 1e-2 decision; every point
without a pose and under two poses T_wc (one 1e4 m away).  The generator asserts that no decision is marginal: no ratio within 1e-6
relative of 1e-2, every disparity <= 0 exactly or >= 1e-6 -- the tests exclude nothing.

The error of a point is max |xyz - xyz_hp| over the coordinates divided by the largest |coordinate| of xyz_hp (rel_err).  The bar of a
disparity decade is  max(1e-9, 4 x the ORACLE's worst error in that decade)  -- 1e-9 is the tolerance the suite already holds the
kernel to against the oracle (tests/test_orb_gpu.py), 4 the factor ref_noise_floor.npz uses for a single worst value; the oracle's
error grows like 1e-13 / disparity[px], so the lowest decades get the oracle's own error as their yardstick.  The kernel is held to
these bars (tests/test_stereo_edges_gpu.py); no number here comes from the kernel.

    python tests/golden/make_tri_hp.py        (needs mpmath)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.synth import KITTI_BASELINE, KITTI_K  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tri_hp.npz")
DPS = 60
RIGS = np.array([[*KITTI_K, KITTI_BASELINE],
                 [458.654, 457.296, 367.215, 248.375, 0.110074],
                 [4000.0, 3990.0, 960.0, 540.0, 0.02]])
DECADES = np.arange(-6, 3)            # floor(log10(disparity)): 1e-6 .. just under 1e3 px
SAMPLES = 6
NO_DECADE = -99                       # disparity <= 0
VOFF = (0.0, 0.3, -0.3, 0.7, -0.7)
SWEEP = (0.0, 0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 8.0, 10.0, 13.0, 16.0, 20.0)


def poses():
    """[P, 7] (qx qy qz qw tx ty tz) and which of them are passed at all (row 0: no T_wc)"""
    T = np.array([[0, 0, 0, 1, 0, 0, 0], [0.01, -0.02, 0.03, 0.9993, 1.0, -2.0, 0.5], [-0.3, 0.5, 0.1, 0.6, 1e4, -2.5e3, 40.0]], np.float64)
    T[:, :4] /= np.linalg.norm(T[:, :4], axis=1, keepdims=True)
    return T, np.array([False, True, True])


def inputs():
    """-> uvL [N, 2], uvR [N, 2], rig_id [N], decade [N] (NO_DECADE where the disparity is not positive)"""
    uvL, uvR, rig_id = [], [], []
    for r in range(len(RIGS)):
        rng = np.random.default_rng(900 + r)
        pts = []                                                   # (disparity, vertical offset)
        for k in DECADES:
            pts += [(10.0 ** (k + (i + 0.5) / SAMPLES), VOFF[(i + k) % len(VOFF)]) for i in range(SAMPLES)]
        pts += [(0.0, 0.0), (0.0, 0.3), (-1e-7, 0.0), (-3.5, -0.7), (-250.0, 0.0)]
        for d in (300.0, 30.0, 3.0):
            pts += [(d, v if i % 2 == 0 else -v) for i, v in enumerate(SWEEP)]
        for d, voff in pts:
            uL, vL = rng.uniform(-200, 2200), rng.uniform(-100, 1200)
            uvL.append((uL, vL)); uvR.append((uL - d, vL + voff)); rig_id.append(r)
    uvL, uvR, rig_id = np.array(uvL), np.array(uvR), np.array(rig_id, np.int32)
    disp = uvL[:, 0] - uvR[:, 0]
    assert ((disp <= 0) | (disp >= 1e-6)).all(), "a disparity between 0 and 1e-6 px"
    decade = np.full(len(disp), NO_DECADE, np.int32)
    pos = disp > 0
    decade[pos] = np.floor(np.log10(disp[pos])).astype(np.int32)
    assert np.isin(decade[pos], DECADES).all() and all(((decade == k) & (rig_id == r)).sum() >= SAMPLES for k in DECADES for r in range(len(RIGS)))
    return uvL, uvR, rig_id, decade


def solve_hp(uvL, uvR, rig, T_all, has_T):
    """one point at 60 digits -> xyz [P, 3] (rounded to double at the very end), sigma3 / sigma2, ok"""
    import mpmath as mp
    mp.mp.dps = DPS
    f = mp.mpf
    fx, fy, cx, cy, base = (f(float(v)) for v in rig)
    x1, y1 = (f(float(uvL[0])) - cx) / fx, (f(float(uvL[1])) - cy) / fy
    x2, y2 = (f(float(uvR[0])) - cx) / fx, (f(float(uvR[1])) - cy) / fy
    A = mp.matrix([[-1, 0, x1, 0], [0, -1, y1, 0], [-1, 0, x2, base], [0, -1, y2, 0]])     # rows x m2 - m0, y m2 - m1 of [I|0], [I|(-b,0,0)]
    E, Q = mp.eigsy(A.T * A)
    order = sorted(range(4), key=lambda i: E[i])
    v = [Q[i, order[0]] for i in range(4)]
    ratio = mp.sqrt(abs(E[order[0]]) / E[order[1]])
    positive = f(float(uvL[0])) - f(float(uvR[0])) > 0
    # without positive disparity the point is at or behind infinity (w = 0 exactly at disparity 0): zeroed, never accepted
    p = [v[0] / v[3], v[1] / v[3], v[2] / v[3]] if positive else [f(0), f(0), f(0)]
    ok = bool(positive and ratio < f("1e-2") and p[2] > 0)
    out = np.zeros((len(T_all), 3))
    for k, (T, on) in enumerate(zip(T_all, has_T)):
        w = p
        if on:                                      # p + qw u + q x u, u = 2 q x p, + t  (the formula of both implementations, exact in q)
            qx, qy, qz, qw, tx, ty, tz = (f(float(t)) for t in T)
            ux, uy, uz = 2 * (qy * p[2] - qz * p[1]), 2 * (qz * p[0] - qx * p[2]), 2 * (qx * p[1] - qy * p[0])
            w = [p[0] + qw * ux + (qy * uz - qz * uy) + tx, p[1] + qw * uy + (qz * ux - qx * uz) + ty, p[2] + qw * uz + (qx * uy - qy * ux) + tz]
        out[k] = [float(c) for c in w]
    return out, float(ratio), ok


def rel_err(xyz, hp):
    """per point: max |xyz - hp| over the coordinates / largest |coordinate| of hp (1 where hp is the origin)"""
    scale = np.abs(hp).max(axis=-1)
    return np.abs(xyz - hp).max(axis=-1) / np.where(scale > 0, scale, 1.0)


def oracle_xyz(po, uvL, uvR, rig_id, T_all, has_T):
    """the CPU oracle over the same inputs -> xyz [P, N, 3], ok [P, N]"""
    xyz = np.zeros((len(T_all), len(uvL), 3)); ok = np.zeros((len(T_all), len(uvL)), np.uint8)
    for r, rig in enumerate(RIGS):
        m = rig_id == r
        for k, (T, on) in enumerate(zip(T_all, has_T)):
            t = po.triangulate(uvL[m], uvR[m], rig[:4], rig[4], T_wc=T if on else None)
            xyz[k, m], ok[k, m] = t["xyz"], t["ok"]
    return xyz, ok


def bars(err, decade):
    """the oracle's worst error per decade and the bar that follows from it"""
    worst = np.array([err[:, decade == k].max() for k in DECADES])
    return worst, np.maximum(1e-9, 4.0 * worst)


def main():
    from oracle import pyoracle as po
    uvL, uvR, rig_id, decade = inputs()
    T_all, has_T = poses()
    N = len(uvL)
    xyz = np.zeros((len(T_all), N, 3)); ratio = np.zeros(N); ok = np.zeros(N, np.uint8)
    for i in range(N):
        xyz[:, i], ratio[i], ok[i] = solve_hp(uvL[i], uvR[i], RIGS[rig_id[i]], T_all, has_T)
    assert (np.abs(ratio / 1e-2 - 1.0) > 1e-6).all(), "a sigma3 / sigma2 within 1e-6 relative of the threshold"
    assert (ok[decade == NO_DECADE] == 0).all() and ok.sum() > N // 2 and ((ok == 0) & (decade != NO_DECADE)).sum() >= 6
    o_xyz, o_ok = oracle_xyz(po, uvL, uvR, rig_id, T_all, has_T)
    assert (o_ok == ok[None]).all()
    err = rel_err(o_xyz, xyz)
    worst, bar = bars(err, decade)
    np.savez_compressed(OUT, uvL=uvL, uvR=uvR, rig_id=rig_id, rigs=RIGS, poses=T_all, pose_on=has_T, xyz=xyz, ratio=ratio, ok=ok,
                        decade=decade, decades=DECADES, oracle_err=err, oracle_worst_by_decade=worst, bar_by_decade=bar)
    print(f"{OUT}: {N} points, {os.path.getsize(OUT)} bytes")
    for k, w, b in zip(DECADES, worst, bar):
        print(f"  disparity 1e{k:+d} px: oracle worst {w:.2e}  bar {b:.2e}")
    print("  sigma3/sigma2 >= 1e-2:", int((ratio >= 1e-2).sum()), " closest to the threshold:", float(np.abs(ratio / 1e-2 - 1).min()))


if __name__ == "__main__":
    main()
