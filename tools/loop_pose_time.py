"""ComputeCorrectPose on the device: ssx_loop_compute_pose end to end, its two kernels, and the same work with the RANSAC's pose
fetched to the host in between.

    python tools/loop_pose_time.py [--sizes 50,300,2000] [--iters 100] [--reps 30] [--warmup 5] [--out FILE]

fused    ssx_loop_compute_pose: the pairs up, k_pnp_ransac, k_pose_only* from the pose where the first kernel left it, the results
         down, ONE synchronisation.  Wall clock around the C call (through ctypes, pointers prepared beforehand).
kernels  the same call between ssx_profile_begin / _end: HIP-event times of the two kernels (a run of its own: the events cost wall
         clock).
chained  ssx_pnp_ransac, then ssx_loop_pose_opt from the pose it returned: two uploads of the pairs, two synchronisations.
Every figure is the median of --reps runs after --warmup runs; the minimum is given beside it.  There is no OpenCV on the machines
this runs on, hence no cv::solvePnPRansac figure to set beside these."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ssvio_amd  # noqa: E402
from ssvio_amd import _lib, loop  # noqa: E402
from ssvio_amd._lib import dbl_p, ptr, u8_p  # noqa: E402
from tools.synth import make_loop_pose_problem  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6, float(np.min(t)) * 1e6


def row(ctx, M, H, reps, warmup):
    lib = ctx.lib
    loop._bind_pose(lib)
    p = make_loop_pose_problem(M=M, seed=M, frac_gross=0.3, noise_px=0.5)
    K, xyz, uv = p["K"], p["xyz"], p["uv"]
    has, kept = np.ones(M, np.uint8), np.zeros(M, np.uint8)
    ident = np.array([0, 0, 0, 1.0, 0, 0, 0])
    res = loop.LoopPoseResult()
    a_fused = (ctx.handle, M, ptr(xyz, dbl_p), ptr(has, u8_p), ptr(uv, dbl_p), ptr(ident, dbl_p), ptr(ident, dbl_p), ptr(K, dbl_p), H, 1, ptr(kept, u8_p),
               C.byref(res))

    def fused():
        if lib.ssx_loop_compute_pose(*a_fused) != 0:
            raise RuntimeError(lib.ssx_last_error(ctx.handle).decode())
    pose, inl = np.zeros(7), np.zeros(M, np.uint8)
    n, best, found = C.c_int32(), C.c_int32(), C.c_int32()
    a_r = (ctx.handle, ptr(K, dbl_p), M, ptr(xyz, dbl_p), ptr(uv, dbl_p), H, 5.991, 1, ptr(pose, dbl_p), None, C.byref(n), C.byref(best), C.byref(found))
    a_o = (ctx.handle, ptr(pose, dbl_p), ptr(K, dbl_p), M, ptr(xyz, dbl_p), ptr(uv, dbl_p), 5.991, 1.0, ptr(inl, u8_p), C.byref(n))

    def chained():
        if lib.ssx_pnp_ransac(*a_r) != 0 or not found.value or lib.ssx_loop_pose_opt(*a_o) != 0:
            raise RuntimeError("chained call failed")
    out = dict(M=M, fused=timed(fused, reps, warmup), chained=timed(chained, reps, warmup))
    assert res.verdict == loop.LOOP_OK and res.n_inliers == n.value and bytes(res.corrected_pose) == pose.tobytes()
    kt = {"k_pnp_ransac": [], "k_pose_only": []}
    for _ in range(warmup + reps):
        _lib.profile_begin(ctx)
        fused()
        for name, (_, ms) in _lib.profile_end(ctx).items():
            kt.setdefault(name, []).append(ms * 1e3)
    out["kernels"] = {k: (float(np.median(v[warmup:])), float(np.min(v[warmup:]))) for k, v in kt.items()}
    out["inliers"] = (res.n_ransac_inliers, res.n_inliers)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="50,300,2000")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = ssvio_amd.Context(0)
    lines = [f"ssx_loop_compute_pose, {a.iters} hypotheses, 30 % wrong matches, 0.5 px noise; microseconds, median (minimum) of {a.reps} after {a.warmup}",
             f"{'pairs':>6} {'fused call':>16} {'k_pnp_ransac':>16} {'k_pose_only':>16} {'chained calls':>16}  inliers RANSAC/refined"]
    for M in [int(s) for s in a.sizes.split(",")]:
        r = row(ctx, M, a.iters, a.reps, a.warmup)
        f = lambda v: f"{v[0]:8.1f} ({v[1]:5.1f})"
        lines.append(f"{M:>6} {f(r['fused']):>16} {f(r['kernels']['k_pnp_ransac']):>16} {f(r['kernels']['k_pose_only']):>16} {f(r['chained']):>16}  "
                     f"{r['inliers'][0]}/{r['inliers'][1]}")
    ctx.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
