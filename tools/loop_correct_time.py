"""LoopCorrect's geometry on the device: ssx_loop_correct end to end, the optimiser inside it, its two new kernels, and the path a caller
had before it -- ssx_pose_graph_opt with stages 1 and 3 on the host.

    python tools/loop_correct_time.py [--keyframes 500,2000] [--points 50000,300000] [--reps 30] [--warmup 5] [--out FILE]

call       ssx_loop_correct: one upload (graph, poses, points, anchors, flags), stage 1, the LM loop, stage 3, one download.  Wall clock
           around the C call (through ctypes, pointers prepared beforehand; the poses and points are restored before every run).
optimiser  ssx_pose_graph_opt alone on the stage-1 poses with the same fixed set: what the call spends in stage 2 (wall clock; the LM
           loop synchronises per trial, so this is host-paced).
kernels    the call between ssx_profile_begin / _end: HIP-event times of k_lc_correct_keyframes + k_lc_invert_keyframes and of the two
           k_reanchor_points launches (a run of its own: the events cost wall clock).
host path  tools/loop_correct_model.py's stage 1 (numpy, vectorised over keyframes and points), ssx_pose_graph_opt, the model's stage 3.
           A C++ host loop over Sophus would be faster than numpy by a small factor; the figure is what this repository could run before.
Every figure is the median of --reps runs after --warmup runs, in milliseconds; the minimum is given beside it."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ssvio_amd  # noqa: E402
from ssvio_amd import _lib, ba, loop  # noqa: E402
from tools import loop_correct_model as lcm  # noqa: E402
from tools import synth  # noqa: E402


def make_problem(P, N, seed=5, n_active=7):
    pg = synth.make_pose_graph_problem(P=P, n_loops=3, seed=seed, meas_noise=0.01, drift=0.02, n_active=n_active)
    rng = np.random.default_rng(seed)
    gt, cur = pg["gt_poses"], P - 1
    active = np.zeros(P, np.uint8); active[P - n_active:] = 1
    D = np.array([0.005, -0.02, 0.01, 1.0, 0.8, -0.1, 1.5]); D[:4] /= np.linalg.norm(D[:4])
    poses = pg["poses"].copy()
    T_cur = synth.pose_mul(D, gt[cur])
    for a in np.nonzero(active)[0]:
        poses[a] = synth.pose_mul(synth.pose_mul(gt[a], synth.pose_inv(gt[cur])), T_cur)
    # a tenth of the points active (anchored in the window), the rest spread over all keyframes, 2 % without an anchor
    pact = (rng.random(N) < 0.1).astype(np.uint8)
    anchor = np.where(pact != 0, rng.integers(P - n_active, P, N), rng.integers(0, P, N)).astype(np.int32)
    pc = np.stack([rng.uniform(-10, 10, N), rng.uniform(-2, 2, N), rng.uniform(3, 40, N)], 1)
    pts = lcm.se3_act(lcm.se3_inverse(poses)[anchor], pc)
    anchor[rng.random(N) < 0.02] = -1
    return dict(P=P, E=pg["E"], N=N, poses=poses, kf_active=active, cur_kf=cur, loop_kf=int(pg["ej"][P - 1]), initial_kf=0, keep_kf=cur,
                corrected_pose=gt[cur].copy(), ei=pg["ei"], ej=pg["ej"], meas=pg["meas"], points=np.ascontiguousarray(pts), point_anchor=anchor,
                point_active=pact)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3


def row(ctx, P, N, reps, warmup):
    lib = ctx.lib
    pr = make_problem(P, N)
    prob, a = loop.loop_correct_struct(pr, 20)
    res = loop.LoopCorrectResult()
    lib.ssx_loop_correct.restype = C.c_int
    lib.ssx_loop_correct.argtypes = [C.c_void_p, C.POINTER(loop.LoopCorrectProblem), C.c_int32, C.POINTER(loop.LoopCorrectResult)]
    poses0, points0 = a["poses"].copy(), a["points"].copy()

    def call():
        a["poses"][:] = poses0; a["points"][:] = points0
        if lib.ssx_loop_correct(ctx.handle, C.byref(prob), 20, C.byref(res)) != 0:
            raise RuntimeError(lib.ssx_last_error(ctx.handle).decode())
    out = dict(P=P, N=N, call=timed(call, reps, warmup), iters=res.pg.n_iters)
    dev_points = a["points"].copy()
    flat = dict(poses=a["stage1_poses"].copy(), fixed=lcm.fixed_set(pr), ei=pr["ei"], ej=pr["ej"], meas=pr["meas"])
    out["optimiser"] = timed(lambda: ba.pose_graph_opt(ctx, flat), reps, warmup)
    host = {}

    def host_path():
        host["r"] = lcm.loop_correct(pr, lambda f, iters: ba.pose_graph_opt(ctx, f, iters))
    out["host"] = timed(host_path, reps, warmup)
    # (the host path's stage-1 poses differ from the device's by FMA rounding, and 20 LM iterations on numeric Jacobians carry that on)
    out["diff"] = float(np.abs(host["r"]["points"] - dev_points).max())
    kt = {}
    for _ in range(warmup + reps):
        _lib.profile_begin(ctx)
        call()
        for name, (_, ms) in _lib.profile_end(ctx).items():
            kt.setdefault(name, []).append(ms)
    out["kernels"] = {k: (float(np.median(v[warmup:])), float(np.min(v[warmup:]))) for k, v in kt.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="500,2000")
    ap.add_argument("--points", default="50000,300000")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loop_correct", "time.txt"))
    a = ap.parse_args()
    ctx = ssvio_amd.Context(0)
    lines = [f"ssx_loop_correct, 20 LM iterations, 7 active keyframes, 3 loop edges; milliseconds, median (minimum) of {a.reps} after {a.warmup}",
             f"{'keyframes':>9} {'points':>7} {'LM its':>6} {'whole call':>18} {'of it optimiser':>18} {'keyframe kernels':>18} {'k_reanchor_points':>18} "
             f"{'host path':>18}  max |points - host path|"]
    f = lambda v: f"{v[0]:9.3f} ({v[1]:7.3f})"
    for P in [int(s) for s in a.keyframes.split(",")]:
        for N in [int(s) for s in a.points.split(",")]:
            r = row(ctx, P, N, a.reps, a.warmup)
            k = r["kernels"]
            lines.append(f"{P:>9} {N:>7} {r['iters']:>6} {f(r['call']):>18} {f(r['optimiser']):>18} {f(k.get('k_lc_keyframes', (0, 0))):>18} "
                         f"{f(k.get('k_reanchor_points', (0, 0))):>18} {f(r['host']):>18}  {r['diff']:.2e}")
            print(lines[-1], flush=True)
    ctx.close()
    lines.append("(last column: the host path starts the optimiser from the model's stage-1 poses, the call from the device's; they differ by FMA rounding, and 20")
    lines.append(" LM iterations on numeric Jacobians (delta = 1e-9), which do not finish a chain this long, carry that on -- tests/test_pg_gpu.py states the effect)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
