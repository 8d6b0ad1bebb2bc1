"""A loop correction of the backend's resident window: ssx_ba_window_loop_correct against the route a caller had before it.

    python tools/window_loop_correct_time.py [--reps 30] [--warmup 5] [--out FILE]

One window of BASELINE's size (12 keyframes, 5 600 landmarks, 20 000 observations), pushed keyframe by keyframe and solved once.

call          ssx_ba_window_loop_correct (no fused landmarks, poses / points / anchors returned): wall clock around the C call through
              ctypes, pointers prepared beforehand.  The corrected pose alternates between two poses, so the window moves every time.
kernels       the call between ssx_profile_begin / _end: HIP-event times of the anchor kernels (k_win_anchor_rank + k_win_anchor_slot),
              k_lc_correct_keyframes and k_reanchor_points (a run of its own: the events cost wall clock).
solve after   ssx_ba_window_solve right after the call (untimed call, timed solve): nothing is pending, the solve uploads its tables only.
before        the route of existing calls: ssx_ba_window_export, ssx_loop_correct on the export (iterations = 0: stage 1 alone; the C call,
              its problem struct prepared outside the clock), then
              ssx_ba_window_set_pose x 12 and ssx_ba_window_set_landmark x 5 600, then the next ssx_ba_window_solve, which sends every
              slot again.  The 5 612 setter calls go through ctypes here; the cost of 5 612 empty ctypes calls (ssx_version) is
              given beside them, a C++ caller pays the difference.
plain solve   ssx_ba_window_solve with no edit before it, for scale.
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
from ssvio_amd._lib import dbl_p, ptr  # noqa: E402
from tools import synth  # noqa: E402

i64_p = C.POINTER(C.c_int64)


def make_window(ctx, P=12, L=5600, E=20000, seed=2):
    pr = synth.make_ba_problem(P=P, L=L, obs_per_lm=4, seed=seed)
    keep = np.ones(pr["E"], bool)
    keep[4 * np.arange(pr["E"] - E) + 3] = False                # the fourth observation of the first landmarks: E observations remain
    for k in ("edge_pose", "edge_point", "edge_uv", "edge_cam"):
        pr[k] = pr[k][keep]
    first = np.full(L, 10 ** 9, dtype=np.int64)
    np.minimum.at(first, pr["edge_point"], pr["edge_pose"])
    win = ba.BaWindow(ctx, pr["K"], pr["cam_ext"], fix_rule=1)
    for k in range(P):
        new = np.nonzero(first == k)[0]
        e = np.nonzero(pr["edge_pose"] == k)[0]
        win.push(k, pr["poses"][k], new_ids=new, new_xyz=pr["points"][new], new_fixed=pr["point_fixed"][new], obs_lm=pr["edge_point"][e],
                 obs_uv=pr["edge_uv"][e], obs_cam=pr["edge_cam"][e])
    win.solve()
    return win


def timed(fn, reps, warmup, before=None):
    t = []
    for i in range(warmup + reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3, float(np.min(t)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "window_loop_correct", "time.txt"))
    a = ap.parse_args()
    ctx = ssvio_amd.Context(0)
    lib = ctx.lib
    win = make_window(ctx)
    P, L, E = win.size()
    cur = P - 1
    ex = win.export()
    d = np.concatenate([synth.small_rot_quat(np.array([0.01, -0.04, 0.02])), [0.8, -0.1, 1.5]]); d[:4] /= np.linalg.norm(d[:4])
    targets = [np.ascontiguousarray(synth.pose_mul(d, ex["poses"][cur])), np.ascontiguousarray(ex["poses"][cur].copy())]
    turn = [0]

    # ---- the new call ----
    lib.ssx_ba_window_loop_correct.restype = C.c_int32
    lib.ssx_ba_window_loop_correct.argtypes = [C.c_void_p, C.c_int64, dbl_p, C.c_int32, i64_p, C.POINTER(ba.BaWindowLoopResult)]
    o_poses, o_points, o_anchor = np.zeros((P, 7)), np.zeros((L, 3)), np.zeros(L, np.int64)
    res = ba.BaWindowLoopResult()
    res.poses_out = ptr(o_poses, dbl_p); res.points_out = ptr(o_points, dbl_p); res.anchor_kf_out = ptr(o_anchor, i64_p)
    tp = [ptr(t, dbl_p) for t in targets]

    def call():
        turn[0] ^= 1
        if lib.ssx_ba_window_loop_correct(win.handle, cur, tp[turn[0]], 0, None, C.byref(res)) != 0:
            raise RuntimeError(lib.ssx_last_error(ctx.handle).decode())
    t_call = timed(call, a.reps, a.warmup)
    kt = {}
    for _ in range(a.warmup + a.reps):
        _lib.profile_begin(ctx)
        call()
        for name, (_, ms) in _lib.profile_end(ctx).items():
            kt.setdefault(name, []).append(ms)
    kern = {k: (float(np.median(v[a.warmup:])), float(np.min(v[a.warmup:]))) for k, v in kt.items()}

    # ---- a solve ----
    sres, sbufs = win._result_buffers(True)

    def solve():
        if lib.ssx_ba_window_solve(win.handle, C.byref(sres)) != 0:
            raise RuntimeError(lib.ssx_last_error(ctx.handle).decode())
    t_plain = timed(solve, a.reps, a.warmup)
    t_solve_after = timed(solve, a.reps, a.warmup, before=call)

    # ---- the route before: export, stage 1 through ssx_loop_correct, 5 612 setters, the sync inside the next solve ----
    lib.ssx_loop_correct.restype = C.c_int
    lib.ssx_loop_correct.argtypes = [C.c_void_p, C.POINTER(loop.LoopCorrectProblem), C.c_int32, C.POINTER(loop.LoopCorrectResult)]
    state = {}

    def export():
        state["ex"] = win.export()

    def marshal():
        # export -> the flat problem of ssx_loop_correct (anchor = the first exported edge of each landmark) and the setters' pointers: not timed,
        # a C++ caller does this with a few loops over arrays it already holds
        e = state["ex"]
        anc = np.full(L, -1, np.int32)
        anc[e["edge_point"][::-1]] = e["edge_pose"][::-1]
        turn[0] ^= 1
        pr = dict(poses=e["poses"], kf_active=np.ones(P, np.uint8), cur_kf=cur, loop_kf=0, initial_kf=-1, keep_kf=-1, corrected_pose=targets[turn[0]],
                  ei=np.zeros(0, np.int32), ej=np.zeros(0, np.int32), meas=np.zeros((0, 7)), points=e["points"], point_anchor=anc, point_active=np.ones(L, np.uint8))
        state["prob"], arr = loop.loop_correct_struct(pr, 0)
        state["arr"] = arr
        state["pp"] = [C.cast(arr["poses"].ctypes.data + 56 * i, dbl_p) for i in range(P)]
        state["lp"] = [C.cast(arr["points"].ctypes.data + 24 * i, dbl_p) for i in range(L)]
    lc_res = loop.LoopCorrectResult()

    def stage1():
        if lib.ssx_loop_correct(ctx.handle, C.byref(state["prob"]), 0, C.byref(lc_res)) != 0:
            raise RuntimeError(lib.ssx_last_error(ctx.handle).decode())
    kf_ids, lm_ids = [int(k) for k in ex["kf_ids"]], [int(l) for l in ex["lm_ids"]]
    set_pose, set_lm, h = lib.ssx_ba_window_set_pose, lib.ssx_ba_window_set_landmark, win.handle

    def setters():
        for k, p in zip(kf_ids, state["pp"]):
            set_pose(h, k, p, -1)
        for l, p in zip(lm_ids, state["lp"]):
            set_lm(h, l, p, -1)
    version = lib.ssx_version

    def empty_calls():
        for _ in range(P + L):
            version()

    def prepare_stage1():
        export(); marshal()

    def prepare_setters():
        export(); marshal(); stage1()
    t_export = timed(export, a.reps, a.warmup)
    t_stage1 = timed(stage1, a.reps, a.warmup, before=prepare_stage1)
    t_set = timed(setters, a.reps, a.warmup, before=prepare_setters)
    t_empty = timed(empty_calls, a.reps, a.warmup)

    def route_until_solve():
        prepare_setters(); setters()
    t_solve_before = timed(solve, a.reps, a.warmup, before=route_until_solve)
    win.close()
    ctx.close()
    f = lambda v: f"{v[0]:9.3f} ({v[1]:7.3f})"     # noqa: E731
    anchor = kern.get("k_win_anchor", (0.0, 0.0))
    new_total = t_call[0] + t_solve_after[0]
    old_total = t_export[0] + t_stage1[0] + t_set[0] + t_solve_before[0]
    lines = [f"ssx_ba_window_loop_correct on a window of {P} keyframes, {L} landmarks, {E} observations; milliseconds, median (minimum) of {a.reps} after {a.warmup}",
             f"{'the call':<58} {f(t_call)}",
             f"{'  its kernels: k_win_anchor_rank + k_win_anchor_slot':<58} {f(anchor)}",
             f"{'               k_lc_correct_keyframes':<58} {f(kern.get('k_lc_keyframes', (0.0, 0.0)))}",
             f"{'               k_reanchor_points':<58} {f(kern.get('k_reanchor_points', (0.0, 0.0)))}",
             f"{'the first solve after the call':<58} {f(t_solve_after)}",
             f"{'a solve with no edit before it':<58} {f(t_plain)}",
             "the route before (existing calls only):",
             f"{'  ssx_ba_window_export':<58} {f(t_export)}",
             f"{'  ssx_loop_correct, iterations = 0 (the C call)':<58} {f(t_stage1)}",
             f"{'  set_pose x ' + str(P) + ', set_landmark x ' + str(L) + ' (through ctypes)':<58} {f(t_set)}",
             f"{'    of it: ' + str(P + L) + ' empty ctypes calls':<58} {f(t_empty)}",
             f"{'  the first solve after them (sends every slot again)':<58} {f(t_solve_before)}",
             f"call + first solve: {new_total:.3f} ms; the route before + first solve: {old_total:.3f} ms ({old_total - t_empty[0]:.3f} ms without the empty-call share)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
