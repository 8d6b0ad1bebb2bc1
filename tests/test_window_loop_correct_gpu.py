"""GPU: ssx_ba_window_loop_correct -- LoopClosing::CorrectActivateKeyframeAndMappoint (reference: src/ssvio/loopclosing.cpp:378-453)
applied to a resident ssx_ba_window where it lies.

1. bit for bit the shipped stage 1: ssx_loop_correct on the exported window (every keyframe and point active, anchor = the first exported
   edge of each landmark, iterations = 0) returns the bits the window call returns and the window then exports
2. against tests/golden/loop_correct_hp.npz (60 digits), with the bar of tests/test_loop_correct_gpu.py
3. both state buffers and the host mirror hold the corrected state: two solves, a twin brought there with set_pose / set_landmark, a batch
4. the fusion is a removal: the call with fused ids == the call without + ssx_ba_window_remove_landmarks
5. a drive of tools.mapmodel through a loop closure: the window equals the re-marshalled map at every keyframe
6. misuse is refused on the host and leaves window, mirror and result untouched"""
import ctypes as C
import os

import numpy as np
import pytest

import loop_correct_cases as lcc
import window_loop_cases as wlc
from ssvio_amd import ba, loop
from ssvio_amd._lib import dbl_p, ptr
from window_loop_cases import WindowSpec

pytestmark = pytest.mark.gpu
HP = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_correct_hp.npz"))
FACTOR = float(HP["factor"])
i64_p = C.POINTER(C.c_int64)

# keyframes 1, 2, 7 x landmarks 0, 1, 63, 64, 65, 255, 257 (the tails of a 64-wide wave and of a 256-thread workgroup); every window's
# keyframe and landmark ids arrive in no order, a sixth of the landmarks is seen by right cameras only, and the last push is unsynced
SPECS = {
    "1kf_0lm": WindowSpec(1, 0, seed=1),
    "1kf_1lm": WindowSpec(1, 1, seed=2),
    "1kf_257lm_after_pops": WindowSpec(1, 257, seed=3, n_extra=3, solve_at=2),                      # the current keyframe alone; fixed by rule 1
    "2kf_63lm": WindowSpec(2, 63, seed=4),
    "2kf_64lm": WindowSpec(2, 64, seed=5, n_extra=1, remove_first_obs=True),
    "7kf_65lm_dead_slots": WindowSpec(7, 65, seed=6, n_extra=3, n_remove_lm=9, remove_first_obs=True, solve_at=6, fix_first_pose=True),
    "7kf_255lm_reused_slots": WindowSpec(7, 255, seed=7, n_extra=2, n_remove_lm=20, remove_first_obs=True, solve_at=5, pops_before_last_push=True),
    "7kf_257lm_rewritten": WindowSpec(7, 257, seed=8, n_extra=9, n_remove_lm=5, remove_first_obs=True, solve_at=6, dense=True),
}
MAIN = "7kf_65lm_dead_slots"


def first_edge_anchors(ex):
    """the keyframe row of the first exported edge of each landmark (export lists the observations in push order), -1: none"""
    anc = np.full(ex["L"], -1, np.int32)
    for e in range(ex["E"] - 1, -1, -1):
        anc[ex["edge_point"][e]] = ex["edge_pose"][e]
    return anc


def stage1_of_export(ctx, ex, cur_row, corrected):
    pr = dict(poses=ex["poses"], kf_active=np.ones(ex["P"], np.uint8), cur_kf=cur_row, loop_kf=0, initial_kf=-1, keep_kf=-1, corrected_pose=corrected,
              ei=np.zeros(0, np.int32), ej=np.zeros(0, np.int32), meas=np.zeros((0, 7)), points=ex["points"], point_anchor=first_edge_anchors(ex),
              point_active=np.ones(ex["L"], np.uint8))
    return pr, loop.loop_correct(ctx, pr, iters=0)


def same_export(a, b, but=()):
    for k in a:
        if k not in but:
            assert np.array_equal(a[k], b[k]), k


def same_solve(a, b):
    for k in ("poses", "points", "edge_chi2", "edge_outlier", "chi2", "lam", "trials"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["rounds"] == b["rounds"] and a["n_iters"] == b["n_iters"]


def solve_like_fresh(ctx, win):
    """one solve of the window, held to ssx_ba_solve of the problem exported just before it"""
    ex = win.export()
    fresh = ba.ba_solve(ctx, ex)
    got = win.solve()
    for k in ("poses", "points", "edge_chi2", "chi2", "trials"):
        assert np.array_equal(got[k], fresh[k]), k
    return got


@pytest.mark.parametrize("name", list(SPECS))
def test_bit_for_bit_the_shipped_stage1(ctx, name):
    spec = SPECS[name]
    win, info = wlc.build_window(ctx, spec)
    try:
        n_rw = wlc.rewrites(win)
        assert (n_rw > 0) == (name == "7kf_257lm_rewritten"), n_rw               # dead entries before a rewrite / after one
        ex = win.export()
        assert (ex["P"], ex["L"]) == (spec.n_kf, spec.n_lm)
        cur_row = list(ex["kf_ids"]).index(info["cur_kf_id"])
        corrected = wlc.corrected_pose(ex["poses"][cur_row], **wlc.FAR)
        pr, want = stage1_of_export(ctx, ex, cur_row, corrected)
        anc = pr["point_anchor"]
        r = win.loop_correct(info["cur_kf_id"], corrected)
        assert np.array_equal(r["poses"], want["poses"]) and np.array_equal(r["points"], want["points"])
        assert np.array_equal(r["poses"][cur_row], corrected)
        assert np.array_equal(r["anchors"], np.where(anc >= 0, ex["kf_ids"][np.maximum(anc, 0)], -1) if ex["L"] else np.zeros(0, np.int64))
        assert r["n_points_moved"] == int((anc >= 0).sum()) == want["n_active_points_moved"] and r["n_fused_removed"] == 0
        after = win.export()
        assert np.array_equal(after["poses"], want["poses"]) and np.array_equal(after["points"], want["points"])
        same_export(ex, after, but=("poses", "points"))                          # ids, fixed flags and observations are untouched
        if spec.n_lm:
            assert not np.array_equal(after["points"], ex["points"])
        # what the window was built to hold
        if spec.n_kf > 1 and spec.n_lm > 10:
            seq = {k: i for i, k in enumerate(info["kf_ids"])}                   # push order of the keyframes
            obs = [[] for _ in range(ex["L"])]
            for p, l in zip(ex["edge_pose"], ex["edge_point"]):
                obs[l].append(int(ex["kf_ids"][p]))
            assert all(o and seq[int(a)] == min(seq[k] for k in o) for o, a in zip(obs, r["anchors"]))
            assert any(int(a) != min(o) for o, a in zip(obs, r["anchors"]))      # ... which is not the order of the ids
            cams = [set() for _ in range(ex["L"])]
            for l, c in zip(ex["edge_point"], ex["edge_cam"]):
                cams[l].add(int(c))
            assert any(c == {1} for c in cams)                                   # seen by right cameras only
        if spec.n_extra and spec.n_lm > 10:
            assert ex["point_fixed"].sum() > (np.arange(spec.n_lm) % 7 == 3).sum()   # fixed by rule 1, beyond the caller's flags
    finally:
        win.close()


@pytest.mark.parametrize("name", ["lc12", "only_cur", "all_fixed", "far", "half_turn", "no_change", "lc12_n1"])
def test_against_60_digits(ctx, name):
    """the active part of a case of tests/loop_correct_cases.py as a window: the active keyframes, the active points with an active
    anchor, one synthetic observation per point at its anchor.  Bar: tests/test_loop_correct_gpu.py's."""
    pr = lcc.make(name)
    act = pr["kf_active"] != 0
    sel = (pr["point_active"] != 0) & (pr["point_anchor"] >= 0) & act[np.maximum(pr["point_anchor"], 0)]
    from tools import synth
    with ba.BaWindow(ctx, synth.KITTI_K, synth.stereo_cam_ext(), fix_rule=1) as win:
        for k in np.nonzero(act)[0]:                                             # ids = the case's indices; the current keyframe comes last
            new = np.nonzero(sel & (pr["point_anchor"] == k))[0]
            win.push(int(k), pr["poses"][k], new_ids=new, new_xyz=pr["points"][new], obs_lm=new, obs_uv=np.stack([100.0 + new, 50.0 + 0 * new], 1))
        r = win.loop_correct(pr["cur_kf"], pr["corrected_pose"])
        after = win.export()
    assert list(r["kf_ids"]) == list(np.nonzero(act)[0]) and list(r["lm_ids"]) == list(np.nonzero(sel)[0])
    assert np.array_equal(r["anchors"], pr["point_anchor"][sel]) and r["n_points_moved"] == int(sel.sum())
    k = lcc.NAMES.index(name)

    def bar(quantity, truth):
        largest = float(np.abs(truth).max()) if np.size(truth) else 1.0
        return max(FACTOR * float(HP[f"model_{quantity}"][k]), FACTOR * float(np.spacing(largest)))

    t_poses, t_pts = HP[f"{name}_s1_poses"], HP[f"{name}_s1_points"]
    got = [("s1_poses", lcc.pose_distance(r["poses"], t_poses[act]), bar("s1_poses", t_poses)),
           ("s1_points", lcc.point_distance(r["points"], t_pts[sel]), bar("s1_points", t_pts))]
    print(name, "  ".join(f"{q} {d:.2e} (bar {b:.2e})" for q, d, b in got))
    for q, d, b in got:
        assert d <= b, (name, q, d, b)
    assert np.array_equal(after["poses"], r["poses"]) and np.array_equal(after["points"], r["points"])


def test_both_buffers_and_the_mirror_hold_the_corrected_state(ctx):
    spec = SPECS[MAIN]
    a, info = wlc.build_window(ctx, spec)
    b, _ = wlc.build_window(ctx, spec)
    c, _ = wlc.build_window(ctx, spec)
    d, d_info = wlc.build_window(ctx, SPECS["7kf_255lm_reused_slots"])
    d1, _ = wlc.build_window(ctx, SPECS["7kf_255lm_reused_slots"])
    try:
        ex = a.export()
        assert ex["pose_fixed"].sum() == 1 and 0 < ex["point_fixed"].sum() < ex["L"]       # fixed vertices live in BOTH buffers
        corrected = wlc.corrected_pose(ex["poses"][list(ex["kf_ids"]).index(info["cur_kf_id"])])
        fused = info["lm_ids"][::9]
        r = a.loop_correct(info["cur_kf_id"], corrected, fused)
        # today's route to the same state
        for k, p in zip(r["kf_ids"], r["poses"]):
            b.set_pose(int(k), p)
        for l, x in zip(r["lm_ids"], r["points"]):
            b.set_landmark(int(l), x)
        assert b.remove_landmarks(fused) == len(fused) == r["n_fused_removed"]
        same_export(a.export(), b.export())
        for _ in range(2):                                                       # the second solve starts from the other buffer
            ga = solve_like_fresh(ctx, a)
            gb = b.solve()
            same_solve(ga, gb)
        # corrected, then solved inside a batch beside an untouched window: per window the bits of the single solve
        c.loop_correct(info["cur_kf_id"], corrected, fused)
        batch = ba.BaWindow.solve_batch([c, d])
        a2, _ = wlc.build_window(ctx, spec)
        try:
            a2.loop_correct(info["cur_kf_id"], corrected, fused)
            same_solve(batch[0], a2.solve())
        finally:
            a2.close()
        same_solve(batch[1], d1.solve())
    finally:
        for w in (a, b, c, d, d1):
            w.close()


def test_fusion_is_the_correction_followed_by_a_removal(ctx):
    spec = SPECS[MAIN]
    a, info = wlc.build_window(ctx, spec)
    b, _ = wlc.build_window(ctx, spec)
    try:
        ex = a.export()
        cur_row = list(ex["kf_ids"]).index(info["cur_kf_id"])
        corrected = wlc.corrected_pose(ex["poses"][cur_row])
        # every landmark of one keyframe (not the current one), some more, ids the window does not hold, one id twice
        victim = [r for r in range(ex["P"]) if r != cur_row][1]
        of_victim = np.unique(ex["lm_ids"][ex["edge_point"][ex["edge_pose"] == victim]])
        fused = np.concatenate([of_victim, ex["lm_ids"][::11], info["removed_lm_ids"][:2], [10 ** 12, -5], of_victim[:1]])
        held = np.unique(fused[np.isin(fused, ex["lm_ids"])])
        ra = a.loop_correct(info["cur_kf_id"], corrected, fused)
        rb = b.loop_correct(info["cur_kf_id"], corrected)
        assert rb["n_fused_removed"] == 0 and b.remove_landmarks(fused) == len(held) == ra["n_fused_removed"]
        for k in ("poses", "points", "anchors", "kf_ids", "lm_ids"):
            assert np.array_equal(ra[k], rb[k]), k                               # points_out: before the fused ones leave
        assert a.size() == b.size() and a.size()[1] == ex["L"] - len(held)
        exa, exb = a.export(), b.export()
        same_export(exa, exb)
        assert not np.isin(exa["lm_ids"], held).any() and not (exa["edge_pose"] == victim).any()   # a keyframe without observations
        outcome = []
        for w in (a, b):
            try:
                outcome.append(w.solve())
            except Exception as e:                                               # noqa: BLE001 -- the existing call's behaviour, whatever it is
                outcome.append(type(e))
        if isinstance(outcome[0], dict):
            same_solve(outcome[0], outcome[1])
        else:
            assert outcome[0] is outcome[1]
    finally:
        a.close(); b.close()


def test_driven_like_the_reference_through_a_loop_closure(ctx):
    """tools.mapmodel drives a window (fix rule 1) through 14 keyframes; at the tenth the loop closes on the first keyframe: 18 pairs
    fuse a current map point into a loop map point, the rest give a current feature without a map point the loop map point (the `else`
    of :449-452).  The keyframes after it track the current keyframe's features, so they observe the loop map points: those come back
    as fixed landmarks.  After every keyframe the window's solve is, bit for bit, ssx_ba_solve of the re-marshalled map.  (A pair
    whose current feature keeps a map point the loop side lacks is left to the CPU test: there the reference leaves a map point
    observing a feature that no longer points back, and dereferences null when that edge is culled, backend.cpp:212-213.)"""
    from tools import synth
    from tools.mapmodel import ActiveMap, apply_edits, make_window_scenario
    n_active, at, loop_kf = 5, 9, 100
    frames = make_window_scenario(n_kf=14, n_active=n_active, new_per_kf=60, seed=3)
    m = ActiveMap(n_active)
    win = ba.BaWindow(ctx, m.K, m.cam_ext, fix_rule=1)
    K = m.K
    carried, reentered, n_else = [], set(), 0
    try:
        for r, fr in enumerate(frames):
            for l in fr["condemn"]:
                m.condemn(l)
            obs = list(fr["obs"])
            for l in carried:                                                    # the loop points, tracked from the current keyframe on
                mp = m.mps.get(l)
                if mp is None:
                    continue
                pc = synth.quat_rot(fr["pose"][:4], mp.pos) + fr["pose"][4:]
                if pc[2] > 1.0:
                    obs.append((l, (K[0] * pc[0] / pc[2] + K[2] + 0.3, K[1] * pc[1] / pc[2] + K[3] - 0.2)))
            m.insert_keyframe(fr["kf_id"], fr["pose"], obs, fr["new_points"], fr["victim"])
            edits = m.take_edits()
            if r > at:
                push = [a for k, a in edits if k == "push"][0]
                back = [int(l) for l in push["new_ids"] if int(l) in carried]
                assert all(push["new_fixed"][list(push["new_ids"]).index(l)] == 1 for l in back)
                reentered.update(back)
            assert apply_edits(win, edits) == []
            pr, kf_ids, lm_ids, e_feat = m.problem()
            ex = win.export()
            assert list(ex["kf_ids"]) == kf_ids and list(ex["lm_ids"]) == lm_ids, r
            assert np.array_equal(ex["point_fixed"], pr["point_fixed"]) and np.array_equal(ex["poses"], pr["poses"]) and np.array_equal(ex["points"], pr["points"]), r
            key_w = ex["edge_pose"].astype(np.int64) * 10 ** 7 + ex["edge_point"]
            key_m = pr["edge_pose"].astype(np.int64) * 10 ** 7 + pr["edge_point"]
            assert len(np.unique(key_w)) == len(key_w) and np.array_equal(np.sort(key_w), np.sort(key_m)), r
            to_w = np.argsort(key_w)[np.argsort(np.argsort(key_m))]              # map edge -> window edge
            assert np.array_equal(ex["edge_uv"][to_w], pr["edge_uv"])
            fresh = ba.ba_solve(ctx, pr)
            got = win.solve()
            assert np.array_equal(got["poses"], fresh["poses"]) and np.array_equal(got["points"], fresh["points"]), r
            assert np.array_equal(got["edge_chi2"][to_w], fresh["edge_chi2"]) and np.array_equal(got["trials"], fresh["trials"]), r
            assert np.array_equal(got["chi2"], fresh["chi2"]), r
            m.apply(kf_ids, lm_ids, e_feat, fresh["poses"], fresh["points"], fresh["edge_outlier"])
            if r != at:
                continue
            # ---- the loop closes ----
            cur = m.kfs[fr["kf_id"]]["feats"]
            n_else = min(8, sum(1 for f in cur if m._lock(f) is None))
            assert n_else >= 2
            pairs = wlc.pick_matches(m, fr["kf_id"], loop_kf, 18, n_else, 0)
            assert 20 <= len(pairs) <= 40
            carried = [m.kfs[loop_kf]["feats"][li].lm for _, li in pairs]
            mr = m.loop_correct(fr["kf_id"], wlc.corrected_pose(m.kfs[fr["kf_id"]]["pose"]), pairs, loop_kf)
            assert len(mr["fused"]) == 18
            before = win.export()
            (wr,) = apply_edits(win, m.take_edits())                             # the culled edges of this solve, then the correction
            assert wr["n_fused_removed"] == 18 and win.size()[1] == len(wr["lm_ids"]) - 18 <= before["L"] - 18
            # the window and the model agree on what moved and where to.  The device contracts to FMA, numpy does not: each of the ~40
            # operations of a chain rounds differently by at most an ulp of its operands, which stay below 256 (m): 40 x 5.7e-14 < 1e-11
            rows = np.isin(mr["lm_ids"], wr["lm_ids"])
            assert list(wr["kf_ids"]) == mr["kf_ids"] and list(wr["lm_ids"]) == list(np.array(mr["lm_ids"])[rows])
            assert list(wr["anchors"]) == list(np.array(mr["anchors"])[rows])
            assert np.abs(wr["poses"] - mr["poses"]).max() < 1e-11 and np.abs(wr["points"] - mr["points"][rows]).max() < 1e-11
            m.adopt(wr["kf_ids"], wr["poses"], wr["lm_ids"], wr["points"])       # the map takes the device's bits
        assert len(frames) - 1 - at >= 4 and len(reentered) >= 10 and m.stats["fixed_by_rule"] > 100, (len(reentered), m.stats)
    finally:
        win.close()


def _raw(ctx, handle, cur, pose, n, ids, res):
    f = ctx.lib.ssx_ba_window_loop_correct
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int64, dbl_p, C.c_int32, i64_p, C.POINTER(ba.BaWindowLoopResult)]
    return f(handle, cur, None if pose is None else ptr(pose, dbl_p), n, None if ids is None else ptr(ids, i64_p), None if res is None else C.byref(res))


def test_misuse_is_refused_on_the_host_and_changes_nothing(ctx):
    spec = SPECS["2kf_64lm"]
    a, info = wlc.build_window(ctx, spec)
    twin, _ = wlc.build_window(ctx, spec)
    empty = ba.BaWindow(ctx, a.K, a.cam_ext, fix_rule=1)
    try:
        ex = a.export()
        cur = info["cur_kf_id"]
        good = wlc.corrected_pose(ex["poses"][list(ex["kf_ids"]).index(cur)])
        ids = np.ascontiguousarray(ex["lm_ids"][:3])
        nan, inf, zero_q = good.copy(), good.copy(), good.copy()
        nan[5] = np.nan; inf[1] = np.inf; zero_q[:4] = 0.0
        guard = -7.25
        poses, points, anchors = np.full((ex["P"], 7), guard), np.full((ex["L"], 3), guard), np.full(ex["L"], -77, np.int64)

        def result():
            res = ba.BaWindowLoopResult(-3, -3, -3, -3)
            res.poses_out = ptr(poses, dbl_p); res.points_out = ptr(points, dbl_p); res.anchor_kf_out = ptr(anchors, i64_p)
            return res

        popped = ba.BaWindow(ctx, a.K, a.cam_ext, fix_rule=1)                    # empty again after its only keyframe left
        popped.push(5, good)
        popped.pop(5)
        cases = [("null window", None, cur, good, 0, None), ("null pose", a.handle, cur, None, 0, None), ("n_fused < 0", a.handle, cur, good, -1, ids),
                 ("ids missing", a.handle, cur, good, 3, None), ("keyframe not held", a.handle, 424242, good, 0, None),
                 ("empty window", empty.handle, cur, good, 0, None), ("emptied window", popped.handle, 5, good, 0, None),
                 ("NaN", a.handle, cur, nan, 0, None), ("infinity", a.handle, cur, inf, 3, ids), ("zero quaternion", a.handle, cur, zero_q, 0, None)]
        for what, handle, kf, pose, n, lm in cases:
            res = result()
            assert _raw(ctx, handle, kf, pose, n, lm, res) == -1, what            # SSX_ERR_INVALID_ARG
            assert (res.n_keyframes, res.n_landmarks, res.n_points_moved, res.n_fused_removed) == (-3, -3, -3, -3), what
            assert (poses == guard).all() and (points == guard).all() and (anchors == -77).all(), what
            same_export(a.export(), twin.export())
            same_solve(a.solve(), twin.solve())                                  # ... and the device copies are the twin's
        popped.close()
        with pytest.raises(Exception):
            a.loop_correct(424242, good)
        # a valid call still works, with the twin's bits (the estimates moved with the solves: a new corrected pose)
        ex = a.export()
        good = wlc.corrected_pose(ex["poses"][list(ex["kf_ids"]).index(cur)], **wlc.FAR)
        ra, rt = a.loop_correct(cur, good, ids), twin.loop_correct(cur, good, ids)
        assert ra["n_fused_removed"] == 3 and np.array_equal(ra["poses"], rt["poses"]) and np.array_equal(ra["points"], rt["points"])
        _, want = stage1_of_export(ctx, ex, list(ex["kf_ids"]).index(cur), good)
        assert np.array_equal(ra["poses"], want["poses"]) and np.array_equal(ra["points"], want["points"])
        same_solve(a.solve(), twin.solve())
        # a null result is allowed
        assert _raw(ctx, a.handle, cur, good, 0, None, None) == 0
    finally:
        a.close(); twin.close(); empty.close()
