"""Shared by tests/test_window_loop_model.py (CPU) and tests/test_window_loop_correct_gpu.py: corrected poses, matched pairs on the
map model, and small ssx_ba_window histories (pushes in any id order, pops, removals, a solve in between) for the loop correction
of a resident window."""
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import synth  # noqa: E402


def corrected_pose(pose, w=(0.002, -0.003, 0.001), t=(0.05, -0.02, 0.08)):
    """`pose` moved by the rotation vector w and the translation t: a corrected_current_pose_ (default: a few centimetres and
    milliradians; the window moves rigidly with it, so any size leaves the reprojection errors where they were)"""
    d = np.concatenate([synth.small_rot_quat(np.array(w, dtype=np.float64)), t])
    d[:4] /= np.linalg.norm(d[:4])
    return synth.pose_mul(d, np.asarray(pose, dtype=np.float64))


FAR = dict(w=(0.01, -0.04, 0.02), t=(0.8, -0.1, 1.5))      # the drift of tests/loop_correct_cases.py


def pick_matches(m, cur_kf, loop_kf, n_both, n_cur_empty, n_loop_empty):
    """(current feature index, loop feature index) pairs on a tools.mapmodel.ActiveMap: n_both with two map points (the `if` of
    loopclosing.cpp:439), n_cur_empty whose current feature has none (the `else`), n_loop_empty whose loop feature has none (the
    `else`, storing a null pointer).  Loop map points are taken from outside the active map: a loop closes on a place left long ago."""
    cur, loop = m.kfs[cur_kf]["feats"], m.kfs[loop_kf]["feats"]
    assert loop_kf not in m.active_kfs
    cur_with = [i for i, f in enumerate(cur) if m._lock(f) is not None]
    cur_without = [i for i, f in enumerate(cur) if m._lock(f) is None]
    loop_with = [i for i, f in enumerate(loop) if m._lock(f) is not None and f.lm not in m.active_mps]
    loop_without = [i for i, f in enumerate(loop) if m._lock(f) is None]
    assert len(cur_with) >= n_both + n_loop_empty and len(cur_without) >= n_cur_empty, (len(cur_with), len(cur_without))
    assert len(loop_with) >= n_both + n_cur_empty and len(loop_without) >= n_loop_empty, (len(loop_with), len(loop_without))
    pairs = [(cur_with[i], loop_with[i]) for i in range(n_both)]
    pairs += [(cur_without[i], loop_with[n_both + i]) for i in range(n_cur_empty)]
    pairs += [(cur_with[n_both + i], loop_without[i]) for i in range(n_loop_empty)]
    return pairs


@dataclass(frozen=True)
class WindowSpec:
    """A window's history.  n_kf + n_extra keyframes are pushed (ids in no order: the current keyframe, pushed last, does not carry
    the highest id), the first n_extra are popped again; n_lm + n_remove_lm landmarks (ids in no order), the last n_remove_lm removed
    again.  Landmark j comes with keyframe j mod (pushes) (dense: j mod 2, and every later keyframe sees it with both cameras, so
    that popping more than half of the keyframes kills more than half of the stored observations: the storage is rewritten) and is seen by the first keyframe that stays, by the last one and by others
    in between; j mod 6 == 1: by right cameras only; j mod 7 == 3: fixed by the caller.  Under fix rule 1 the landmarks that came
    with a popped keyframe are fixed.  remove_first_obs: the observations the earliest remaining keyframe holds of the landmarks
    j mod 5 == 2 are removed (their anchor moves to a later keyframe).  solve_at >= 0: a solve after that many pushes (everything
    before it is on the device, everything after it pending).  pops_before_last_push: the pops and removals come before the last
    push (its slots are reused ones) instead of after it.  The last push is never followed by a solve."""
    n_kf: int
    n_lm: int
    seed: int = 0
    n_extra: int = 0
    n_remove_lm: int = 0
    remove_first_obs: bool = False
    solve_at: int = -1
    pops_before_last_push: bool = False
    dense: bool = False
    fix_first_pose: bool = False
    fix_rule: int = 1


def _project(T, p, cam, K, ext):
    pc = synth.quat_rot(T[:4], p) + T[4:]
    if cam:
        pc = synth.quat_rot(ext[1][:4], pc) + ext[1][4:]
    return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]])


def build_window(ctx, spec, **window_args):
    """-> (ssvio_amd.ba.BaWindow, info): the window after spec's history; info = dict(kf_ids in push order (the survivors), cur_kf_id,
    lm_ids (all that were pushed), removed_lm_ids)"""
    from ssvio_amd import ba
    s = spec
    rng = np.random.default_rng(7000 + s.seed)
    K, ext = np.array(synth.KITTI_K), synth.stereo_cam_ext()
    n_push, n_all = s.n_kf + s.n_extra, s.n_lm + s.n_remove_lm
    kf_ids = 1000 + 3 * rng.permutation(n_push)
    if n_push > 1 and kf_ids[-1] == kf_ids.max():                                     # the current keyframe is not the highest id
        kf_ids[[0, -1]] = kf_ids[[-1, 0]]
    lm_ids = 5000 + 7 * rng.permutation(n_all)
    gt = np.array([[0, 0, 0, 1, 0.05 * np.sin(0.7 * i), 0, -0.8 * i] for i in range(n_push)], dtype=np.float64)
    poses = gt.copy()
    for i in range(n_push):
        q = synth.small_rot_quat(rng.uniform(-0.002, 0.002, 3))
        poses[i, :4] = q / np.linalg.norm(q)
        poses[i, 4:] = synth.quat_rot(q, gt[i, 4:]) + rng.uniform(-0.02, 0.02, 3)
    xyz = np.stack([rng.uniform(-12, 12, n_all), rng.uniform(-3, 3, n_all), rng.uniform(16, 50, n_all)], 1)
    first = np.arange(n_all) % (2 if s.dense else n_push)                             # dense: everything comes with the first two keyframes
    first[s.n_lm:] = np.arange(s.n_lm, n_all) % max(n_push - 1, 1)                    # (what is removed again never comes with the last keyframe)
    stay = min(s.n_extra, n_push - 1)                                                 # the earliest keyframe that is never popped
    seen = []
    for j in range(n_all):
        ks = {int(first[j]), max(int(first[j]), stay), n_push - 1}
        ks |= {k for k in range(int(first[j]) + 1, n_push - 1) if s.dense or rng.random() < 0.5}
        seen.append(ks)
    win = ba.BaWindow(ctx, K, ext, fix_rule=s.fix_rule, **window_args)

    gone = set()                                                                      # landmarks removed again

    def push(k):
        new = np.nonzero(first == k)[0]
        obs_lm, obs_uv, obs_cam = [], [], []
        for j in range(n_all):
            if k not in seen[j] or j in gone:
                continue
            cams = [1] if j % 6 == 1 else ([0, 1] if (s.dense or rng.random() < 0.5) else [0])
            for c in cams:
                obs_lm.append(lm_ids[j]); obs_cam.append(c)
                obs_uv.append(_project(gt[k], xyz[j], c, K, ext) + rng.normal(0, 0.4, 2))
        win.push(int(kf_ids[k]), poses[k], new_ids=lm_ids[new], new_xyz=xyz[new] + rng.normal(0, 0.05, (len(new), 3)),
                 new_fixed=(new % 7 == 3).astype(np.uint8), obs_lm=obs_lm, obs_uv=np.array(obs_uv).reshape(-1, 2), obs_cam=obs_cam,
                 pose_fixed=bool(s.fix_first_pose and k == stay))

    def edits(before_last):
        for k in range(s.n_extra):
            win.pop(int(kf_ids[k]))
        if s.n_remove_lm:
            assert win.remove_landmarks(lm_ids[s.n_lm:]) == s.n_remove_lm
            gone.update(range(s.n_lm, n_all))
        if s.remove_first_obs and s.n_kf > 1:
            last_seen = n_push - 1 if before_last else n_push                          # (a landmark keeps an observer that is in the window now)
            ids = [lm_ids[j] for j in range(s.n_lm) if j % 5 == 2 and stay in seen[j] and first[j] <= stay and any(stay < k < last_seen for k in seen[j])]
            win.remove_observations(int(kf_ids[stay]), ids)

    for k in range(n_push):
        if k == n_push - 1 and s.pops_before_last_push:
            assert s.n_kf > 1
            edits(True)
        push(k)
        if k + 1 == s.solve_at:
            assert k < n_push - 1
            win.solve()
    if not s.pops_before_last_push:
        edits(False)
    assert win.size()[:2] == (s.n_kf, s.n_lm), (win.size(), s)
    return win, dict(kf_ids=[int(k) for k in kf_ids[s.n_extra:]], cur_kf_id=int(kf_ids[-1]), lm_ids=lm_ids[:s.n_lm].copy(), removed_lm_ids=lm_ids[s.n_lm:].copy())


def rewrites(win):
    """how often the window's observation storage has been rewritten (include/ssx_test_hooks.h)"""
    import ctypes as C
    f = win.ctx.lib.ssx_ba_window_debug_rewrites
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p]
    return int(f(win.handle))
