"""CPU: ActiveMap.loop_correct (tools/mapmodel.py) -- LoopClosing::CorrectActivateKeyframeAndMappoint (reference:
src/ssvio/loopclosing.cpp:378-456) restated on the map model that drives an ssx_ba_window in the GPU tests.

Stage 1 is held, exactly, to tools/loop_correct_model.stage1 on flat arrays gathered from the same map by this file (in another row
order: the arithmetic is elementwise, so the order must not matter).  The fusion is held to what the reference's pointers do: the
current map point is deleted, its features point at the loop map point, the loop map point is NOT active until a later keyframe
observes it, and then it is a fixed landmark with exactly one edge."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import loop_correct_model as lcm  # noqa: E402
from tools.mapmodel import ActiveMap, make_window_scenario  # noqa: E402
from window_loop_cases import corrected_pose as small_correction, pick_matches  # noqa: E402

N_ACTIVE, CUR_FRAME, LOOP_KF = 5, 8, 100


def drive(frames, upto, outlier_every=29):
    """the map after frames[0 .. upto] with a stand-in for the backend: no estimate moves, every `outlier_every`-th edge is culled
    (backend.cpp:205-227), so that features without a map point and deleted map points exist as in a real drive"""
    m = ActiveMap(N_ACTIVE)
    for r, fr in enumerate(frames[:upto + 1]):
        for l in fr["condemn"]:
            m.condemn(l)
        m.insert_keyframe(fr["kf_id"], fr["pose"], fr["obs"], fr["new_points"], fr["victim"])
        pr, kf_ids, lm_ids, e_feat = m.problem()
        out = (np.arange(pr["E"]) % outlier_every) == (r % outlier_every)
        m.apply(kf_ids, lm_ids, e_feat, pr["poses"], pr["points"], out)
    m.take_edits()
    return m


@pytest.fixture(scope="module")
def frames():
    return make_window_scenario(n_kf=12, n_active=N_ACTIVE, new_per_kf=40, seed=3)


def test_stage1_equals_the_flat_model_exactly(frames):
    m = drive(frames, CUR_FRAME)
    cur_kf = frames[CUR_FRAME]["kf_id"]
    corrected = small_correction(m.kfs[cur_kf]["pose"])
    # flat arrays, gathered here: keyframes in INSERTION order, points in the map's dict order reversed
    kf_rows = list(m.active_kfs)
    mp_rows = list(m.active_mps)[::-1]
    row = {k: i for i, k in enumerate(kf_rows)}
    flat = dict(poses=np.array([m.kfs[k]["pose"] for k in kf_rows]), kf_active=np.ones(len(kf_rows), np.uint8), cur_kf=row[cur_kf],
                corrected_pose=corrected, points=np.array([m.active_mps[l].pos for l in mp_rows]),
                point_anchor=np.array([row[m.active_mps[l].active_obs[0].kf] for l in mp_rows]), point_active=np.ones(len(mp_rows), np.uint8))
    s1, pts, moved = lcm.stage1(flat)
    assert moved.all() and len(mp_rows) > 100
    held = {l: m.active_mps[l] for l in mp_rows}                                        # (a fused point leaves the map; the object keeps its position)
    r = m.loop_correct(cur_kf, corrected, pick_matches(m, cur_kf, LOOP_KF, 6, 2, 2), LOOP_KF)
    for k, T in zip(kf_rows, s1):
        assert np.array_equal(m.kfs[k]["pose"], T), k
    assert np.array_equal(m.kfs[cur_kf]["pose"], corrected)
    for l, x in zip(mp_rows, pts):
        assert np.array_equal(held[l].pos, x), l
    # what the call reports is the same state, rows ascending by id
    assert r["kf_ids"] == sorted(kf_rows) and r["lm_ids"] == sorted(mp_rows)
    assert np.array_equal(r["poses"], s1[np.argsort(kf_rows)]) and np.array_equal(r["points"], pts[np.argsort(mp_rows)])
    assert r["anchors"] == [held[l].active_obs[0].kf for l in sorted(mp_rows)]
    # keyframes outside the window keep their bits
    old = [k for k in m.kfs if k not in m.active_kfs]
    assert old and all(np.array_equal(m.kfs[k]["pose"], fr["pose"]) for fr in frames for k in old if fr["kf_id"] == k)
    # the anchor follows the order of the active observations, not the ids: the oldest ACTIVE observer
    seq = {k: i for i, k in enumerate(m.active_kfs)}
    for l in mp_rows:
        obs = [f.kf for f in held[l].active_obs]
        assert obs and seq[obs[0]] == min(seq[k] for k in obs)


def test_fusion_is_a_removal_until_the_loop_point_is_observed_again(frames):
    m = drive(frames, CUR_FRAME)
    cur_kf = frames[CUR_FRAME]["kf_id"]
    pairs = pick_matches(m, cur_kf, LOOP_KF, 6, 2, 2)
    cur, loop = m.kfs[cur_kf]["feats"], m.kfs[LOOP_KF]["feats"]
    before = [(m._lock(cur[c]), m._lock(loop[l])) for c, l in pairs]
    fused_cur = [c for c, l in before if c is not None and l is not None]
    obs_before = {c.id: list(c.obs) for c in fused_cur}
    loop_obs_before = {l.id: len(l.obs) for _, l in before if l is not None}
    in_window_before = set(m.in_window)
    r = m.loop_correct(cur_kf, small_correction(m.kfs[cur_kf]["pose"]), pairs, LOOP_KF)
    assert r["fused"] == [c.id for c in fused_cur] and len(fused_cur) == 6
    pr, kf_ids, lm_ids, _ = m.problem()
    for (c, l), (ci, li) in zip(before, pairs):
        if c is not None and l is not None:
            # the current point is gone, from the map and from the graph; its features (every keyframe's) point at the loop point
            assert c.id not in m.mps and c.id not in m.active_mps and c.id not in lm_ids and c.id not in m.in_window
            assert all(f.lm == l.id for f in obs_before[c.id]) and cur[ci].lm == l.id
            assert l.obs[loop_obs_before[l.id]:] == obs_before[c.id]                  # AddObservation, in order
        elif l is not None:
            assert cur[ci].lm == l.id and len(l.obs) == loop_obs_before[l.id]         # the `else`: no AddObservation
        else:
            assert cur[ci].lm is None                                                 # the `else` with a null loop point
            assert c.id in m.mps and c.obs and cur[ci] in c.obs                       # (the reference leaves the point its observation)
        if l is not None:
            assert l.id not in m.active_mps and l.id not in lm_ids and not l.active_obs   # never AddActiveObservation
    # the edit a window replays: the fused points it held leave
    (kind, arg), = m.take_edits()
    assert kind == "loop_correct" and arg["cur"] == cur_kf and list(arg["fused"]) == r["fused"]
    assert set(r["fused"]) <= in_window_before
    # the next keyframe tracks the current keyframe's features: it observes the loop points
    loop_pts = [l for _, l in before if l is not None]
    nxt = frames[CUR_FRAME + 1]
    obs = list(nxt["obs"]) + [(l.id, (600.0 + 3 * i, 180.0 + i)) for i, l in enumerate(loop_pts)]
    m.insert_keyframe(nxt["kf_id"], nxt["pose"], obs, nxt["new_points"], nxt["victim"])
    pr, kf_ids, lm_ids, e_feat = m.problem()
    push = [a for k, a in m.take_edits() if k == "push"][0]
    for l in loop_pts:
        assert l.id in m.active_mps and l.id in lm_ids
        row = lm_ids.index(l.id)
        assert pr["point_fixed"][row] == 1 and int((pr["edge_point"] == row).sum()) == 1
        assert pr["edge_pose"][pr["edge_point"] == row][0] == kf_ids.index(nxt["kf_id"])
        at = list(push["new_ids"]).index(l.id)                                        # it comes back like any landmark that left ...
        assert push["new_fixed"][at] == 1 and np.array_equal(push["new_xyz"][at], l.pos)   # ... fixed, at the position the map holds
    assert not any(c.id in lm_ids for c in fused_cur)
    # the fused points' observations in the new keyframe are dropped (weak_ptr expired, keyframe.cpp:48 never sees them)
    assert not any(f.lm in r["fused"] for f in m.kfs[nxt["kf_id"]]["feats"])


def test_a_pair_whose_points_are_one_point_is_refused(frames):
    m = drive(frames, CUR_FRAME)
    cur_kf = frames[CUR_FRAME]["kf_id"]
    cur = m.kfs[cur_kf]["feats"]
    i = [k for k, f in enumerate(cur) if m._lock(f) is not None][0]
    with pytest.raises(AssertionError):
        m.loop_correct(cur_kf, m.kfs[cur_kf]["pose"], [(i, i)], cur_kf)                 # the loop keyframe IS the current one


def test_existing_edits_replay_is_unchanged(frames):
    """apply_edits still accepts the old edit kinds and now returns the (empty) list of corrections"""
    from tools.mapmodel import apply_edits

    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a, **k: self.calls.append(name) or {"name": name}

    m = ActiveMap(N_ACTIVE)
    fr = frames[0]
    m.insert_keyframe(fr["kf_id"], fr["pose"], fr["obs"], fr["new_points"], fr["victim"])
    w = Recorder()
    assert apply_edits(w, m.take_edits()) == [] and w.calls == ["push"]
    m._edits.append(("loop_correct", dict(cur=fr["kf_id"], corrected=fr["pose"], fused=np.zeros(0, np.int64))))
    assert apply_edits(w, m.take_edits()) == [{"name": "loop_correct"}]
