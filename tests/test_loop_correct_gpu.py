"""GPU: ssx_loop_correct (the geometry of LoopClosing::LoopCorrect as one call) against the 60-digit fixture
tests/golden/loop_correct_hp.npz, against the shipped optimiser, against its model tools/loop_correct_model.py, and at its edges.

Bars.  The kernels perform the model's operations in the model's order and differ from it in FMA contraction only, so each distance
from the 60-digit truth is held to  max(4 x the model's own distance, 4 x np.spacing(the quantity's largest coordinate))  -- the
factor 4 of the fixture (the project's margin for an equivalent evaluation order), and the ulp floor so that a case where
the model happens to be exact does not demand exactness of a differently contracted build.  Distances: loop_correct_cases.pose_distance /
point_distance.  Stage 3 has two truths (tests/golden/make_loop_correct_hp.py): with the optimiser bypassed (iterations = 0) its points are
exactly the points it was given; for stated poses the CPU test holds the model to the fixture, and here the device is held to the model on
the poses the device itself produced (test_stage3_on_real_optimiser_output), with the same bar.  Every measured distance is printed (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

import loop_correct_cases as lcc
from ssvio_amd import ba, loop
from tools import loop_correct_model as lcm

pytestmark = pytest.mark.gpu
HP = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_correct_hp.npz"))
FACTOR = float(HP["factor"])
CASE = {n: lcc.make(n) for n in lcc.NAMES}
_RUNS = {}


def bar(name, quantity, truth):
    k = lcc.NAMES.index(name)
    largest = float(np.abs(truth).max()) if np.size(truth) else 1.0
    return max(FACTOR * float(HP[f"model_{quantity}"][k]), FACTOR * float(np.spacing(largest)))


def run(ctx, name, iters):
    """one call per (case, iterations), shared by the tests and left unchanged"""
    if (name, iters) not in _RUNS:
        _RUNS[(name, iters)] = loop.loop_correct(ctx, CASE[name], iters=iters)
    return _RUNS[(name, iters)]


def flat_problem(pr, s1_poses):
    return dict(poses=s1_poses, fixed=lcm.fixed_set(pr), ei=pr["ei"], ej=pr["ej"], meas=pr["meas"])


@pytest.mark.parametrize("name", lcc.NAMES)
def test_stage1_and_stage3_against_60_digits(ctx, name):
    pr = CASE[name]
    r = run(ctx, name, 0)                                                   # the optimiser bypassed: stage 3's new pose is its old pose
    assert r["n_iters"] == 0
    pact = pr["point_active"] != 0
    t_poses, t_pts = HP[f"{name}_s1_poses"], HP[f"{name}_s1_points"]
    got = [("s1_poses", lcc.pose_distance(r["stage1_poses"], t_poses), bar(name, "s1_poses", t_poses)),
           ("s1_points", lcc.point_distance(r["points"][pact], t_pts[pact]), bar(name, "s1_points", t_pts)),
           ("identity", lcc.point_distance(r["points"][~pact], t_pts[~pact]), bar(name, "identity", t_pts))]
    print(name, "  ".join(f"{q} {d:.2e} (bar {b:.2e})" for q, d, b in got))
    for q, d, b in got:
        assert d <= b, (name, q, d, b)
    # with the optimiser bypassed the poses returned are the stage-1 poses
    assert np.array_equal(r["poses"], r["stage1_poses"])


@pytest.mark.parametrize("name", ["lc12", "lc60", "lc200", "only_cur", "far", "half_turn", "no_change"])
def test_stage2_is_the_shipped_optimiser_bit_for_bit(ctx, name):
    pr = CASE[name]
    r = run(ctx, name, 20)
    g = ba.pose_graph_opt(ctx, flat_problem(pr, r["stage1_poses"]), iters=20)
    keep = pr["keep_kf"]
    others = np.arange(pr["P"]) != keep
    assert r["n_iters"] == g["n_iters"] >= 1
    assert np.array_equal(r["poses"][others], g["poses"][others])
    assert np.array_equal(r["chi2"], g["chi2"]) and np.array_equal(r["lambdas"], g["lambdas"]) and np.array_equal(r["trials"], g["trials"])
    assert r["chi2_initial"] == g["chi2_initial"] and r["chi2_final"] == g["chi2_final"]
    assert np.array_equal(r["edge_err"], g["edge_err"])
    fixed = lcm.fixed_set(pr) != 0
    assert np.array_equal(r["poses"][fixed & others], r["stage1_poses"][fixed & others])
    if keep >= 0:
        assert np.array_equal(r["poses"][keep], r["stage1_poses"][keep])
    if name == "lc60":                                                      # the kept keyframe is free here: the optimiser did move it
        assert not fixed[keep] and not np.array_equal(g["poses"][keep], r["stage1_poses"][keep])
    # the stage-1 state does not depend on what follows it
    assert np.array_equal(r["stage1_poses"], run(ctx, name, 0)["stage1_poses"])


@pytest.mark.parametrize("name", ["lc12", "lc60", "lc200", "only_cur", "far", "half_turn", "no_change"])
def test_stage3_on_real_optimiser_output(ctx, name):
    pr = CASE[name]
    r, r0 = run(ctx, name, 20), run(ctx, name, 0)
    pact = pr["point_active"] != 0
    assert np.array_equal(r["points"][pact], r0["points"][pact])            # stage 1's points do not depend on the optimiser
    g = ba.pose_graph_opt(ctx, flat_problem(pr, r["stage1_poses"]), iters=20)   # the estimates (the kept keyframe's too)
    p1 = r0["points"].copy(); p1[~pact] = pr["points"][~pact]
    _, p3, _ = lcm.stage3(pr, r["stage1_poses"], g["poses"], p1)
    d = lcc.point_distance(r["points"][~pact], p3[~pact])
    b = bar(name, "s3_points", p3)                                          # the bar of the first test, for stage 3's quantity
    print(name, f"stage 3 on the optimiser's poses: device - model {d:.2e} (bar {b:.2e})")
    assert d <= b
    lcc.check_invariants(pr, r["stage1_poses"], g["poses"], r["poses"], r["points"])
    for key, v in lcc.expected_counts(pr).items():
        assert r[key] == v, key


@pytest.mark.parametrize("name", ["all_fixed", "no_edges", "lc12_n0", "lc12_n1"])
def test_nothing_to_optimise_and_tiny_point_sets(ctx, name):
    pr = CASE[name]
    r = run(ctx, name, 20)
    if name in ("all_fixed", "no_edges"):
        assert r["n_iters"] == 0 and len(r["chi2"]) == 0 and np.array_equal(r["poses"], r["stage1_poses"])
        assert not np.array_equal(r["stage1_poses"], pr["poses"])           # stage 1 ran
        moved3 = (pr["point_active"] == 0) & (pr["point_anchor"] >= 0)
        assert moved3.any() and not np.array_equal(r["points"][moved3], pr["points"][moved3])   # stage 3 ran (points move by rounding)
        opt = r["stage1_poses"]
    else:
        assert r["n_iters"] >= 1 and r["points"].shape == (pr["N"], 3)
        opt = ba.pose_graph_opt(ctx, flat_problem(pr, r["stage1_poses"]), iters=20)["poses"]
    lcc.check_invariants(pr, r["stage1_poses"], opt, r["poses"], r["points"])
    for key, v in lcc.expected_counts(pr).items():
        assert r[key] == v, key
    r0 = run(ctx, name, 0)
    lcc.check_invariants(pr, r0["stage1_poses"], r0["stage1_poses"], r0["poses"], r0["points"])


def _raw_call(ctx, pr, iters=20, guard=0.0):
    """the C call on arrays with guard words behind poses and points -> (status, arrays, guarded poses, guarded points)"""
    prob, a = loop.loop_correct_struct(pr, iters)
    P, N = len(a["poses"]), len(a["points"])
    gp = np.full(7 * P + 16, guard); gp[:7 * P] = a["poses"].ravel()
    gx = np.full(3 * N + 16, guard); gx[:3 * N] = a["points"].ravel()
    prob.poses = gp.ctypes.data_as(loop.dbl_p)
    prob.points = gx.ctypes.data_as(loop.dbl_p)
    res = loop.LoopCorrectResult()
    ctx.lib.ssx_loop_correct.restype = C.c_int
    ctx.lib.ssx_loop_correct.argtypes = [C.c_void_p, C.POINTER(loop.LoopCorrectProblem), C.c_int32, C.POINTER(loop.LoopCorrectResult)]
    st = ctx.lib.ssx_loop_correct(ctx.handle, C.byref(prob), iters, C.byref(res))
    return st, a, gp, gx, res


def test_guard_words_invalid_arguments_and_determinism(ctx):
    pr = CASE["lc60"]
    P, N = pr["P"], pr["N"]
    guard = -7.25
    st, a, gp, gx, res = _raw_call(ctx, pr, guard=guard)
    assert st == 0 and (gp[7 * P:] == guard).all() and (gx[3 * N:] == guard).all()
    r = run(ctx, "lc60", 20)
    assert np.array_equal(gp[:7 * P].reshape(P, 7), r["poses"]) and np.array_equal(gx[:3 * N].reshape(N, 3), r["points"])   # identical calls, identical bits
    assert np.array_equal(a["stage1_poses"], r["stage1_poses"]) and np.array_equal(a["edge_err"][:pr["E"]], r["edge_err"])
    assert res.pg.n_iters == r["n_iters"] and res.n_points_skipped == r["n_points_skipped"]
    # skipped points keep their bits
    exp = lcc.expected_counts(pr)
    act, anc, pact = pr["kf_active"] != 0, pr["point_anchor"], pr["point_active"] != 0
    skipped = ~((pact & (anc >= 0) & act[np.maximum(anc, 0)]) | (~pact & (anc >= 0)))
    assert skipped.sum() == exp["n_points_skipped"] > 0 and np.array_equal(r["points"][skipped], pr["points"][skipped])
    # invalid arguments: SSX_ERR_INVALID_ARG, every in/out array and optional output untouched
    not_active = dict(pr, kf_active=pr["kf_active"].copy()); not_active["kf_active"][pr["cur_kf"]] = 0
    bad_anchor = dict(pr, point_anchor=pr["point_anchor"].copy()); bad_anchor["point_anchor"][N - 1] = P
    low_anchor = dict(pr, point_anchor=pr["point_anchor"].copy()); low_anchor["point_anchor"][0] = -2
    bad_edge = dict(pr, ej=pr["ej"].copy()); bad_edge["ej"][3] = P
    for what, bad in [("cur not active", not_active), ("cur_kf", dict(pr, cur_kf=P)), ("loop_kf", dict(pr, loop_kf=-1)), ("keep_kf", dict(pr, keep_kf=P)),
                      ("initial_kf", dict(pr, initial_kf=-2)), ("anchor high", bad_anchor), ("anchor low", low_anchor), ("edge", bad_edge)]:
        st, a, gp, gx, res = _raw_call(ctx, bad, guard=guard)
        assert st == -1, what                                               # SSX_ERR_INVALID_ARG
        assert np.array_equal(gp[:7 * P].reshape(P, 7), pr["poses"]) and np.array_equal(gx[:3 * N].reshape(N, 3), pr["points"]), what
        assert (gp[7 * P:] == guard).all() and (gx[3 * N:] == guard).all(), what
        assert not a["stage1_poses"].any() and not a["edge_err"].any() and not a["chi2"].any() and not a["trials"].any(), what
    with pytest.raises(Exception):
        loop.loop_correct(ctx, not_active)
    # the context still works, with the same bits
    again = loop.loop_correct(ctx, pr)
    assert np.array_equal(again["poses"], r["poses"]) and np.array_equal(again["points"], r["points"])


def test_pose_graph_opt_after_loop_correct_has_fresh_context_bits():
    """the shared workspace is left clean: ssx_pose_graph_opt after ssx_loop_correct on one context == on a fresh context"""
    import ssvio_amd
    from tools import synth
    pg = synth.make_pose_graph_problem(P=60, n_loops=2, seed=11, meas_noise=0.02, drift=0.05)
    fresh_ctx = ssvio_amd.Context(0)
    try:
        fresh = ba.pose_graph_opt(fresh_ctx, pg)
    finally:
        fresh_ctx.close()
    used_ctx = ssvio_amd.Context(0)
    try:
        loop.loop_correct(used_ctx, CASE["lc200"])
        loop.loop_correct(used_ctx, CASE["no_edges"])
        after = ba.pose_graph_opt(used_ctx, pg)
    finally:
        used_ctx.close()
    for k in ("poses", "chi2", "lambdas", "trials", "edge_err"):
        assert np.array_equal(fresh[k], after[k]), k
    assert fresh["n_iters"] == after["n_iters"]
