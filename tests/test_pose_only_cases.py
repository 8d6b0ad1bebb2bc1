"""CPU: the pose-only cases of tests/pose_only_cases.py against tests/golden/ref_po_trace.npz -- the compiled reference's runs WITH the
record g2o exposes in postIteration (trials, lambda, robust chi2 per LM iteration; active edges, iterations, terminated, outliers per
optimize()).  The oracle must reproduce every count and flag of every stable iteration and stay within the stored bars
(pose_only_cases.compare_with_fixture); where oracle/_ref exists the live reference is held to the fixture and the oracle to it.
Each case's claim is checked on the reference's record, and the fixture's own conditions (make_po_trace.py refuses to write one that
breaks them) are checked again here.

The test that matters most: test_oracle_matches_the_fixture fails for an oracle in which an accepted trial no longer resets ni to 2
(plane-257 and plane-513 among others: lambda of the next rejected trial is off by a factor of 2 and more) -- a defect that moves no
final pose by more than 4.2e-13 and no mask at all, and which the suite could not see before."""
import os

import numpy as np
import pytest

import pose_only_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUN_IDS = [pc.run_key(*r) for r in pc.RUNS]


def _have_ref_lib(po):
    return os.path.exists(os.path.join(os.path.dirname(po.__file__), "_ref", "libssvio_ref.so"))


@pytest.mark.parametrize("name,rounds,iters", pc.RUNS, ids=RUN_IDS)
def test_oracle_matches_the_fixture(po, name, rounds, iters):
    runs, glob = pc.load_fixture()
    got = po.pose_only_trace(pc.problem(name), "oracle", rounds=rounds, iters=iters)
    pc.compare_with_fixture(got, runs[pc.run_key(name, rounds, iters)], glob)


@pytest.mark.parametrize("name,rounds,iters", pc.RUNS, ids=RUN_IDS)
def test_live_reference_matches_the_fixture_and_the_oracle(po, name, rounds, iters):
    if not _have_ref_lib(po):
        pytest.skip("oracle/_ref/libssvio_ref.so is not built here")
    runs, glob = pc.load_fixture()
    fx = runs[pc.run_key(name, rounds, iters)]
    ref = po.pose_only_trace(pc.problem(name), "ref", rounds=rounds, iters=iters)
    pc.compare_with_fixture(ref, fx, glob)
    # the traced entry of the driver is the plain one plus a listener: same bytes
    plain = po.pose_only(pc.problem(name), "ref", rounds=rounds, iters=iters)
    assert plain["pose"].tobytes() == ref["pose"].tobytes() and np.array_equal(plain["inliers"], ref["inliers"])
    # the oracle against the LIVE reference: the fixture's structure, the live record's values
    live = dict(fx, pose=ref["pose"], inliers=ref["inliers"], n_inliers=ref["n_inliers"], chi2=ref["chi2"], lam=ref["lam"], trials=ref["trials"],
                active=ref["active"], iters_run=ref["iters_run"], terminated=ref["terminated"], outliers=ref["outliers"])
    pc.compare_with_fixture(po.pose_only_trace(pc.problem(name), "oracle", rounds=rounds, iters=iters), live, glob)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_each_case_contains_what_it_claims(name):
    runs, _ = pc.load_fixture()
    fx = runs[pc.run_key(name, *pc.FULL)]
    pr = pc.problem(name)
    assert pr["M"] == pc.CASES[name][2] and np.isfinite(pr["xyz"]).all() and np.isfinite(pr["uv"]).all() and np.isfinite(pr["pose"]).all()
    assert np.abs(pr["xyz"]).sum(1).min() > 0                                   # no point at the world origin, where the start camera sits
    assert pc.claim_holds(name, fx, pr["gt_pose"]), pc.CLAIMS[name]
    fam = pc.CASES[name][0]
    # ... and the inputs hold what the family says (camera frame of the true pose)
    from tools.synth import quat_rot
    z = np.array([(quat_rot(pr["gt_pose"][:4], p) + pr["gt_pose"][4:])[2] for p in pr["xyz"]])
    if fam == "behind":
        assert (z < -5).sum() == max(1, pr["M"] // 5)
    if fam == "plane":
        assert (np.abs(z) <= 0.02).sum() == max(1, pr["M"] // 10) and (z < -5).sum() == pr["M"] // 10
    if fam == "tinyz":
        assert (np.abs(pr["xyz"][:, 2]) <= 1e-6).sum() == 3
    if fam == "clean":
        from pose_only_cases import _project
        # float32 pixels: half a float32 ulp below 4096 px is 1.2e-4 px
        assert np.abs(pr["uv"]).max() < 4096 and np.abs(_project(pr["gt_pose"], pr["xyz"]) - pr["uv"]).max() < 1.23e-4
    if fam == "axis":
        assert not pr["xyz"][:, :2].any()
    if fam == "coincident":
        assert len(np.unique(pr["xyz"], axis=0)) == (pr["M"] + 1) // 2 - (pr["M"] % 2)


def test_the_ni_case():
    """inside ONE optimize(), within its stable prefix: a rejected trial followed by an accepted one in the same iteration, and a rejected
    trial in a later iteration -- the only place where `ni = 2` on acceptance shows"""
    runs, _ = pc.load_fixture()
    fx = runs[pc.run_key(pc.NI_CASE, *pc.FULL)]
    assert pc.ni_property(fx["trials"], fx["iters_run"], fx["stable"])
    hit = [r for r in range(fx["rounds"]) if pc.ni_property(fx["trials"][r:r + 1], fx["iters_run"][r:r + 1], fx["stable"][r:r + 1])]
    t = fx["trials"][hit[0], :fx["stable"][hit[0]]]
    multi = np.nonzero(t >= 2)[0]
    # the lambda of the later iteration: every rejected trial doubles a factor that restarted at 2 (2, 4, 8, ...), the accepted one
    # multiplies by something in [1/3, 2/3] -- so lambda grows by less than 2^(n (n + 1) / 2) for n rejections; without the reset it grows by more
    j = multi[1]
    n_rej = int(t[j]) - (0 if j == fx["iters_run"][hit[0]] - 1 and fx["terminated"][hit[0]] else 1)
    growth = fx["lam"][hit[0], j] / fx["lam"][hit[0], j - 1]
    assert 2.0 ** (n_rej * (n_rej + 1) / 2) / 3 <= growth * (1 + 1e-12) and growth <= 2.0 ** (n_rej * (n_rej + 1) / 2) * (1 + 1e-12)


def test_every_kernel_sees_every_family_it_must():
    for kern in ("k2", "k6", "generic"):
        names = [n for n in pc.CASES if pc.kernel_of(pc.CASES[n][2]) == kern]
        fams = {pc.CASES[n][0] for n in names}
        assert {"far", "plane", "clean"} <= fams, (kern, fams)
        assert any(pc.CLAIMS[n] == "no_active_round" for n in names), kern
    assert {pc.CASES[n][2] for n in pc.CASES} == set(pc.SIZES)
    for n in pc.CASES:
        if pc.CASES[n][0] in ("far", "plane"):
            assert set(pc.settings(n)) == {pc.FULL, *pc.TRUNCATED}
    assert {"farsmall1.5-1", "small-3", "coincident-6"} <= set(pc.CASES)


def test_fixture_invariants():
    runs, glob = pc.load_fixture()
    assert set(runs) == set(RUN_IDS)
    assert os.path.getsize(os.path.join(GOLDEN, "ref_po_trace.npz")) < os.path.getsize(os.path.join(GOLDEN, "ref_golden.npz"))
    n_rec = n_stable = 0
    floor_lam = floor_chi2 = 0.0
    for key, fx in runs.items():
        assert (fx["stable"] <= fx["iters_run"]).all() and (fx["iters_run"] <= fx["iters"]).all()
        assert fx["stable"][0] >= min(5, fx["iters_run"][0]), key          # what "stable" may hide, part 1
        for r in range(fx["rounds"]):
            k, n = fx["stable"][r], fx["iters_run"][r]
            assert (fx["trials"][r, :n] >= 1).all() and (fx["trials"][r, :n] <= 10).all() and not fx["trials"][r, n:].any(), key
            assert (fx["lam"][r, :n] > 0).all() and (fx["chi2"][r, :n] >= 0).all(), key
            assert not fx["d_lam"][r, k:].any() and not fx["d_chi2"][r, k:].any()
            assert fx["iters_run"][r] == 0 if fx["active"][r] == 0 else fx["iters_run"][r] >= 1, key
            assert not fx["round_stable"][r] or k == n
            if r + 1 < fx["rounds"]:
                assert fx["active"][r + 1] == fx["M"] - fx["outliers"][r], key
            # Terminate ends an optimize(); one that ran fewer iterations than asked was terminated
            assert fx["terminated"][r] == 1 if 0 < n < fx["iters"] else True, key
        assert fx["active"][0] == fx["M"] and fx["n_inliers"] == fx["M"] - fx["outliers"][-1] == int(fx["inliers"].sum()), key
        n_rec += int(fx["iters_run"].sum()); n_stable += int(fx["stable"].sum())
        head = min(5, int(fx["stable"][0]))
        floor_lam = max(floor_lam, fx["d_lam"][0, :head].max(initial=0.0)); floor_chi2 = max(floor_chi2, fx["d_chi2"][0, :head].max(initial=0.0))
    assert (n_rec, n_stable) == (glob["n_recorded"], glob["n_stable"]) and n_stable >= 0.9 * n_rec      # part 2
    # the floors are what the decisive head of every run measures (float32, rounded up, in the per-iteration arrays)
    assert glob["floor_lam"] <= floor_lam <= glob["floor_lam"] * (1 + 1e-6) and glob["floor_chi2"] <= floor_chi2 <= glob["floor_chi2"] * (1 + 1e-6)
    assert glob["K"] == 4.0
