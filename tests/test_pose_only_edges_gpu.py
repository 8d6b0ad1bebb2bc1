"""GPU: every Levenberg decision of the three pose-only kernels -- k_pose_only<2>, k_pose_only<6>, k_pose_only_generic -- against the
COMPILED REFERENCE's record (tests/golden/ref_po_trace.npz, written by tests/golden/make_po_trace.py), on the cases of
tests/pose_only_cases.py: far starts, points behind the camera and within 2 cm of its plane, |z| <= 1e-6, 70 % and 100 % gross
pixels, noise-free pixels from identity and from the solution, coincident points, points on the optical axis, a scene 3 km deep,
M = 1, 3, 6, rounds that start with no active edge -- at (rounds, iters) = (4, 10) and, for the far-start and camera-plane
families, cut short at (1, 1), (1, 3) and (2, 2).

The kernels fill the record through ssx_pose_only_debug_trace (include/ssx_test_hooks.h): traced instantiations of the same kernel
bodies.  Every case goes through it alone and as one job of ONE batch that mixes the three kernels and an empty problem.  Asserted
per run (pose_only_cases.compare_with_fixture):
  * on the stable iterations -- those in which the reference and two builds of the CPU oracle agree on the count; at least the first
    five of every run and 90 % of all -- the trials of each LM iteration, the iterations each optimize() ran, its terminated flag;
    the active edges and the outliers of every round; the mask and the inlier count;
  * lambda and the robust chi2 of each stable iteration within max(floor, 4 x the oracle's own distance from the reference in that
    iteration), the floors measured by make_po_trace.py; the final pose within max(2e-9 (1e-8 for M < 8), 4 x the oracle's distance);
  * the traced run's pose, mask and count are the bytes of ssx_pose_only_opt and ssx_pose_only_opt_batch.
Two cases go through ssx_loop_pose_opt (one warm-up optimize() in front) and are held to the oracle's composition.

test_summary prints, per family and kernel, the worst pose / lambda / chi2 distance as oracle | bar | kernel."""
import collections

import numpy as np
import pytest

import pose_only_cases as pc
from loop_pose_cases import refine_bar
from ssvio_amd import ba, loop

pytestmark = pytest.mark.gpu

RUN_IDS = [pc.run_key(*r) for r in pc.RUNS]
EMPTY = dict(M=0, pose=np.array([0, 0, 0, 1.0, 0, 0, 0]), K=pc.problem("base-200")["K"], xyz=np.zeros((0, 3)), uv=np.zeros((0, 2)))
WORST = collections.defaultdict(lambda: dict(pose=(0.0, 0.0, 0.0), lam=(0.0, 0.0, 0.0), chi2=(0.0, 0.0, 0.0)))      # (family, kernel) -> oracle, bar, kernel


@pytest.fixture(scope="module")
def singles(ctx):
    """every run through the hook in a call of its own"""
    return {pc.run_key(n, r, i): ba.pose_only_trace(ctx, [pc.problem(n)], [(r, i)])[0] for n, r, i in pc.RUNS}


@pytest.fixture(scope="module")
def batch(ctx):
    """every run as one job of ONE call: the three kernel classes mixed, an empty problem in the middle"""
    half = len(pc.RUNS) // 2
    probs = [pc.problem(n) for n, _, _ in pc.RUNS]
    sets = [(r, i) for _, r, i in pc.RUNS]
    res = ba.pose_only_trace(ctx, probs[:half] + [EMPTY] + probs[half:], sets[:half] + [pc.FULL] + sets[half:])
    empty = res.pop(half)
    return dict(zip(RUN_IDS, res)), empty


def _note(name, fx, w):
    slot = WORST[(pc.CASES[name][0], pc.kernel_of(fx["M"]))]
    k = fx["stable"]
    orc = dict(pose=fx["d_pose"], lam=max((fx["d_lam"][r, :k[r]].max(initial=0.0) for r in range(fx["rounds"])), default=0.0),
               chi2=max((fx["d_chi2"][r, :k[r]].max(initial=0.0) for r in range(fx["rounds"])), default=0.0))
    for f in ("pose", "lam", "chi2"):
        d, bar = w[f]
        if d / bar >= slot[f][2] / slot[f][1] if slot[f][1] else True:
            slot[f] = (float(orc[f]), bar, d)


@pytest.mark.parametrize("name,rounds,iters", pc.RUNS, ids=RUN_IDS)
def test_single_call_matches_the_reference(singles, record_property, name, rounds, iters):
    runs, glob = pc.load_fixture()
    key = pc.run_key(name, rounds, iters)
    fx, got = runs[key], singles[key]
    w = pc.compare_with_fixture(got, fx, glob, check_pose=False)
    for f in ("pose", "lam", "chi2"):
        print(f"{key} {pc.kernel_of(fx['M'])} {f}: kernel {w[f][0]:.2e} bar {w[f][1]:.2e}")
        record_property(f"{f}_kernel_vs_reference", w[f][0]); record_property(f"{f}_bar", w[f][1])
    _note(name, fx, w)
    assert w["pose"][0] <= w["pose"][1], ("pose", w["pose"])


@pytest.mark.parametrize("name,rounds,iters", pc.RUNS, ids=RUN_IDS)
def test_batch_matches_the_reference_and_the_single_call(singles, batch, name, rounds, iters):
    runs, glob = pc.load_fixture()
    key = pc.run_key(name, rounds, iters)
    got = batch[0][key]
    pc.compare_with_fixture(got, runs[key], glob)
    one = singles[key]
    for f in ("pose", "inliers", "chi2", "lam", "trials", "active", "iters_run", "terminated", "outliers"):
        assert np.asarray(got[f]).tobytes() == np.asarray(one[f]).tobytes(), f          # one workgroup per problem: the same bits
    assert got["n_inliers"] == one["n_inliers"]


def test_empty_problem_in_the_batch(batch):
    e = batch[1]
    assert e["n_inliers"] == 0 and not e["trials"].any() and not e["active"].any() and not e["iters_run"].any()
    assert np.array_equal(e["pose"], EMPTY["pose"])


@pytest.mark.parametrize("name,rounds,iters", pc.RUNS, ids=RUN_IDS)
def test_traced_run_equals_the_plain_entry_point(ctx, singles, name, rounds, iters):
    p = pc.problem(name)
    plain = ba.pose_only_opt(ctx, p["pose"], p["K"], p["xyz"], p["uv"], rounds=rounds, iters=iters)
    got = singles[pc.run_key(name, rounds, iters)]
    assert plain["pose"].tobytes() == got["pose"].tobytes() and plain["inliers"].tobytes() == got["inliers"].tobytes()
    assert plain["n_inliers"] == got["n_inliers"]


@pytest.mark.parametrize("rounds,iters", (pc.FULL,) + pc.TRUNCATED)
def test_traced_batch_equals_the_plain_batch(ctx, batch, rounds, iters):
    names = [n for n, r, i in pc.RUNS if (r, i) == (rounds, iters)]
    probs = [pc.problem(n) for n in names]
    plain = ba.pose_only_opt_batch(ctx, probs[:3] + [EMPTY] + probs[3:], rounds=rounds, iters=iters)
    assert plain.pop(3)["n_inliers"] == 0
    assert {pc.kernel_of(p["M"]) for p in probs} == {"k2", "k6", "generic"}
    for n, a in zip(names, plain):
        got = batch[0][pc.run_key(n, rounds, iters)]
        assert a["pose"].tobytes() == got["pose"].tobytes() and a["inliers"].tobytes() == got["inliers"].tobytes() and a["n_inliers"] == got["n_inliers"], n


@pytest.mark.parametrize("name", ["far0.2-200", "plane-257", "plane-513", "plane-1537"])
def test_warm_up_pass(ctx, po, name):
    """ssx_loop_pose_opt = one optimize(10) over all edges, its classification discarded, then the four classified rounds (lambda and
    ni restart with every optimize()): against the oracle's composition, as tests/test_loop_pose_gpu.py holds it; and the hook with
    warmup = 1 is that call, bytes and all, with the warm-up pass in its record"""
    p = pc.problem(name)
    a = po.pose_only(p, rounds=1)
    o = po.pose_only(dict(p, pose=a["pose"]), rounds=4)
    g = loop.loop_pose_opt(ctx, p["pose"], p["K"], p["xyz"], p["uv"])
    assert g["n_inliers"] == o["n_inliers"] and np.array_equal(g["inliers"], o["inliers"])
    d = np.abs(g["pose"] - o["pose"]).max()
    print(f"warm-up {name}: kernel - oracle composition {d:.2e} bar {refine_bar(p['M']):.1e}")
    assert d <= refine_bar(p["M"])
    t = ba.pose_only_trace(ctx, [p], [pc.FULL], warmup=1)[0]
    assert t["pose"].tobytes() == g["pose"].tobytes() and t["inliers"].tobytes() == g["inliers"].tobytes() and t["n_inliers"] == g["n_inliers"]
    assert t["active"][0] == t["active"][1] == p["M"] and t["outliers"][0] == -1 and t["iters_run"][0] >= 1
    # the warm-up optimize() is the first optimize() of a plain run: the same record
    runs, glob = pc.load_fixture()
    fx = runs[pc.run_key(name, *pc.FULL)]
    k = fx["stable"][0]
    assert np.array_equal(t["trials"][0, :k], fx["trials"][0, :k])
    assert (np.abs(t["lam"][0, :k] - fx["lam"][0, :k]) / fx["lam"][0, :k] <= np.maximum(glob["floor_lam"], glob["K"] * fx["d_lam"][0, :k])).all()


def test_summary(record_property):
    """per family and kernel: the worst pose / lambda / chi2 distance from the reference as oracle | bar | kernel (filled by
    test_single_call_matches_the_reference)"""
    assert WORST, "run the whole module"
    for (fam, kern), w in sorted(WORST.items()):
        line = "  ".join(f"{f} {w[f][0]:.1e} | {w[f][1]:.1e} | {w[f][2]:.1e}" for f in ("pose", "lam", "chi2"))
        print(f"{fam:11s} {kern:8s} {line}")
        record_property(f"{fam}_{kern}", line)
