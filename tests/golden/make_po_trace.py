"""tests/golden/ref_po_trace.npz: the compiled reference's pose-only runs on the cases of tests/pose_only_cases.py, WITH the record g2o
exposes in postIteration (oracle/ref_driver.cpp: ref_pose_only_trace), and how far a faithful CPU implementation lands from it.

Per run (case x (rounds, iters), key = pose_only_cases.run_key; the file holds each field packed run after run, and
pose_only_cases.load_fixture() unpacks it):
    _pose, _mask (packbits), _n            the reference's result
    _chi2, _lam, _trials [rounds, iters]   its record per LM iteration (zero where an iteration did not run)
    _round [rounds, 4]                     active edges, iterations run, terminated, outliers after the classification
    _stable [rounds]                       the STABLE PREFIX of each optimize(): the leading iterations in which the reference and both
                                           builds of the oracle took the same number of trials -- on the problem as it is, with its edges
                                           in reverse order, with its map points moved by two ulps and with its start moved by one (witnesses())
    _round_stable [rounds]                 1 = all three also ran the same number of iterations and agree on terminated
    _d_pose                                the oracle's distance from the reference, the larger of its two builds: max |pose difference|
    _d_lam, _d_chi2 [rounds, iters]        ... and the relative difference of lambda / chi2 in every stable iteration (0 elsewhere; float32,
                                           rounded up)
The two builds are the regular one (-ffp-contract=off) and one with fused multiply-adds (-mfma -ffp-contract=fast: every product-sum
rounds differently, as the GPU's do) -- tests/golden/make_noise_floor.py's yardstick.  Once a run has converged, whether a trial is
accepted hangs on the last bits of two nearly equal chi2 sums, and three faithful implementations stop agreeing on the counts: those
iterations are not held against anybody, but they may not be many.  This script REFUSES to write a fixture in which
    * some case's first optimize() is not stable through its first five iterations (all of them when it runs fewer), or
    * fewer than 90 % of all recorded iterations are stable, or
    * the three do not agree on every mask and on the active / outlier counts of every round, or
    * a case's claim (pose_only_cases.CLAIMS) does not hold on the reference's record;
pick another seed in tests/pose_only_cases.py then.
Global: K = 4 (the factor of the triangulation and P3P fixtures) and the floors floor_lam, floor_chi2: the largest _d_lam / _d_chi2 over the
first five iterations of every run's first optimize() -- the part of a run in which every decision is decisive (the first condition
above), so that what the two builds differ by there is what rounding alone does to lambda and chi2.  The bar of an iteration is
max(floor, K x that iteration's own distance): an iteration in which the three agree on the count by luck only -- rho at rounding
level, where lambda's factor max(1/3, 1 - (2 rho - 1)^3) can be anything between 1/3 and 2/3 -- carries a large distance of its own
and is held to no more than that; it cannot widen the bar of any other.  chi2_abs: see rel_chi2.

Run where the reference compiles (oracle/_ref):  python tests/golden/make_po_trace.py     (--dry: measure and print, write nothing)"""
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as po  # noqa: E402
import pose_only_cases as pc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_po_trace.npz")
K_FACTOR = 4.0
HEAD = 5          # the iterations of a run's first optimize() that must be stable, and over which the floors are taken
# chi2 is compared relative to |reference| + 1e-7 x the run's first chi2 (make_noise_floor.py's form) + CHI2_ABS: a noise-free run ends
# at chi2 ~ 1e-20 px^2, the square of the projection's rounding error, where a relative difference means nothing.  1e-12 px^2 is a
# residual of 1e-6 px, a sixtieth of the spacing of float32 pixels at 1000 px.
CHI2_ABS = 1e-12
# A projected pixel below 4096 px carries a rounding error of a few ulps, say 8 x 2^-53 x 4096 = 3.6e-12 px; a chi2 of two such
# residuals per edge is nothing but that rounding and cannot decide a trial.
CHI2_ROUNDING = 2 * (8 * 2.0 ** -53 * 4096) ** 2


def rel_chi2(a, ref, first):
    return np.abs(a - ref) / (np.abs(ref) + 1e-7 * first + CHI2_ABS)


def rel_lam(a, ref):
    return np.abs(a - ref) / np.abs(ref)


def fma_oracle():
    so = os.path.join(tempfile.mkdtemp(prefix="ssx_oracle_fma_"), "liboracle_fma.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-mfma", "-ffp-contract=fast", "-w", "-o", so,
                           *sorted(glob.glob(os.path.join(ROOT, "oracle", "src", "*.cpp"))), "-lm"])
    return C.CDLL(so)


def stable_prefix(recs, r):
    n = min(int(x["iters_run"][r]) for x in recs)
    k = 0
    while k < n and len({int(x["trials"][r, k]) for x in recs}) == 1:
        k += 1
    return k


def witnesses(pr, rounds, iters, fma):
    """More runs that decide what is stable, none of them the code under test: the GPU sums its edges in another order and rounds
    every product-sum differently, so a decision counts as decisive only if it also survives the edges in reverse order and map points
    moved by two ulps (x (1 + 4.4e-16)) and the start pose by one, in the reference and in both builds of the oracle."""
    rev = dict(pr, xyz=np.ascontiguousarray(pr["xyz"][::-1]), uv=np.ascontiguousarray(pr["uv"][::-1]))
    jit = dict(pr, xyz=pr["xyz"] * (1.0 + 2.0 ** -51))
    # ... and the start pose moved by an ulp: its quaternion's norm then rounds to 1 or not as the GPU's differently fused sum may
    start = dict(pr, pose=pr["pose"] * (1.0 + 2.0 ** -52))
    out = []
    for q in (rev, jit, start):
        out.append(po.pose_only_trace(q, "ref", rounds=rounds, iters=iters))
        out.append(po.pose_only_trace(q, "oracle", rounds=rounds, iters=iters))
        out.append(po.pose_only_trace(q, "oracle", rounds=rounds, iters=iters, lib=fma))
    return out


def measure(name, rounds, iters, fma):
    pr = pc.problem(name)
    ref = po.pose_only_trace(pr, "ref", rounds=rounds, iters=iters)
    orc = [po.pose_only_trace(pr, "oracle", rounds=rounds, iters=iters), po.pose_only_trace(pr, "oracle", rounds=rounds, iters=iters, lib=fma)]
    recs = [ref] + orc + witnesses(pr, rounds, iters, fma)
    stable = np.array([stable_prefix(recs, r) for r in range(rounds)], dtype=np.int32)
    # ... and a decision is decisive only if the chi2 difference it hangs on is more than two sums of M terms can differ by when they
    # are added in another order: (M - 1) 2^-53 chi2 each, plus a few roundings per term -> (M + 8) 2^-52 chi2 for the difference.  The
    # record holds the chi2 a one-trial iteration compared: the one before it.  (An accepted step that lowers chi2 by less than that
    # is rho == 0, Terminate, for whoever sums the two to the same bits.)  Nor is it where chi2 has reached the rounding error of the
    # projection itself (CHI2_ROUNDING): one point, or noise-free pixels met exactly.
    for r in range(rounds):
        for i in range(1, int(stable[r])):
            c0, c1 = ref["chi2"][r, i - 1], ref["chi2"][r, i]
            if abs(c0 - c1) <= (pr["M"] + 8) * 2.0 ** -52 * max(c0, c1) or min(c0, c1) <= CHI2_ROUNDING * pr["M"]:
                stable[r] = i
                break
    round_stable = np.array([len({(int(x["iters_run"][r]), int(x["terminated"][r])) for x in recs}) == 1 and stable[r] == ref["iters_run"][r]
                             for r in range(rounds)], dtype=np.uint8)
    agree = all(np.array_equal(o["inliers"], ref["inliers"]) and np.array_equal(o["active"], ref["active"]) and np.array_equal(o["outliers"], ref["outliers"])
                and o["n_inliers"] == ref["n_inliers"] for o in orc)
    d_pose = max(float(np.abs(o["pose"] - ref["pose"]).max()) for o in orc)
    d_lam = np.zeros((rounds, iters)); d_chi = np.zeros((rounds, iters))
    first = ref["chi2"][0, 0]
    for r in range(rounds):
        k = int(stable[r])
        for o in orc:
            d_lam[r, :k] = np.maximum(d_lam[r, :k], rel_lam(o["lam"][r, :k], ref["lam"][r, :k]))
            d_chi[r, :k] = np.maximum(d_chi[r, :k], rel_chi2(o["chi2"][r, :k], ref["chi2"][r, :k], first))
    return dict(ref=ref, stable=stable, round_stable=round_stable, agree=agree, d_pose=d_pose, d_lam=d_lam, d_chi2=d_chi)


def main():
    dry = "--dry" in sys.argv
    assert po.have_ref(), "oracle/_ref/libssvio_ref.so is needed (where the reference compiles)"
    fma = fma_oracle()
    g = {}
    n_rec = n_stable = 0
    floor_lam = floor_chi2 = 0.0
    problems = []
    for name, rounds, iters in pc.RUNS:
        m = measure(name, rounds, iters, fma)
        ref = m["ref"]
        key = pc.run_key(name, rounds, iters)
        rr = np.stack([ref["active"], ref["iters_run"], ref["terminated"], ref["outliers"]], 1).astype(np.int32)
        g[key + "_pose"] = ref["pose"]; g[key + "_mask"] = np.packbits(ref["inliers"]); g[key + "_n"] = np.array(ref["n_inliers"], dtype=np.int32)
        g[key + "_chi2"] = ref["chi2"]; g[key + "_lam"] = ref["lam"]; g[key + "_trials"] = ref["trials"].astype(np.int8); g[key + "_round"] = rr
        g[key + "_stable"] = m["stable"]; g[key + "_round_stable"] = m["round_stable"]
        g[key + "_d_pose"] = np.array(m["d_pose"]); g[key + "_d_lam"] = m["d_lam"]; g[key + "_d_chi2"] = m["d_chi2"]
        head = min(HEAD, int(m["stable"][0]))
        floor_lam = max(floor_lam, float(m["d_lam"][0, :head].max(initial=0.0))); floor_chi2 = max(floor_chi2, float(m["d_chi2"][0, :head].max(initial=0.0)))
        n_rec += int(ref["iters_run"].sum()); n_stable += int(m["stable"].sum())
        need = min(5, int(ref["iters_run"][0]))
        bad = []
        if m["stable"][0] < need:
            bad.append(f"first optimize() stable for {m['stable'][0]} < {need} iterations")
        if not m["agree"]:
            bad.append("masks / active / outlier counts differ between the reference and the oracle")
        if (rounds, iters) == pc.FULL and not pc.claim_holds(name, dict(ref, stable=m["stable"]), pc.problem(name)["gt_pose"]):
            bad.append(f"claim {pc.CLAIMS[name]} does not hold")
        print(f"{key:22s} M {pc.CASES[name][2]:5d} inl {ref['n_inliers']:5d} active {ref['active']} its {ref['iters_run']} term {ref['terminated']} "
              f"stable {m['stable']} d_pose {m['d_pose']:.1e} d_lam {m['d_lam'].max():.1e} (head {m['d_lam'][0, :head].max(initial=0.0):.1e}) d_chi2 {m['d_chi2'].max():.1e} "
              f"(head {m['d_chi2'][0, :head].max(initial=0.0):.1e}){' NI' if pc.ni_property(ref['trials'], ref['iters_run'], m['stable']) else ''} {'; '.join(bad)}")
        if dry and bad:
            print("    trials", ref["trials"].tolist())
        problems += [f"{key}: {b}" for b in bad]
    frac = n_stable / max(n_rec, 1)
    print(f"stable iterations: {n_stable} of {n_rec} = {100 * frac:.1f} %")
    if frac < 0.9:
        problems.append(f"only {100 * frac:.1f} % of the recorded iterations are stable")
    g["floor_lam"] = np.array(floor_lam); g["floor_chi2"] = np.array(floor_chi2)
    g["K"] = np.array(K_FACTOR); g["chi2_abs"] = np.array(CHI2_ABS)
    g["n_recorded"] = np.array(n_rec); g["n_stable"] = np.array(n_stable)
    print(f"floor_lam {float(g['floor_lam']):.2e} floor_chi2 {float(g['floor_chi2']):.2e}  worst d_pose {max(float(g[pc.run_key(*r) + '_d_pose']) for r in pc.RUNS):.2e}")
    if problems:
        print("REFUSED:\n  " + "\n  ".join(problems))
        if not dry:
            sys.exit(1)
    if dry:
        return
    # packed run after run (a zip entry per run and field would cost more than the data): see pose_only_cases.load_fixture
    keys = [pc.run_key(*r) for r in pc.RUNS]
    cat = lambda f, dt: np.concatenate([np.asarray(g[k + f]).reshape(-1) for k in keys]).astype(dt)   # noqa: E731
    up32 = lambda a: np.nextafter(a.astype(np.float32), np.float32(np.inf)).astype(np.float32) * (a > 0)   # noqa: E731  (rounded UP: a bar never shrinks)
    packed = dict(runs=np.array(keys), rounds=np.array([r for _, r, _ in pc.RUNS], dtype=np.int32), iters=np.array([i for _, _, i in pc.RUNS], dtype=np.int32),
                  M=np.array([pc.CASES[n][2] for n, _, _ in pc.RUNS], dtype=np.int32), pose=cat("_pose", np.float64), mask=cat("_mask", np.uint8),
                  n=cat("_n", np.int32), chi2=cat("_chi2", np.float64), lam=cat("_lam", np.float64), trials=cat("_trials", np.int8),
                  round=cat("_round", np.int32), stable=cat("_stable", np.int8), round_stable=cat("_round_stable", np.uint8),
                  d_pose=cat("_d_pose", np.float64), d_lam=up32(cat("_d_lam", np.float64)), d_chi2=up32(cat("_d_chi2", np.float64)),
                  **{k: g[k] for k in ("floor_lam", "floor_chi2", "K", "chi2_abs", "n_recorded", "n_stable")})
    # (a plain zip with fixed timestamps: the same inputs give the same bytes)
    import io
    import zipfile
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(packed):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(packed[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)
    print("ref_po_trace.npz:", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
