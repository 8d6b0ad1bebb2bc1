"""BA driver A/B: the same solves on two builds of the library must return the same BYTES, and how long one window takes.
Every branch of the host driver is visited: small windows singly and in a batch (both Jacobian modes), large windows on the tile
solver, the band chain and the block cyclic reduction, each also through an identity all-reduce hook (the collective branches),
resident ssx_ba_window objects through pushes and pops solved singly and in a batch, and calls with iters = 0 / outer_rounds = 0.
    python tools/ba_driver_ab.py out.npz     (run once per library: SSX_LIB=...; then compare the two files with --compare a.npz b.npz)
    SSX_BA_BAND_CHAIN=1 python tools/ba_driver_ab.py out_chain.npz   (the band chain with segments instead of the cyclic reduction)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = [k for k in a.files if k not in b.files or not np.array_equal(a[k], b[k])] + [k for k in b.files if k not in a.files]
    print("arrays", len(a.files), "different", bad)
    sys.exit(1 if bad else 0)
import ssvio_amd
from ssvio_amd import ba
from tools.synth import make_ba_problem
ctx = ssvio_amd.Context(0)
out = {}
KEYS = ("poses", "points", "chi2", "lam", "trials", "rounds", "n_iters", "n_inliers", "n_outliers", "edge_chi2", "edge_outlier")


def keep(tag, r, keys=KEYS):
    for k in keys:
        if r.get(k) is not None:
            out[f"{tag}_{k}"] = np.asarray(r[k])


cases = [dict(P=10, L=4000, seed=1), dict(P=10, L=700, seed=41), dict(P=4, L=60, obs_per_lm=4, seed=44), dict(P=7, L=300, obs_per_lm=2, seed=45),
         dict(P=10, L=500, seed=46, fix_first_pose=True, frac_fixed=0.3), dict(P=2, L=40, obs_per_lm=2, seed=47), dict(P=9, L=900, seed=48, fix_first_pose=True)]
for i, kw in enumerate(cases):
    pr = make_ba_problem(**kw)
    for jac in (ba.JAC_ANALYTIC, ba.JAC_NUMERIC_G2O):
        keep(f"{i}_{jac}", ba.ba_solve(ctx, pr, jac_mode=jac), KEYS[:5])
probs = [make_ba_problem(**kw) for kw in cases[:5]] * 4
rb = ba.BaBatch(ctx, probs, resident=True).solve()
for i, r in enumerate(rb["results"]):
    keep(f"b{i}", r)
for jac in (ba.JAC_ANALYTIC, ba.JAC_NUMERIC_G2O):                     # one-shot batch, with and without per-edge errors
    for we in (True, False):
        for i, r in enumerate(ba.BaBatch(ctx, probs[:9], jac_mode=jac).solve(want_edges=we)["results"]):
            keep(f"s{jac}{int(we)}_{i}", r)

# one window per large class (more than 16 free keyframes); large_solver: 1 = tiles, 2 = band (refused if the window is not banded)
identity = lambda user, buf, count, stream: 0                         # world_size 1: the collective branches, same sums
large = {"tiles": (dict(P=40, L=1500, obs_per_lm=5, seed=9, loop=False, fix_first_pose=True), 1),
         "chain": (dict(P=30, L=1500, obs_per_lm=5, seed=51, fix_first_pose=True), 2),              # fewer than 8 super-blocks: one workgroup
         "dissected": (dict(P=120, L=4000, obs_per_lm=6, seed=52, fix_first_pose=True), 2),
         "c4": (dict(P=500, L=12000, obs_per_lm=6, seed=43, loop=True, fix_first_pose=True), 2)}    # BASELINE configs[3] shape
for name, (kw, solver) in large.items():
    pr = make_ba_problem(**kw)
    keep(f"L{name}", ba.ba_solve(ctx, pr, outer_rounds=2, iters=5, large_solver=solver))
    keep(f"L{name}_num", ba.ba_solve(ctx, pr, outer_rounds=1, iters=3, large_solver=solver, jac_mode=ba.JAC_NUMERIC_G2O, want_edges=False))
    keep(f"L{name}_hook", ba.ba_solve(ctx, pr, outer_rounds=1, iters=4, large_solver=solver, allreduce=identity, world_size=1))
    keep(f"L{name}_stats", ba.ba_solve(ctx, pr, outer_rounds=1, iters=2, large_solver=solver, collect_stats=True))
pr = make_ba_problem(**cases[1])
keep("hook", ba.ba_solve(ctx, pr, allreduce=identity, world_size=1))
keep("hook_num", ba.ba_solve(ctx, pr, allreduce=identity, world_size=1, jac_mode=ba.JAC_NUMERIC_G2O))

# calls in which no optimize() runs: the input state and its errors come back
for tag, kw in (("it0", dict(iters=0)), ("or0", dict(outer_rounds=0)), ("it0_tiles", dict(iters=0, large_solver=1))):
    pr = make_ba_problem(**(large["tiles"][0] if "tiles" in tag else cases[1]))
    keep(tag, ba.ba_solve(ctx, pr, **kw))
    keep(tag + "_lean", ba.ba_solve(ctx, pr, want_edges=False, **kw))
    if "tiles" not in tag:
        for i, r in enumerate(ba.BaBatch(ctx, probs[:3], **kw).solve()["results"]):
            keep(f"{tag}_b{i}", r)


# resident windows through a few pushes and pops, solved singly and in a batch
def feed_of(pr):
    first = np.full(pr["L"], 10 ** 9, dtype=np.int64)
    np.minimum.at(first, pr["edge_point"], pr["edge_pose"])
    for k in range(pr["P"]):
        new = np.nonzero(first == k)[0]
        e = np.nonzero(pr["edge_pose"] == k)[0]
        yield dict(pose=pr["poses"][k], new_ids=1000 + new, new_xyz=pr["points"][new], new_fixed=pr["point_fixed"][new],
                   obs_lm=1000 + pr["edge_point"][e], obs_uv=pr["edge_uv"][e], obs_cam=pr["edge_cam"][e])


prs = [make_ba_problem(P=14, L=1800, obs_per_lm=5, seed=300 + q, pose_t_noise=0.05) for q in range(3)]
feeds = [list(feed_of(p)) for p in prs]
single = [ba.BaWindow(ctx, p["K"], p["cam_ext"]) for p in prs]
batched = [ba.BaWindow(ctx, p["K"], p["cam_ext"]) for p in prs]
for k in range(14):
    for wins in (single, batched):
        for w, f in zip(wins, feeds):
            if k >= 10:
                w.pop(100 + k - 10)
            w.push(100 + k, **f[k])
    if k >= 8:
        for q, w in enumerate(single):
            keep(f"w{k}_{q}", w.solve())
        for q, r in enumerate(ba.BaWindow.solve_batch(batched)):
            keep(f"wb{k}_{q}", r)
for w in single + batched:
    w.close()
np.savez(sys.argv[1], **out)
print("arrays", len(out))
pr = make_ba_problem(P=10, L=4000, seed=1, uv_f32=True)
for _ in range(5): r = ba.ba_solve(ctx, pr, want_edges=False)
best = 1e9
for rep in range(5):
    t = time.perf_counter()
    for _ in range(20): r = ba.ba_solve(ctx, pr, want_edges=False)
    best = min(best, (time.perf_counter() - t) / 20)
print(f"one window: wall {best * 1e3:.4f} ms, gpu {r['ms_total']:.3f} ms")
