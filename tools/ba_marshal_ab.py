"""BA marshalling A/B without a GPU: the digest of everything prepare() hands on and of the arena plan made from it
(ssx_ba_debug_prepare_digest: every array and scalar of HostPrep the upload reads, every offset of the plan for the single / one-shot
batch placement and for the resident batch's) must be the same on two builds of the library.
    python tools/ba_marshal_ab.py out.json      (once per library: SSX_LIB=...)      python tools/ba_marshal_ab.py --compare a.json b.json
The other side is the parent commit with tools/patches/ba_marshal_digest_parent.diff (the same digest lines over its upload()'s sizing
pass): in a checkout of the parent, `patch -p0 -i <the patch>`, `python -m ssvio_amd.build`, and SSX_LIB=<its libssx.so>.
Cases: those of tools/ba_driver_ab.py (seven small, four large, the problems its resident windows are fed from -- a window itself
cannot be exported without a device), the C3 bench shape with double and float-valued pixels, a fixed first pose with duplicate
observations, the shuffled large window of tests/test_window_host.py.  Every case in three fresh processes: default, SSX_BA_HOST_PREP=1,
SSX_BA_HOST_LISTS=1 (the host reference paths)."""
import ctypes as C, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CASES = [dict(P=10, L=4000, seed=1), dict(P=10, L=700, seed=41), dict(P=4, L=60, obs_per_lm=4, seed=44), dict(P=7, L=300, obs_per_lm=2, seed=45),
         dict(P=10, L=500, seed=46, fix_first_pose=True, frac_fixed=0.3), dict(P=2, L=40, obs_per_lm=2, seed=47), dict(P=9, L=900, seed=48, fix_first_pose=True),
         dict(P=40, L=1500, obs_per_lm=5, seed=9, loop=False, fix_first_pose=True), dict(P=30, L=1500, obs_per_lm=5, seed=51, fix_first_pose=True),
         dict(P=120, L=4000, obs_per_lm=6, seed=52, fix_first_pose=True), dict(P=500, L=12000, obs_per_lm=6, seed=43, loop=True, fix_first_pose=True),
         dict(P=14, L=1800, obs_per_lm=5, seed=300, pose_t_noise=0.05), dict(P=14, L=1800, obs_per_lm=5, seed=301, pose_t_noise=0.05),
         dict(P=14, L=1800, obs_per_lm=5, seed=302, pose_t_noise=0.05),
         dict(P=10, L=4000, seed=1, uv_f32=True), dict(P=3, L=1, obs_per_lm=3, seed=1),
         dict(P=10, L=600, seed=49, fix_first_pose=True, dup=True), dict(P=30, L=1200, obs_per_lm=5, seed=28, fix_first_pose=True, dup=True),
         dict(P=40, L=14000, obs_per_lm=5, seed=3, loop=True, fix_first_pose=True, shuffle=True)]
MODES = {"default": {}, "host_prep": {"SSX_BA_HOST_PREP": "1"}, "host_lists": {"SSX_BA_HOST_LISTS": "1"}}


def problem(kw):
    from tools.synth import make_ba_problem
    kw = dict(kw)
    dup, shuffle = kw.pop("dup", False), kw.pop("shuffle", False)
    pr = make_ba_problem(**kw)
    cols = [k for k in ("edge_pose", "edge_point", "edge_uv", "edge_cam") if pr.get(k) is not None]
    if dup:                                       # every seventh observation a second time, away from its twin
        again = np.arange(0, pr["E"], 7)
        for k in cols:
            pr[k] = np.ascontiguousarray(np.concatenate([pr[k], pr[k][again][::-1]]))
        pr["E"] = int(pr["edge_pose"].shape[0])
    if shuffle:
        order = np.random.default_rng(0).permutation(pr["E"])
        for k in cols:
            pr[k] = np.ascontiguousarray(pr[k][order])
    return pr


if sys.argv[1] == "--compare":
    a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k) or a.get(k) == "0" * 16]   # (0: prepare() failed)
    print("digests", len(a), "different", bad)
    sys.exit(1 if bad or not a else 0)
if sys.argv[1] == "--one":                        # child: one mode, every case (the switches are read once per process)
    from ssvio_amd import _lib, ba
    lib = _lib.load()
    lib.ssx_ba_debug_prepare_digest.restype = C.c_uint64
    out = {}
    for i, kw in enumerate(CASES):
        keep = []
        st = ba._problem_struct(problem(kw), keep)
        lib.ssx_ba_debug_prepare_digest.argtypes = [C.POINTER(type(st)), C.c_int32]
        for threads in ((1, 4) if kw.get("shuffle") or kw["P"] == 500 else (0,)):
            out[f"{sys.argv[2]}/{i}/t{threads}"] = "%016x" % lib.ssx_ba_debug_prepare_digest(C.byref(st), threads)
    print(json.dumps(out))
    sys.exit(0)
res = {}
for mode, env in MODES.items():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode], env={**os.environ, **env}, capture_output=True, text=True, check=True)
    res.update(json.loads(r.stdout.strip().splitlines()[-1]))
json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
print("digests", len(res), "zero", sum(v == "0" * 16 for v in res.values()))
