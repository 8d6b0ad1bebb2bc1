"""What the lens models cost the radtan path, and what the KB4 lens costs, on the MI355X -> profiles/rectify/time.txt.  Nothing here is a
bar; the figures decide whether ud_map branches on the model or is instantiated per model (csrc/undistort.hip).

Kernel times are device events (ssx_profile_begin / _end) on images in DEVICE memory at 1241 x 376, warm, as median [p10 - p90]:
k_undistort over n = 2 and n = 64 jobs, k_undistort_map over parameter sets new to a plan.  One process measures one library
(SSX_LIB names another build of it); --ab runs the parent's library and this one in child processes, alternating, twice each, so the
parent's own run-to-run spread stands beside the difference.

    python tools/rectify_time.py --ab PARENT_LIBSSX [--rounds 100] [--out profiles/rectify/time.txt]
    python tools/rectify_time.py --one              (the rows of the library SSX_LIB names, or of the tree's)
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS, COLS = 376, 1241


def spread(ts):
    a = 1e6 * np.asarray(ts)
    return "%8.1f us [%7.1f - %7.1f]" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def one(rounds):
    import torch                                                    # device buffers (and one HIP runtime per process)
    import ssvio_amd
    from ssvio_amd import _lib
    from ssvio_amd import undistort as ud
    from tools.synth import KITTI00_SETTINGS, make_stereo_pair
    ctx = ssvio_amd.Context(0)                                      # raises without a GPU: no figure is taken anywhere else
    has_lens = hasattr(ctx.lib, "ssx_undistort_lens")
    K = tuple(float(np.float32(KITTI00_SETTINGS["Camera1." + k])) for k in ("fx", "fy", "cx", "cy"))
    dists = [tuple(float(np.float32(v)) for v in d) + (0.0,) for d in ((-0.20, 0.03, 0.001, -0.0005), (-0.18, 0.02, -0.0008, 0.0004))]
    kbs = [(-0.02, 0.005, -0.001, 0.0002), (0.03, -0.01, 0.002, -0.0003)]
    L, R, _ = make_stereo_pair(seed=0)
    img_bytes = ROWS * COLS
    pair = torch.from_numpy(np.concatenate([np.ascontiguousarray(L).reshape(-1), np.ascontiguousarray(R).reshape(-1)])).to("cuda:0")
    forms = {"radtan": [ud.make_params(K, d) for d in dists]}
    if has_lens:
        forms["radtan through ssx_undistort_lens"] = [ud.make_lens_params(_lib.SSX_LENS_RADTAN, K, d) for d in dists]
        forms["kb4"] = [ud.make_lens_params(_lib.SSX_LENS_KB4, K, k) for k in kbs]
    for n in (2, 64):
        src = torch.empty(n * img_bytes, dtype=torch.uint8, device="cuda:0")
        dst = torch.zeros(n * img_bytes, dtype=torch.uint8, device="cuda:0")
        src.view(-1, 2 * img_bytes)[:] = pair
        torch.cuda.synchronize()
        t = {name: [] for name in forms}
        for r in range(3 + rounds):
            for name, prm in forms.items():                         # the forms alternate call by call
                jobs = [(src.data_ptr() + k * img_bytes, COLS, dst.data_ptr() + k * img_bytes, COLS, prm[k % 2]) for k in range(n)]
                _lib.profile_begin(ctx)
                ud.undistort_ptrs(ctx, jobs, ROWS, COLS, images_on_device=True)
                v = 1e-3 * _lib.profile_end(ctx)["k_undistort"][1]
                if r >= 3:
                    t[name].append(v)
        for name in forms:
            print("ROW k_undistort      n = %2d  %-34s %s" % (n, name, spread(t[name])))
        del src, dst
    # k_undistort_map: every set is new to the plan (k1 moved by steps no lens is made to)
    n_sets = min(rounds, _lib.SSX_UNDISTORT_PLAN_MAX_MAPS // 2)
    with ud.UndistortPlan(ctx, ROWS, COLS) as plan:
        t = {"radtan": [], "kb4": []}
        for k in range(n_sets):
            _lib.profile_begin(ctx)
            plan.add(ud.make_params(K, (dists[0][0] + 1e-4 * k,) + dists[0][1:]))
            v = 1e-3 * _lib.profile_end(ctx)["k_undistort_map"][1]
            if k >= 2:
                t["radtan"].append(v)
            if has_lens:
                _lib.profile_begin(ctx)
                plan.add_lens(ud.make_lens_params(_lib.SSX_LENS_KB4, K, (kbs[0][0] + 1e-4 * k,) + kbs[0][1:]))
                v = 1e-3 * _lib.profile_end(ctx)["k_undistort_map"][1]
                if k >= 2:
                    t["kb4"].append(v)
        for name, ts in t.items():
            if ts:
                print("ROW k_undistort_map          %-34s %s" % (name, spread(ts)))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify", "time.txt"))
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--ab", metavar="PARENT_LIBSSX")
    ap.add_argument("--one", action="store_true")
    args = ap.parse_args()
    if args.one:
        return one(args.rounds)
    if not args.ab or not os.path.exists(args.ab):
        raise SystemExit("--ab names the parent commit's libssx.so")
    lines = ["the lens models at %d x %d: kernel times from device events, images in device memory, %d rounds; median [p10 - p90]." % (COLS, ROWS, args.rounds),
             "Each block is a process of its own; parent and new alternate, twice each: the two parent blocks show the parent's own run-to-run spread."]
    for tag, lib in (("parent, run 1", args.ab), ("new, run 1", None), ("parent, run 2", args.ab), ("new, run 2", None)):
        env = dict(os.environ)
        env.pop("SSX_LIB", None)
        if lib:
            env["SSX_LIB"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--rounds", str(args.rounds)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit(tag + ": " + (r.stdout + r.stderr)[-2000:])
        lines.append(tag + ":")
        lines += ["  " + l[4:] for l in r.stdout.splitlines() if l.startswith("ROW ")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
