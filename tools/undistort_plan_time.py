"""Time of the undistortion plan (ssx_undistort_plan_*) on the MI355X against the inline form (ssx_undistort)
-> profiles/undistort_plan/time.txt.  Nothing here is a bar; the figures decide two choices the code states (whether a thread of
k_undistort_remap loops over the jobs of its map or the cache serves them; whether the batcher applies the plan at all).

Kernel times are device events (ssx_profile_begin / _end) on images in DEVICE memory, the two forms alternating call by call in one
process, warm, as median [p10 - p90].  Whole calls are a host clock around a call that ends in its own stream synchronisation, likewise
alternating.  --system adds the batched runner on a full-size distorted drive (64 streams, preloaded).

    python tools/undistort_plan_time.py [--rounds 100] [--system] [--out profiles/undistort_plan/time.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS, COLS = 376, 1241
MAP_BYTES = 3 * ROWS * ((COLS + 3) // 4 * 4) * 2


def spread(ts):
    a = 1e6 * np.asarray(ts)
    return "%8.1f us [%7.1f - %7.1f]" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def system_rows(lines, frames=24, streams=64):
    """the runner on a full-size drive seen through the lenses of tools/undistort_drive.py: batched with the plan, batched on the
    model's undistorted images with the key 0, and unbatched with the key"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import host_util
    from tools import synth
    from tools import undistort_drive as drv
    from tools import undistort_model as um
    built = host_util.build_test_binaries()
    root = tempfile.mkdtemp()
    seq = host_util.write_sequence(os.path.join(root, "rect"), n_frames=frames, step=0.6)
    K = tuple(float(np.float32(synth.KITTI00_SETTINGS["Camera1." + k])) for k in ("fx", "fy", "cx", "cy"))
    dl, dr = drv.as_read(drv.COEFFS["Camera1"]), drv.as_read(drv.COEFFS["Camera2"])
    dist = [(um.distort_image(L, K, dl), um.distort_image(R, K, dr)) for L, R in seq["frames"]]
    model = [(um.undistort(L, K, dl), um.undistort(R, K, dr)) for L, R in dist]
    dirs = dict(dist=drv._write(os.path.join(root, "dist", "seq"), dist, seq["dt"]), model=drv._write(os.path.join(root, "model", "seq"), model, seq["dt"]))
    on = dict({"Camera.NeedUndistortion": 1}, **drv.coefficient_settings())

    def run(tag, which, overrides, extra):
        cfg = synth.write_settings(os.path.join(root, tag + ".yaml"), overrides)
        r = subprocess.run([built["run_kitti"], "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + dirs[which], "--streams=%d" % streams, "--preload=1", *extra],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(tag + ": " + (r.stdout + r.stderr)[-2000:])
        rate = float(re.search(r"to the last stream's end = ([0-9.]+) frames/s", r.stdout).group(1))
        return rate, [l for l in r.stdout.splitlines() if l.startswith("batched calls:")]

    lines.append("the runner, %d streams x %d frames of %d x %d, preloaded; frames/s from the common start to the last stream's end, three runs each, alternating:" % (streams, frames, COLS, ROWS))
    forms = [("batched, key 1, --undistort_batched=1 (distorted images)", "dist", on, ("--batched=1", "--undistort_batched=1")),
             ("batched, key 0 (the model's undistorted images)       ", "model", {}, ("--batched=1",)),
             ("unbatched --streams, key 1 (distorted images)          ", "dist", on, ())]
    rates = {f[0]: [] for f in forms}
    calls = {}
    for rep in range(3):
        for name, which, ov, extra in forms:
            rate, cl = run("sys%d" % len(calls), which, ov, extra)
            rates[name].append(rate)
            calls[name] = cl
    for name, *_ in forms:
        lines.append("  %s  %s" % (name, "  ".join("%8.1f" % v for v in rates[name])))
        for l in calls[name]:
            lines.append("      " + l)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_plan", "time.txt"))
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--system", action="store_true")
    args = ap.parse_args()
    import torch                                                    # device buffers (and one HIP runtime per process)
    import ssvio_amd
    from ssvio_amd import _lib
    from ssvio_amd import undistort as ud
    from tools import undistort_model as um
    from tools.synth import KITTI00_SETTINGS, make_stereo_pair
    ctx = ssvio_amd.Context(0)                                      # raises without a GPU: no figure is taken anywhere else
    lib = ctx.lib
    lib.ssx_host_alloc.restype = C.c_void_p; lib.ssx_host_alloc.argtypes = [C.c_size_t]
    lib.ssx_host_free.restype = None; lib.ssx_host_free.argtypes = [C.c_void_p]
    K = tuple(float(np.float32(KITTI00_SETTINGS["Camera1." + k])) for k in ("fx", "fy", "cx", "cy"))
    dists = [tuple(float(np.float32(v)) for v in d) + (0.0,) for d in ((-0.20, 0.03, 0.001, -0.0005), (-0.18, 0.02, -0.0008, 0.0004))]
    L, R, _ = make_stereo_pair(seed=0)
    assert L.shape == (ROWS, COLS)
    imgs = [np.ascontiguousarray(L), np.ascontiguousarray(R)]
    want = [um.undistort(im, K, d) for im, d in zip(imgs, dists)]
    img_bytes = ROWS * COLS
    plan = ud.UndistortPlan(ctx, ROWS, COLS)
    # 64 parameter sets: the two cameras, then sets that differ from them in k1 by steps no lens is made to (maps of their own all the same)
    sets = [ud.make_params(K, dists[k % 2] if k < 2 else (dists[k % 2][0] + 1e-4 * (k // 2),) + dists[k % 2][1:]) for k in range(_lib.SSX_UNDISTORT_PLAN_MAX_MAPS)]
    t_map = []
    for prm in sets:
        _lib.profile_begin(ctx)
        plan.add(prm)
        t_map.append(1e-3 * _lib.profile_end(ctx)["k_undistort_map"][1])
    lines = ["the undistortion plan at %d x %d against the inline form; the two forms of a row alternating call by call; median [p10 - p90]" % (COLS, ROWS),
             "k_undistort_map, once per camera: first launch %.1f us, the %d after it %s; a stored map is %d bytes" % (1e6 * t_map[0], len(t_map) - 1, spread(t_map[1:]), MAP_BYTES),
             "kernels from device events, images in device memory (n images in, n out, buffers of their own):"]

    for n, reps in ((2, args.rounds), (64, args.rounds), (128, args.rounds), (256, max(20, args.rounds // 2)), (1024, max(10, args.rounds // 5))):
        src = torch.empty(n * img_bytes, dtype=torch.uint8, device="cuda:0")
        dst = torch.zeros(n * img_bytes, dtype=torch.uint8, device="cuda:0")
        pair = torch.from_numpy(np.concatenate([imgs[0].reshape(-1), imgs[1].reshape(-1)])).to("cuda:0")
        src.view(-1, 2 * img_bytes)[:] = pair
        torch.cuda.synchronize()
        at = [(src.data_ptr() + k * img_bytes, COLS, dst.data_ptr() + k * img_bytes, COLS) for k in range(n)]
        inline = [a + (sets[k % 2],) for k, a in enumerate(at)]
        forms = {"two maps": [a + (k % 2,) for k, a in enumerate(at)]}
        if n > 2:                                                   # a map per job, as far as a plan holds maps
            forms["%d maps" % min(n, len(sets))] = [a + (k % len(sets),) for k, a in enumerate(at)]
        for jobs in forms.values():                                 # warm, and the same bytes as the model
            plan.apply_ptrs(jobs, images_on_device=True)
        got = dst[:2 * img_bytes].cpu().numpy().reshape(2, ROWS, COLS)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        ud.undistort_ptrs(ctx, inline, ROWS, COLS, images_on_device=True)
        t = {name: [] for name in ("inline", *forms)}
        for _ in range(reps):
            _lib.profile_begin(ctx)
            ud.undistort_ptrs(ctx, inline, ROWS, COLS, images_on_device=True)
            t["inline"].append(1e-3 * _lib.profile_end(ctx)["k_undistort"][1])
            for name, jobs in forms.items():
                _lib.profile_begin(ctx)
                plan.apply_ptrs(jobs, images_on_device=True)
                t[name].append(1e-3 * _lib.profile_end(ctx)["k_undistort_remap"][1])
        lines.append("  n = %4d  k_undistort %s   k_undistort_remap, %s" % (n, spread(t["inline"]), ";  ".join("%s %s (x %.2f)" % (name, spread(t[name]), np.median(t["inline"]) / np.median(t[name])) for name in forms)))
        del src, dst
        if n != 128:
            continue
        # the same jobs with the results at a pitch of 1244: every row dword-aligned, no byte stores (at 1241 three rows of four take them)
        pitch = (COLS + 3) // 4 * 4
        src = torch.empty(n * img_bytes, dtype=torch.uint8, device="cuda:0")
        dst = torch.zeros(n * ROWS * pitch, dtype=torch.uint8, device="cuda:0")
        src.view(-1, 2 * img_bytes)[:] = pair
        torch.cuda.synchronize()
        at = [(src.data_ptr() + k * img_bytes, COLS, dst.data_ptr() + k * ROWS * pitch, pitch) for k in range(n)]
        inline, jobs = [a + (sets[k % 2],) for k, a in enumerate(at)], [a + (k % 2,) for k, a in enumerate(at)]
        ta, tb = [], []
        for r in range(3 + reps):
            _lib.profile_begin(ctx)
            ud.undistort_ptrs(ctx, inline, ROWS, COLS, images_on_device=True)
            a = 1e-3 * _lib.profile_end(ctx)["k_undistort"][1]
            _lib.profile_begin(ctx)
            plan.apply_ptrs(jobs, images_on_device=True)
            b = 1e-3 * _lib.profile_end(ctx)["k_undistort_remap"][1]
            if r >= 3:
                ta.append(a); tb.append(b)
        assert np.array_equal(dst[:ROWS * pitch].cpu().numpy().reshape(ROWS, pitch)[:, :COLS], want[0])
        lines.append("  n = %4d  results at a pitch of %d (every row dword-aligned: no byte stores)  k_undistort %s   k_undistort_remap, two maps %s (x %.2f)" %
                     (n, pitch, spread(ta), spread(tb), np.median(ta) / np.median(tb)))
        del src, dst

    # ---- the whole call on a pinned arena: the plan (one copy up, the kernel device to device, one copy down) against ssx_undistort in place
    lines.append("the whole call on an ssx_host_alloc arena (sources in the first n slices, results in the next n), host clock:")
    NMAX = 256
    sl = (img_bytes + 255) & ~255
    p = lib.ssx_host_alloc(2 * NMAX * sl)
    assert p
    arena = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(2 * NMAX * sl,))
    for k in range(NMAX):
        arena[k * sl:k * sl + img_bytes] = imgs[k % 2].reshape(-1)
    for n, reps in ((64, args.rounds), (256, max(20, args.rounds // 4))):
        pj = [(p + k * sl, COLS, p + (n + k) * sl, COLS, k % 2) for k in range(n)]
        ij = [(p + k * sl, COLS, p + (n + k) * sl, COLS, sets[k % 2]) for k in range(n)]
        ta, tb = [], []
        for r in range(3 + reps):
            t0 = time.perf_counter(); ud.undistort_ptrs(ctx, ij, ROWS, COLS, images_on_device=True)
            t1 = time.perf_counter(); plan.apply_ptrs(pj, images_on_device=True); t2 = time.perf_counter()
            if r >= 3:
                ta.append(t1 - t0); tb.append(t2 - t1)
        st = plan.last_call()
        assert np.array_equal(arena[n * sl:n * sl + img_bytes].reshape(ROWS, COLS), want[0])
        lines.append("  n = %3d  ssx_undistort, in place over PCIe %s   ssx_undistort_plan_apply %s (x %.2f)  [%d launch, %d synchronisation, %d copy up of %d bytes, %d down of %d]" %
                     (n, spread(ta), spread(tb), np.median(ta) / np.median(tb), st["launches"], st["syncs"], st["copies_up"], st["bytes_up"], st["copies_down"], st["bytes_down"]))
    lib.ssx_host_free(p)
    plan.close()
    ctx.close()
    if args.system:
        system_rows(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
