"""Time of ssx_stereo_dense per KITTI-size pair (376 x 1241) on an MI355X, alone on the chip -> profiles/dense/time.txt.

    python tools/dense_time.py [--out profiles/dense/time.txt] [--trace-dir bench_out/dense_trace] [--no-trace]

Two ways, as section 4 of the measuring guide asks:
  * device events around warmed calls on the context's stream (images and maps in device memory, images_on_device = 1), repeated until
    the window is well over 0.1 s -- per pair at D = 64 / 128 and paths = 4 / 8, and for a batch of 16 pairs per call;
  * per kernel from `rocprofv3 --kernel-trace`, in runs of their own (a fresh child process per paths value: this script with --child).
Beside each kernel the bytes it must move, computed from the shapes, and the time those bytes take at the HBM rate of
MI355X_MICROARCH.md (6.29 TB/s measured); a kernel far above that time is bound by latency / issue, not by bandwidth."""
import csv
import glob
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, COLS = 376, 1241
HBM_BYTES_PER_S = 6.29e12
CONFIGS = [(64, 4), (64, 8), (128, 4), (128, 8)]
BATCH = 16


def kernel_bytes(D, paths, pix=ROWS * COLS):
    """name -> (bytes the kernel must move through HBM at least once, bytes of atomic traffic it sends to the L2) for one pair"""
    vol = 2 * D * pix
    return {
        "k_dense_census": (2 * pix + 16 * pix, 0),                       # both images in, both census planes out
        "fill S": (vol, 0),
        "k_dense_paths": (16 * pix + 2 * vol, paths * vol),              # census in; S read and written once if it stayed in cache; one add per direction
        "fill right keys": (4 * pix, 0),
        "k_dense_right": (vol + 8 * pix, 4 * D * pix),                    # S in, the keys read and written; a 4-byte minimum per (pixel, d)
        "k_dense_select": (vol + 4 * pix + 2 * pix, 0),                   # S in, keys in, the map out
    }


def _pair():
    from tools.synth import make_stereo_pair
    L, R, _ = make_stereo_pair(seed=1)
    assert L.shape == (ROWS, COLS)
    return L, R


def _setup(n):
    import torch

    import ssvio_amd
    from ssvio_amd import dense as dn
    L, R = _pair()
    ctx = ssvio_amd.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    Ld = [torch.from_numpy(L).cuda() for _ in range(n)]
    Rd = [torch.from_numpy(R).cuda() for _ in range(n)]
    out = [torch.empty((ROWS, COLS), dtype=torch.int16, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    jobs = [(Ld[k].data_ptr(), COLS, Rd[k].data_ptr(), COLS, out[k].data_ptr(), COLS) for k in range(n)]
    return torch, dn, ctx, jobs, (Ld, Rd, out)


def child(paths):
    """the run that goes under rocprofv3: per D three warm calls, then 20 of one pair each"""
    torch, dn, ctx, jobs, keep = _setup(1)
    for D in (64, 128):
        prm = dn.DenseParams(disparities=D, paths=paths)
        for _ in range(23):
            dn.dense_ptrs(ctx, jobs, ROWS, COLS, prm, images_on_device=True)
    ctx.close()


def events(lines):
    torch, dn, ctx, jobs16, keep = _setup(BATCH)
    lines.append("device events around warmed calls, images and maps in device memory (one job table up, one synchronisation per call):")
    for n in (1, BATCH):
        for D, paths in CONFIGS:
            prm = dn.DenseParams(disparities=D, paths=paths)
            jobs = jobs16[:n]
            for _ in range(3):
                dn.dense_ptrs(ctx, jobs, ROWS, COLS, prm, images_on_device=True)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); dn.dense_ptrs(ctx, jobs, ROWS, COLS, prm, images_on_device=True); b.record(); torch.cuda.synchronize()
            reps = max(10, int(np.ceil(300.0 / max(a.elapsed_time(b), 1e-3))))
            reps = min(reps, 400)
            windows = []
            for _ in range(3):
                a.record()
                for _ in range(reps):
                    dn.dense_ptrs(ctx, jobs, ROWS, COLS, prm, images_on_device=True)
                b.record(); torch.cuda.synchronize()
                windows.append(a.elapsed_time(b))
            st = dn.last_call(ctx)
            per = [w / reps for w in windows]
            lines.append("  n = %2d  D = %3d  paths = %d   %8.3f ms per call [%.3f - %.3f over 3 windows of %d calls, %.0f ms each]  %8.3f ms per pair   %d groups, %d launches"
                         % (n, D, paths, np.median(per), min(per), max(per), reps, np.median(windows), np.median(per) / n, st["groups"], st["launches"]))
    ctx.close()


def trace(lines, trace_dir):
    lines.append("")
    lines.append("per kernel from rocprofv3 --kernel-trace (a run of its own per paths value; 20 calls of one pair after 3 warm ones): median [p10 - p90];")
    lines.append("beside it the bytes the kernel must move through HBM, the time they take at %.2f TB/s, and the atomic traffic it sends to the L2" % (HBM_BYTES_PER_S / 1e12))
    for paths in (4, 8):
        d = os.path.join(trace_dir, "paths%d" % paths)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", str(paths)],
                           capture_output=True, text=True, timeout=900)
        files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        if r.returncode != 0 or not files:
            lines.append("  paths = %d: rocprofv3 run failed (rc %d): not measured\n%s" % (paths, r.returncode, r.stderr[-600:]))
            continue
        rows = list(csv.DictReader(open(files[-1])))
        rows.sort(key=lambda q: int(q["Start_Timestamp"]))
        # a call's kernels in stream order: census, fill S, paths, fill keys, right, select; D = 64 first (23 calls), then D = 128
        per = {}
        order = ["k_dense_census", "fill S", "k_dense_paths", "fill right keys", "k_dense_right", "k_dense_select"]
        seq = []
        for q in rows:
            name = q["Kernel_Name"]
            m = re.search(r"k_dense_\w+", name)
            us = (int(q["End_Timestamp"]) - int(q["Start_Timestamp"])) / 1e3
            if m:
                seq.append((m.group(0), us))
            elif "fill" in name.lower() or "memset" in name.lower():
                seq.append(("fill", us))
        calls, cur = [], None
        for name, us in seq:
            if name == "k_dense_census":
                cur = {}
                calls.append(cur)
            if cur is None:
                continue
            if name == "fill":
                name = "fill S" if "k_dense_paths" not in cur else "fill right keys"
            cur[name] = cur.get(name, 0.0) + us
        for D, block in ((64, calls[3:23]), (128, calls[26:46])):
            kb = kernel_bytes(D, paths)
            lines.append("  D = %3d  paths = %d   (%d calls)" % (D, paths, len(block)))
            total = 0.0
            for name in order:
                v = np.array([c[name] for c in block if name in c])
                if v.size == 0:
                    lines.append("    %-16s not in the trace" % name)
                    continue
                must, atom = kb[name]
                t_hbm = must / HBM_BYTES_PER_S * 1e6
                med = float(np.median(v))
                total += med
                kind = "bandwidth-bound" if med < 3 * t_hbm else "latency / issue-bound (%.0fx the time of its bytes)" % (med / t_hbm)
                lines.append("    %-16s %9.1f us [%8.1f - %8.1f]   must move %6.1f MB = %6.1f us at the HBM rate%s   %s"
                             % (name, med, np.percentile(v, 10), np.percentile(v, 90), must / 1e6, t_hbm, ("; %6.1f MB of atomics to the L2" % (atom / 1e6)) if atom else "", kind))
            lines.append("    %-16s %9.1f us" % ("sum of medians", total))


# ---- the speckle filter and the samples -> profiles/dense_post/time.txt ----
#     python tools/dense_time.py --post [--parent-lib <libssx.so of the parent commit>] [--out profiles/dense_post/time.txt]
# Each library is timed in fresh child processes of its own (this script with --post-child, the library named by SSX_LIB), parent and new
# alternating, three children each: device events around warmed calls on one KITTI-size pair in device memory, and for the new library
# the per-kernel times of the library's own profiler (HIP events around every launch: ssx_profile_begin / _end).
POST_CONFIGS = [(64, 4), (128, 8)]
POST_KERNELS = ["k_dense_label_tile", "k_dense_label_merge", "k_dense_label_count", "k_dense_speckle", "k_dense_sample_rows", "k_dense_sample_write"]


def post_child():
    import json

    from ssvio_amd import _lib
    from tools import synth
    torch, dn, ctx, jobs, keep = _setup(1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        for _ in range(3):
            fn()
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        reps = min(max(10, int(np.ceil(300.0 / max(a.elapsed_time(b), 1e-3)))), 400)
        per = []
        for _ in range(3):
            a.record()
            for _ in range(reps):
                fn()
            b.record(); torch.cuda.synchronize()
            per.append(a.elapsed_time(b) / reps)
        return [float(np.median(per)), min(per), max(per), reps]

    res = {}
    has_post = hasattr(ctx.lib, "ssx_stereo_dense_post")
    # ssx_stereo_dense bound here, the same way for both libraries: the parent's has none of the new symbols that ssvio_amd.dense binds
    import ctypes as C
    plain = ctx.lib.ssx_stereo_dense
    plain.restype = C.c_int
    plain.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_lib.DenseJob), C.c_int32, C.c_int32, C.POINTER(_lib.DenseParamsC), C.c_int32]
    arr = (_lib.DenseJob * 1)(_lib.DenseJob(*jobs[0]))
    for D, paths in POST_CONFIGS:
        prm = dn.DenseParams(disparities=D, paths=paths)
        res["ssx_stereo_dense %d %d" % (D, paths)] = timed(lambda: ctx.check(plain(ctx.handle, 1, arr, ROWS, COLS, C.byref(prm), 1)))
        if not has_post:
            continue
        bar = dn.min_disp16(synth.KITTI_BF, 40.0)
        posts = {"everything off": dn.DensePost(), "filter 100 / 16": dn.DensePost(100, 16), "filter + samples (stride 4)": dn.DensePost(100, 16, 4, bar),
                 "samples only, no map asked for": dn.DensePost(0, 16, 4, bar)}
        for name, post in posts.items():
            buf = dn.samples_buffers(1, ROWS, COLS, post, device="cuda")[0] if post.cloud_stride > 0 else None
            clouds = [(buf.data_ptr(), dn.sample_capacity(ROWS, COLS, post))] if buf is not None else None
            jb = [(l, ls, r, rs, None, 0) for l, ls, r, rs, _, _ in jobs] if name.startswith("samples only") else jobs
            res["ssx_stereo_dense_post %d %d %s" % (D, paths, name)] = timed(lambda: dn.dense_post_ptrs(ctx, jb, clouds, ROWS, COLS, prm, post, images_on_device=True))
            if name.startswith("filter + samples"):
                _lib.profile_begin(ctx)
                for _ in range(20):
                    counts = dn.dense_post_ptrs(ctx, jb, clouds, ROWS, COLS, prm, post, images_on_device=True)
                t = _lib.profile_end(ctx)
                res["kernels %d %d" % (D, paths)] = {k: [t[k][0], 1e3 * t[k][1] / max(t[k][0], 1)] for k in t if k.startswith("k_dense")}
                res["samples %d %d" % (D, paths)] = counts[0]
    ctx.close()
    print("POSTJSON " + json.dumps(res))


def post(out, parent_lib):
    import json
    new_lib = os.path.join(ROOT, "ssvio_amd", "libssx.so")
    runs = {"parent": [], "new": []}
    for _ in range(3):
        for who, lib in (("parent", parent_lib), ("new", new_lib)):
            if not lib:
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--post-child"], capture_output=True, text=True, timeout=600, env=dict(os.environ, SSX_LIB=lib))
            line = [l for l in r.stdout.splitlines() if l.startswith("POSTJSON ")]
            if r.returncode != 0 or not line:
                raise SystemExit("the %s child failed (rc %d):\n%s" % (who, r.returncode, (r.stdout + r.stderr)[-2000:]))
            runs[who].append(json.loads(line[0][9:]))
    lines = ["ssx_stereo_dense_post at %d x %d (tools/dense_time.py --post), alone on one MI355X: one pair, images, map and samples in device memory" % (ROWS, COLS),
             "ms per call, median [min - max] over 3 fresh processes per library (parent and new alternating), each the median of 3 windows of ~0.3 s of warmed calls"]

    def spread(who, key):
        v = [r[key][0] for r in runs[who] if key in r]
        return "%8.3f [%.3f - %.3f]" % (np.median(v), min(v), max(v)) if v else "   not measured"

    for D, paths in POST_CONFIGS:
        lines.append("  D = %3d  paths = %d" % (D, paths))
        key = "ssx_stereo_dense %d %d" % (D, paths)
        lines.append("    %-52s %s" % ("ssx_stereo_dense, parent commit's library", spread("parent", key)))
        lines.append("    %-52s %s" % ("ssx_stereo_dense, this library", spread("new", key)))
        for name in ("everything off", "filter 100 / 16", "filter + samples (stride 4)", "samples only, no map asked for"):
            lines.append("    %-52s %s" % ("ssx_stereo_dense_post, " + name, spread("new", "ssx_stereo_dense_post %d %d %s" % (D, paths, name))))
        lines.append("    per kernel (the library's profiler: HIP events around each launch, 20 calls with filter + samples; %d samples a call), us a launch:" % runs["new"][0]["samples %d %d" % (D, paths)])
        for k in ["k_dense_census", "k_dense_paths", "k_dense_right", "k_dense_select"] + POST_KERNELS:
            v = [r["kernels %d %d" % (D, paths)][k][1] for r in runs["new"] if k in r["kernels %d %d" % (D, paths)]]
            if v:
                lines.append("      %-24s %8.1f [%.1f - %.1f]" % (k, np.median(v), min(v), max(v)))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if "--post-child" in sys.argv:
        post_child()
        sys.exit(0)
    if "--post" in sys.argv:
        post(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "dense_post", "time.txt"),
             sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None)
        sys.exit(0)
    if "--child" in sys.argv:
        child(int(sys.argv[sys.argv.index("--child") + 1]))
        sys.exit(0)
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "dense", "time.txt")
    trace_dir = sys.argv[sys.argv.index("--trace-dir") + 1] if "--trace-dir" in sys.argv else os.path.join(ROOT, "bench_out", "dense_trace")
    lines = ["ssx_stereo_dense at %d x %d (tools/dense_time.py), alone on one MI355X" % (ROWS, COLS)]
    events(lines)
    if "--no-trace" not in sys.argv:
        trace(lines, trace_dir)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
