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


if __name__ == "__main__":
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
