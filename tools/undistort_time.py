"""Time of ssx_undistort on the MI355X -> profiles/undistort/time.txt.

Every figure is a host clock around a call that ends in the call's own stream synchronisation, taken warm (the first calls load the
kernel and size the staging), the two forms of a comparison alternating, as median [p10 - p90] over the rounds.  The kernel's own time
is from device events (ssx_profile_begin / _end) in a run of its own, on images in DEVICE memory, beside the bytes the kernel must move
(rows * cols read + rows * cols written per job) at the HBM rate a streaming copy reaches on this part (6.29 TB/s).  A pair is 0.9 MB
and 64 pairs are 60 MB -- both live in the 256 MiB Infinity Cache once warm -- so the last row uses 1024 jobs with buffers of their own
(0.96 GB), which do not.

    python tools/undistort_time.py [--rounds 200] [--out profiles/undistort/time.txt]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS, COLS = 376, 1241
HBM_BYTES_PER_S = 6.29e12          # a float4 streaming copy on the MI355X


def spread(ts):
    a = 1e6 * np.asarray(ts)
    return "%8.1f us [%7.1f - %7.1f]" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def alternate(a, b, rounds, warm=5):
    ta, tb = [], []
    for r in range(warm + rounds):
        t0 = time.perf_counter(); a(); t1 = time.perf_counter(); b(); t2 = time.perf_counter()
        if r >= warm:
            ta.append(t1 - t0); tb.append(t2 - t1)
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort", "time.txt"))
    ap.add_argument("--rounds", type=int, default=200)
    args = ap.parse_args()
    import torch                                                    # device buffers for the kernel-time rows (and one HIP runtime per process)
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
    prm = [ud.make_params(K, d) for d in dists]
    L, R, _ = make_stereo_pair(seed=0)
    assert L.shape == (ROWS, COLS)
    imgs = [np.ascontiguousarray(L), np.ascontiguousarray(R)]
    img_bytes = ROWS * COLS
    lines = ["ssx_undistort at %d x %d, barrel coefficients, left and right different; %d rounds, the two forms of a row alternating; median [p10 - p90]" % (COLS, ROWS, args.rounds)]

    # ---- one pair: host in / host out against pinned buffers read and written in place
    NMAX = 64
    p = lib.ssx_host_alloc(2 * NMAX * img_bytes)
    assert p
    arena = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(2 * NMAX * img_bytes,))
    for k in range(NMAX):
        arena[k * img_bytes:(k + 1) * img_bytes] = imgs[k % 2].reshape(-1)
    pinned_jobs = [(p + k * img_bytes, COLS, p + (NMAX + k) * img_bytes, COLS, prm[k % 2]) for k in range(NMAX)]
    host_out = [np.zeros((ROWS, COLS), np.uint8) for _ in range(NMAX)]
    host_jobs = [(imgs[k % 2].ctypes.data, COLS, host_out[k].ctypes.data, COLS, prm[k % 2]) for k in range(NMAX)]

    def host(n=2):
        ud.undistort_ptrs(ctx, host_jobs[:n], ROWS, COLS, images_on_device=False)

    def pinned(n=2):
        ud.undistort_ptrs(ctx, pinned_jobs[:n], ROWS, COLS, images_on_device=True)

    host(); pinned()
    want = [um.undistort(im, K, d) for im, d in zip(imgs, dists)]
    for k in (0, 1):                                                # the two forms do the same work, and it is the model's
        assert np.array_equal(host_out[k], want[k]) and np.array_equal(arena[(NMAX + k) * img_bytes:(NMAX + k + 1) * img_bytes].reshape(ROWS, COLS), want[k])
    ta, tb = alternate(host, pinned, args.rounds)
    host(); sh = ud.last_call(ctx)
    pinned(); sp = ud.last_call(ctx)
    lines.append("one pair (n = 2)   host in, host out %s  [%d launch, %d synchronisation, %d bytes up, %d down]" % (spread(ta), sh["launches"], sh["syncs"], sh["bytes_up"], sh["bytes_down"]))
    lines.append("one pair (n = 2)   pinned, in place  %s  [%d launch, %d synchronisation, %d bytes up, %d down; the kernel reads and writes the images over PCIe]" %
                 (spread(tb), sp["launches"], sp["syncs"], sp["bytes_up"], sp["bytes_down"]))

    # ---- n jobs in one call against n single calls
    for n in (2, 16, 64):
        rounds = max(20, args.rounds // max(1, n // 4))
        for name, jobs, dev in (("host in, host out", host_jobs, False), ("pinned, in place ", pinned_jobs, True)):
            def one():
                ud.undistort_ptrs(ctx, jobs[:n], ROWS, COLS, images_on_device=dev)

            def singles():
                for j in jobs[:n]:
                    ud.undistort_ptrs(ctx, [j], ROWS, COLS, images_on_device=dev)

            ta, tb = alternate(one, singles, rounds)
            lines.append("n = %2d  %s  one call %s   %2d single calls %s" % (n, name, spread(ta), n, spread(tb)))

    # ---- the kernel's own time: device events, images in device memory, a run of its own
    lines.append("k_undistort from device events (images in device memory; bytes = 2 * rows * cols * n; bound = bytes at %.2f TB/s):" % (HBM_BYTES_PER_S / 1e12))
    for n, reps in ((2, 200), (16, 100), (64, 50), (1024, 10)):
        src = torch.empty(n * img_bytes, dtype=torch.uint8, device="cuda:0")
        dst = torch.zeros(n * img_bytes, dtype=torch.uint8, device="cuda:0")
        pair = torch.from_numpy(np.concatenate([imgs[0].reshape(-1), imgs[1].reshape(-1)])).to("cuda:0")
        src.view(-1, 2 * img_bytes)[:] = pair
        torch.cuda.synchronize()
        jobs = [(src.data_ptr() + k * img_bytes, COLS, dst.data_ptr() + k * img_bytes, COLS, prm[k % 2]) for k in range(n)]
        for _ in range(3):
            ud.undistort_ptrs(ctx, jobs, ROWS, COLS, images_on_device=True)
        got = dst[:2 * img_bytes].cpu().numpy().reshape(2, ROWS, COLS)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        per_call = []
        for _ in range(reps):
            _lib.profile_begin(ctx)
            ud.undistort_ptrs(ctx, jobs, ROWS, COLS, images_on_device=True)
            per_call.append(1e-3 * _lib.profile_end(ctx)["k_undistort"][1])
        byts = 2 * img_bytes * n
        med = float(np.median(per_call))
        lines.append("  n = %4d  %s   %11d bytes  bound %8.1f us  -> %5.1f %% of the bound's rate, %6.1f GB/s, %5.2f ps per pixel" %
                     (n, spread(per_call), byts, 1e6 * byts / HBM_BYTES_PER_S, 100 * (byts / HBM_BYTES_PER_S) / med, byts / med / 1e9, 1e12 * med / (img_bytes * n)))
        del src, dst
        share = (byts / HBM_BYTES_PER_S) / med
    # (the last row is the one past the Infinity Cache)
    lines.append("the kernel is %s the memory bound: %.0f %% of it at n = 1024.  It issues about 62 f64 instructions per pixel (the map inline) and as many "
                 "integer / branch instructions for the four tested taps: %.1f T f64 lane-instructions/s of the 36.5 T/s tools/microbench/f64_rate.hip measures." %
                 ("within sight of" if share > 0.5 else "NOT within sight of", 100 * share, 62 * img_bytes * n / med / 1e12))
    lib.ssx_host_free(p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
