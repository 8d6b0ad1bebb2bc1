"""Undistort host side A/B: two builds of the library must write the same bytes and report the same counters.

    SSX_LIB=<library> python tools/undistort_host_ab.py out.json   digests of one library's outputs (GPU; a fresh process per library)
    python tools/undistort_host_ab.py --compare a.json b.json      exit 1 unless every entry is equal
    python tools/undistort_host_ab.py --times LABEL=FILE ...       (no GPU) the whole-call rows of tools/undistort_time.py (one pair: host in /
        host out, pinned in place) and tools/undistort_plan_time.py (the arena rows) outputs, FILEs of the same label being runs of one
        library: every run, min / median / max per row, and where the second label's median lies in the first's min-max (exit 1 if above)

The device code of two commits is compared by tools/po_host_ab.py --asm, which takes the assembly of any file.

Recorded (sha256 of the bytes of every output image and stored map, and the last_call counters as they are):
  every case of tests/undistort_call_cases.py that a GPU realises, through its real entry point;
  CASES of tests/test_undistort_gpu.py through ssx_undistort, MAPS of tests/test_undistort_plan_gpu.py through a plan (map and image)."""
import hashlib
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sha(*arrays):
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def outputs():
    import numpy as np
    import ssvio_amd
    import test_undistort_gpu as tg
    import test_undistort_plan_gpu as tp
    import undistort_call_cases as cc
    from ssvio_amd import undistort as ud
    out = {}
    with ssvio_amd.Context(0) as ctx:
        imgs = [tg._image(cc.ROWS, cc.COLS, 30 + k) for k in range(8)]
        sets = [((38.0, 41.0, 30.2, 20.7), (-0.28, 0.07, 0.004, -0.003, 0.01)), ((39.0, 40.0, 31.0, 21.5), (0.2, -0.05, -0.002, 0.003, 0.0))]
        prms = [ud.make_params(*s) for s in sets]
        with ud.UndistortPlan(ctx, cc.ROWS, cc.COLS) as plan:
            assert [plan.add(p) for p in prms] == [0, 1]
            for name, case in cc.CASES.items():
                if case["gpu"]:
                    outs, stats, _ = cc.run(ctx, plan, case, imgs, prms)
                    out[f"case/{name}"] = dict(images=sha(*outs), **stats)
        for name, (rows, cols, K, dist, ss, ds, rotated) in tg.CASES.items():
            got = ud.undistort(ctx, [tg._image(rows, cols, 11, ss)], [ud.make_params(K, dist, tg._iR(K, rotated))], dst_stride=ds)
            out[f"inline/{name}"] = dict(images=sha(*got), **ud.last_call(ctx))
        for name, (rows, cols, K, dist, kind) in tp.MAPS.items():
            with ud.UndistortPlan(ctx, rows, cols) as plan:
                m = plan.add(ud.make_params(K, dist, tp._iR(K, kind)))
                added = plan.last_call()
                stored = sha(*plan.packed_map(m))
                got = plan.apply([tp._image(rows, cols, 11)], [m])
                out[f"stored/{name}"] = dict(map=stored, images=sha(*got), add=added, **plan.last_call())
    return out


# ---- --times ---------------------------------------------------------------------------------------------------------------------
def time_figures(path):
    """{row: microseconds (the row's median)} of a tools/undistort_time.py or a tools/undistort_plan_time.py output"""
    out = {}
    for line in open(path):
        m = re.match(r"one pair \(n = 2\)\s+(host in, host out|pinned, in place)\s+([\d.]+) us", line)
        if m:
            out[f"ssx_undistort one pair, {m.group(1)}"] = float(m.group(2))
        m = re.match(r"\s+n = +(\d+)\s+ssx_undistort, in place over PCIe\s+([\d.]+) us \[[^\]]*\]\s+ssx_undistort_plan_apply\s+([\d.]+) us", line)
        if m:
            out[f"ssx_undistort arena in place n = {int(m.group(1)):3d}"] = float(m.group(2))
            out[f"ssx_undistort_plan_apply arena n = {int(m.group(1)):3d}"] = float(m.group(3))
    return out


def times(args):
    runs, bad = {}, 0
    for a in args:
        label, path = a.split("=", 1)
        figures = time_figures(path)
        if figures:
            print(f"{label} {os.path.basename(path)}: " + "; ".join(f"{k} {v:.1f} us" for k, v in figures.items()))
        for k, v in figures.items():
            runs.setdefault(k, {}).setdefault(label, []).append(v)
    for k, by in runs.items():
        (la, va), (lb, vb) = list(by.items())[:2]
        med = statistics.median(vb)
        where = "ABOVE" if med > max(va) else "below (faster than)" if med < min(va) else "inside"
        bad += med > max(va)
        f = lambda l, v: f"{l} min {min(v):.1f} median {statistics.median(v):.1f} max {max(v):.1f} ({len(v)} runs)"      # noqa: E731
        print(f"{k:44s} {f(la, va)} | {f(lb, vb)} | {lb} median {where} {la}'s min-max")
    return bad or not runs


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        a, b = json.load(open(sys.argv[2])), json.load(open(sys.argv[3]))
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        for g in sorted({k.split("/")[0] for k in a}):
            print(f"{g:8s} {sum(k.startswith(g + '/') for k in a):4d} entries, different: {[k for k in bad if k.startswith(g + '/')]}")
        print("entries", len(a), "|", len(b), "different", len(bad))
        sys.exit(1 if bad or not a else 0)
    if sys.argv[1] == "--times":
        sys.exit(1 if times(sys.argv[2:]) else 0)
    res = outputs()
    json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
    print("entries", len(res), "library", os.environ.get("SSX_LIB") or "ssvio_amd/libssx.so")
