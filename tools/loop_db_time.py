"""DetectLoop / MatchFeatures on the device-resident keyframe database against the host way of doing the same.

    python tools/loop_db_time.py [--sizes 500,2000,8000] [--words 1000] [--word-range 20000] [--reps 30] [--warmup 5] [--out FILE]

detect: ssx_kfdb_detect_loop end to end (upload of the query, k_kfdb_score, download of the winner; wall clock around the C call)
        against a loop over ssx_bow_score_l1, one call per stored keyframe on one core, with the float arg-max beside it.  Both
        sides are called through ctypes with their pointers prepared beforehand; the cost of N empty calls is measured too and
        reported as "call overhead", so that the host scan can also be read net of it.
match:  ssx_kfdb_match_features (current descriptors up, k_bf_match on the resident loop descriptors, k_kfdb_pairs, pairs down)
        against ssx_bf_match (both descriptor sets up, matches down) plus the screen and the set on the host.
Every figure is the median of --reps runs after --warmup runs; the minimum is given beside it."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ssvio_amd  # noqa: E402
from ssvio_amd import _lib, loop, orb  # noqa: E402
from ssvio_amd._lib import dbl_p, i32_p, u8_p  # noqa: E402


def make_bow(rng, n, word_range):
    ids = np.sort(rng.choice(word_range, n, replace=False)).astype(np.int32)
    vals = rng.random(n) + 0.05
    return ids, vals / vals.sum()


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6, float(np.min(t)) * 1e6


def detect_row(ctx, n, words, word_range, reps, warmup):
    rng = np.random.default_rng(n)
    lib = ctx.lib
    lib.ssx_bow_score_l1.restype = C.c_double
    lib.ssx_bow_score_l1.argtypes = [C.c_int32, i32_p, dbl_p, C.c_int32, i32_p, dbl_p]
    rows = [make_bow(rng, int(rng.integers(words * 8 // 10, words * 12 // 10)), word_range) for _ in range(n)]
    q = make_bow(rng, words, word_range)
    db = loop.KeyframeDatabase(ctx, keyframes_hint=n)
    for i, r in enumerate(rows):
        db.add(i, r)
    qi, qv = q[0].ctypes.data_as(i32_p), q[1].ctypes.data_as(dbl_p)
    args = [(len(r[0]), r[0].ctypes.data_as(i32_p), r[1].ctypes.data_as(dbl_p)) for r in rows]
    score = lib.ssx_bow_score_l1
    host = {}

    def host_scan():
        best = 0.0
        for m, pi, pv in args:
            s = score(len(q[0]), qi, qv, m, pi, pv)
            if s > best:                                      # (compared as doubles here: the narrowing is not what is timed)
                best = s
        host["best"] = best

    def empty_calls():
        for m, pi, pv in args:
            score(0, qi, qv, 0, pi, pv)

    found, best, sc, ns = C.c_int32(), C.c_int64(), C.c_float(), C.c_int32()

    def device_query():
        st = lib.ssx_kfdb_detect_loop(db.handle, n + 100, len(q[0]), qi, qv, 20, 0.0, C.byref(found), C.byref(best), C.byref(sc), 0, None, C.byref(ns))
        assert st == 0

    t_host = timed(host_scan, max(3, reps // 5), 1)
    t_empty = timed(empty_calls, max(3, reps // 5), 1)
    t_dev = timed(device_query, reps, warmup)
    assert found.value and sc.value == np.float32(host["best"]) and ns.value == n, (sc.value, host["best"])
    _lib.profile_begin(ctx)
    for _ in range(reps):
        device_query()
    prof = _lib.profile_end(ctx)
    calls, ms = prof["k_kfdb_score"]
    db.close()
    return dict(n=n, host=t_host, empty=t_empty, dev=t_dev, kernel=ms * 1e3 / calls)


def match_row(ctx, n_desc, reps, warmup):
    rng = np.random.default_rng(7)
    cur = rng.integers(0, 256, (n_desc, 32), dtype=np.uint8)
    loop_desc = cur[rng.permutation(n_desc)].copy()
    flips = rng.integers(0, 256, n_desc)
    loop_desc[np.arange(n_desc), flips >> 3] ^= (1 << (flips & 7)).astype(np.uint8)     # one flipped bit each, two thirds of them;
    loop_desc[::3] = rng.integers(0, 256, (len(loop_desc[::3]), 32), dtype=np.uint8)     # the rest unrelated
    cls_l = rng.integers(0, n_desc // 4, n_desc).astype(np.int32)
    cls_c = rng.integers(0, n_desc // 4, n_desc).astype(np.int32)
    db = loop.KeyframeDatabase(ctx, keyframes_hint=1)
    db.add(0, (np.zeros(0, np.int32), np.zeros(0)), loop_desc, cls_l)
    out = {}

    def host_way():
        idx, dist = orb.bf_match(ctx, loop_desc, cur)
        keep = dist <= max(2 * int(dist.min()), 30)
        out["host"] = np.unique(np.stack([cls_c[idx[keep]], cls_l[keep]], axis=1), axis=0)

    def device_way():
        out["dev"] = db.match_features(0, cur, cls_c)[0]

    t_host = timed(host_way, reps, warmup)
    t_dev = timed(device_way, reps, warmup)
    assert np.array_equal(out["host"], out["dev"])
    _lib.profile_begin(ctx)
    for _ in range(reps):
        device_way()
    prof = _lib.profile_end(ctx)
    db.close()
    return dict(n=n_desc, pairs=len(out["dev"]), host=t_host, dev=t_dev, k_match=prof["kfdb_bf_match"][1] * 1e3 / prof["kfdb_bf_match"][0],
                k_pairs=prof["k_kfdb_pairs"][1] * 1e3 / prof["k_kfdb_pairs"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="500,2000,8000")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--word-range", type=int, default=20000, help="word ids are drawn below this: two keyframes share words^2 / range words")
    ap.add_argument("--match-desc", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = ssvio_amd.Context(0)
    lines = ["# " + " ".join(["python", "tools/loop_db_time.py"] + sys.argv[1:]),
             f"# commit: {a.commit or 'working tree'}; median (min) of {a.reps} runs after {a.warmup} warm-up runs, microseconds, one process",
             f"# keyframes of about {a.words} words, ids below {a.word_range} (about {a.words * a.words // a.word_range} common words per pair)",
             "# detect_loop end to end = query upload + k_kfdb_score + download of the winner; host scan = ssx_bow_score_l1 per stored keyframe, one core",
             f"{'keyframes':>9} {'host scan':>20} {'call overhead':>20} {'device query':>18} {'k_kfdb_score':>12} {'host/device':>11}"]
    for n in [int(s) for s in a.sizes.split(",")]:
        r = detect_row(ctx, n, a.words, a.word_range, a.reps, a.warmup)
        lines.append(f"{r['n']:>9} {r['host'][0]:>11.1f} ({r['host'][1]:>6.1f}) {r['empty'][0]:>11.1f} ({r['empty'][1]:>6.1f}) "
                     f"{r['dev'][0]:>9.1f} ({r['dev'][1]:>6.1f}) {r['kernel']:>12.1f} {r['host'][0] / r['dev'][0]:>10.1f}x")
        print(lines[-1], flush=True)
    m = match_row(ctx, a.match_desc, a.reps, a.warmup)
    lines += ["#", f"# match_features, {m['n']} loop x {m['n']} current descriptors, {m['pairs']} pairs: ssx_kfdb_match_features against ssx_bf_match + numpy screen and unique",
              f"{'descriptors':>11} {'host way':>20} {'device way':>20} {'k_bf_match':>10} {'k_kfdb_pairs':>12}",
              f"{m['n']:>11} {m['host'][0]:>11.1f} ({m['host'][1]:>6.1f}) {m['dev'][0]:>11.1f} ({m['dev'][1]:>6.1f}) {m['k_match']:>10.1f} {m['k_pairs']:>12.1f}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    ctx.close()


if __name__ == "__main__":
    main()
