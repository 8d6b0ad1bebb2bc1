"""The candidate query of relocalisation for S lost frames: one ssx_kfdb_relocalize_query_batch call of S jobs against S calls of
ssx_kfdb_relocalize_query on S databases.

    python tools/reloc_batch_time.py [--streams 1,8,32] [--features 200] [--stored 100] [--candidates 4] [--reps 30] [--warmup 5] [--out FILE]

A KITTI-sized synthetic image (1241 x 376), --features features x 8 levels, a synthetic vocabulary of 10 000 words, databases of --stored
keyframes (the image's own keyframe under id 0, the others of about 1000 random words that share some with the query), K = --candidates,
threshold 0 and ratio 0 so that every job has K candidates to match.  Nothing is committed, so every repetition sees the same databases.
The single calls run on one context and the batch call on another, each with its own copy of the vocabulary and its own databases, so
that neither re-plans the other's ORB workspace; both are called through ctypes with their arrays prepared beforehand.  Host clock around
calls that end in their synchronisation; per S the two alternate in the same process, --reps repetitions after --warmup; median,
quartiles and extremes in microseconds."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ssvio_amd  # noqa: E402
from ssvio_amd import loop, orb, voc as svoc  # noqa: E402
from ssvio_amd._lib import KP_DTYPE, i32_p, u8_p  # noqa: E402
from tools.loop_batch_time import LEVELS, fill, spread  # noqa: E402
from tools.synth import make_stereo_pair, make_vocabulary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,32")
    ap.add_argument("--features", type=int, default=200)
    ap.add_argument("--stored", type=int, default=100)
    ap.add_argument("--candidates", type=int, default=4)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    Ss, K = [int(s) for s in a.streams.split(",")], a.candidates
    voc = make_vocabulary(k=10, L=4)
    img = np.ascontiguousarray(make_stereo_pair(seed=0)[0])
    side = {}
    for name in ("single", "batch"):
        ctx = ssvio_amd.Context(0)
        V = svoc.Vocabulary.from_arrays(ctx, 10, 4, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
        ex = orb.ORBextractor(ctx, nfeatures=a.features)
        side[name] = dict(ctx=ctx, V=V, ex=ex)
    ex = side["single"]["ex"]
    feats = np.ascontiguousarray(ex.Detect(img), dtype=KP_DTYPE)
    pyr = np.repeat(feats, LEVELS)
    pyr["octave"] = np.tile(np.arange(LEVELS, dtype=np.int32), len(feats)); pyr["response"] = -1.0
    pyr["class_id"] = np.repeat(np.arange(len(feats), dtype=np.int32), LEVELS)
    kps, desc = ex.ScreenAndComputeKPsParams_CalcDescriptors(img, pyr)
    own = dict(bow=side["single"]["V"].transform(desc), desc=desc, cls=np.ascontiguousarray(kps["class_id"]))
    for name in side:
        side[name]["dbs"] = [fill(side[name]["ctx"], a.stored, own, side[name]["V"].n_words, np.random.default_rng(1)) for _ in range(max(Ss))]
    lib = side["single"]["ctx"].lib
    loop._bind(lib)
    n_in, cap = len(pyr), len(own["cls"])
    lines = ["# " + " ".join(["python", "tools/reloc_batch_time.py"] + sys.argv[1:]),
             f"# commit: {a.commit or 'working tree'}; image {img.shape[1]}x{img.shape[0]}, {len(feats)} features x {LEVELS} levels = {n_in} pyramid keypoints, "
             f"{len(own['cls'])} survive, {len(own['bow'][0])} words; databases of {a.stored} keyframes, K = {K}, threshold 0, ratio 0",
             f"# microseconds per S queries: median [quartiles] (min .. max) of {a.reps} repetitions after {a.warmup}, the two alternating in one process",
             "# single = S calls of ssx_kfdb_relocalize_query on S databases; batch = one ssx_kfdb_relocalize_query_batch of S jobs; launches / syncs: ssx_kfdb_debug_last_batch",
             f"{'S':>3} {'single':>44} {'batch':>44} {'single/batch':>12} {'launches':>8} {'syncs':>5}"]
    fmt = lambda s: f"{s['med']:>9.1f} [{s['q1']:>8.1f} {s['q3']:>8.1f}] ({s['lo']:>8.1f} .. {s['hi']:>8.1f})"
    results = {}
    for S in Ss:
        sd, bd = side["single"], side["batch"]
        res = loop.RelocQueryResult()
        o_pairs = np.zeros((K, cap, 2), np.int32)

        def single():
            for db in sd["dbs"][:S]:
                assert lib.ssx_kfdb_relocalize_query(db.handle, sd["V"].handle, img.ctypes.data_as(u8_p), img.strides[0], img.shape[0], img.shape[1], C.byref(sd["ex"].prm),
                                                     len(feats), feats.ctypes.data_as(C.c_void_p), LEVELS, K, 0.0, 0.0, cap, o_pairs.ctypes.data_as(i32_p), C.byref(res)) == 0
                assert res.n_candidates == min(K, a.stored) and res.cand[0].kf_id == 0

        table = (loop.RelocQueryJob * S)()
        bres, status = (loop.RelocQueryResult * S)(), (C.c_int32 * S)()
        b_pairs = [np.zeros((K, cap, 2), np.int32) for _ in range(S)]
        for j, db in enumerate(bd["dbs"][:S]):
            table[j] = loop.RelocQueryJob(db.handle, img.ctypes.data, img.strides[0], len(feats), feats.ctypes.data, 0, cap, b_pairs[j].ctypes.data_as(i32_p),
                                          C.pointer(bres[j]), C.cast(C.byref(status, 4 * j), i32_p))

        def batch():
            assert lib.ssx_kfdb_relocalize_query_batch(bd["V"].handle, S, table, img.shape[0], img.shape[1], C.byref(bd["ex"].prm), LEVELS, K, 0.0, 0.0, 0) == 0
            assert all(bres[j].n_candidates == res.n_candidates and bres[j].cand[0].n_pairs == res.cand[0].n_pairs for j in range(S))

        ts, tb = [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter(); single(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
            if rep >= a.warmup:
                ts.append(t1 - t0); tb.append(t2 - t1)
        st = loop.debug_last_batch(bd["ctx"])
        s, b = spread(ts), spread(tb)
        results[S] = (s, b)
        lines.append(f"{S:>3} {fmt(s)} {fmt(b)} {s['med'] / b['med']:>11.2f}x {st['launches']:>8} {st['syncs']:>5}")
        print(lines[-1], flush=True)
    lines.append("#")
    if 1 in results:
        s, b = results[1]
        verdict = "met" if s["q1"] <= b["med"] <= s["q3"] else ("met (below the range: faster)" if b["med"] < s["q1"] else "not met")
        lines.append(f"# condition: at S = 1 the batch call takes {b['med']:.1f} us; the single call's interquartile range is [{s['q1']:.1f}, {s['q3']:.1f}] us "
                     f"around {s['med']:.1f} us: {verdict}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    for sd in side.values():
        for db in sd["dbs"]:
            db.close()
        sd["V"].close(); sd["ctx"].close()


if __name__ == "__main__":
    main()
