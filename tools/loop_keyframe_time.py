"""The per-keyframe step of loop closing: ssx_kfdb_process_keyframe (+ ssx_kfdb_add_pending) against the five calls it replaces.

    python tools/loop_keyframe_time.py [--features 150,500,2000] [--stored 500,2000] [--reps 30] [--warmup 5] [--out FILE]

five calls: ssx_orb_describe_at (the features replicated over the levels beforehand, outside the clock), ssx_voc_transform,
            ssx_kfdb_detect_loop, then ssx_kfdb_match_features when a loop was found, else ssx_kfdb_add: what a caller of the library had to
            issue per keyframe before the step existed.  Five synchronisations; the descriptors come down once and go up three times.
step:       ssx_kfdb_process_keyframe, then ssx_kfdb_add_pending when no loop was found (the reference does not store a keyframe that closed
            a loop, loopclosing.cpp:57-66).
Both are called through ctypes with their arrays prepared beforehand; wall clock around the C calls, median (min) of --reps runs after
--warmup runs.  A KITTI-sized synthetic image, a synthetic vocabulary of 10 000 words, stored keyframes of about --words words; the
loop keyframe is the image itself stored under id 0, and "no loop" is the same database asked with a threshold no score reaches, so
that both verdicts score the same rows.  The kernels are timed by HIP events (ssx_profile_begin / _end) in a run of their own."""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ssvio_amd  # noqa: E402
from ssvio_amd import _lib, loop, orb, voc as svoc  # noqa: E402
from ssvio_amd._lib import KP_DTYPE, dbl_p, i32_p, u8_p  # noqa: E402
from tools.synth import make_stereo_pair, make_vocabulary  # noqa: E402

LEVELS = 8
STEP_KERNELS = ("k_resize", "k_gauss7", "k_orient_brief", "orb_misc", "k_kf_compact", "kf_voc_words", "k_kf_bow", "k_kfdb_score", "kfdb_bf_match",
                "k_kfdb_pairs", "k_kfdb_commit")


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e6, float(np.min(t)) * 1e6


def expand(features):
    out = np.repeat(np.ascontiguousarray(features, dtype=KP_DTYPE), LEVELS)
    out["octave"] = np.tile(np.arange(LEVELS, dtype=np.int32), len(features))
    out["response"] = -1.0
    out["class_id"] = np.repeat(np.arange(len(features), dtype=np.int32), LEVELS)
    return out


def fill(ctx, n_stored, own, words, n_words, rng):
    """the image's own keyframe under id 0, then n_stored - 1 keyframes of about `words` random words and a few descriptors each"""
    db = loop.KeyframeDatabase(ctx, keyframes_hint=n_stored + 128)
    db.add(0, own["bow"], own["desc"], own["cls"])
    for i in range(1, n_stored):
        n = int(rng.integers(words * 8 // 10, words * 12 // 10))
        ids = np.sort(rng.choice(n_words, n, replace=False)).astype(np.int32)
        vals = rng.random(n) + 0.05
        db.add(i, (ids, vals / vals.sum()), own["desc"][:8], own["cls"][:8])
    return db


def case(ctx, V, ex, img, feats, n_stored, words, reps, warmup):
    lib = ctx.lib
    rng = np.random.default_rng(n_stored + len(feats))
    pyr = expand(feats)
    n_in = len(pyr)
    kps, desc = ex.ScreenAndComputeKPsParams_CalcDescriptors(img, pyr)
    own = dict(bow=V.transform(desc), desc=desc, cls=np.ascontiguousarray(kps["class_id"]))
    # the five calls' arrays, allocated once
    o_kps = np.zeros(n_in, KP_DTYPE); o_desc = np.zeros((n_in, 32), np.uint8); o_ids = np.zeros(n_in, np.int32); o_vals = np.zeros(n_in)
    o_pairs = np.zeros((n_in, 2), np.int32)
    n, m, found, best, score, ns, npairs, md = (C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_float(), C.c_int32(), C.c_int32(), C.c_int32())
    res = loop.StepResult()
    prm = C.byref(ex.prm)
    pimg, pfeat, ppyr = img.ctypes.data_as(u8_p), feats.ctypes.data_as(C.c_void_p), pyr.ctypes.data_as(C.c_void_p)
    out = {}
    for verdict, threshold in (("loop", 0.6), ("no loop", 2.0)):
        dbs = {"five": fill(ctx, n_stored, own, words, V.n_words, np.random.default_rng(1)), "step": fill(ctx, n_stored, own, words, V.n_words, np.random.default_rng(1))}
        next_id = {"five": 10 ** 6, "step": 10 ** 6}

        def five():
            db = dbs["five"]
            next_id["five"] += 1
            assert lib.ssx_orb_describe_at(ctx.handle, pimg, img.strides[0], img.shape[0], img.shape[1], prm, ppyr, n_in, o_kps.ctypes.data_as(C.c_void_p),
                                           o_desc.ctypes.data_as(u8_p), C.byref(n)) == 0
            cls = np.ascontiguousarray(o_kps["class_id"][:n.value])
            assert lib.ssx_voc_transform(V.handle, o_desc.ctypes.data_as(u8_p), n.value, None, None, n_in, o_ids.ctypes.data_as(i32_p), o_vals.ctypes.data_as(dbl_p),
                                         C.byref(m)) == 0
            assert lib.ssx_kfdb_detect_loop(db.handle, next_id["five"], m.value, o_ids.ctypes.data_as(i32_p), o_vals.ctypes.data_as(dbl_p), 20, threshold,
                                            C.byref(found), C.byref(best), C.byref(score), 0, None, C.byref(ns)) == 0
            if found.value:
                assert lib.ssx_kfdb_match_features(db.handle, best.value, n.value, o_desc.ctypes.data_as(u8_p), cls.ctypes.data_as(i32_p), n_in,
                                                   o_pairs.ctypes.data_as(i32_p), C.byref(npairs), C.byref(md)) == 0
            else:
                assert lib.ssx_kfdb_add(db.handle, next_id["five"], m.value, o_ids.ctypes.data_as(i32_p), o_vals.ctypes.data_as(dbl_p), n.value,
                                        o_desc.ctypes.data_as(u8_p), cls.ctypes.data_as(i32_p)) == 0

        def step():
            db = dbs["step"]
            next_id["step"] += 1
            assert lib.ssx_kfdb_process_keyframe(db.handle, V.handle, next_id["step"], pimg, img.strides[0], img.shape[0], img.shape[1], prm, len(feats), pfeat, LEVELS,
                                                 50, 20, threshold, n_in, o_pairs.ctypes.data_as(i32_p), C.byref(res)) == 0
            if not res.found:
                assert lib.ssx_kfdb_add_pending(db.handle) == 0

        t_five = timed(five, reps, warmup)
        five_found, five_pairs = found.value, npairs.value
        t_step = timed(step, reps, warmup)
        assert bool(res.found) == bool(five_found) == (verdict == "loop") and (not res.found or res.n_pairs == five_pairs), (res.found, five_found, res.n_pairs, five_pairs)
        stats = dbs["step"].debug_last_step()
        _lib.profile_begin(ctx)
        for _ in range(reps):
            step()
        prof = _lib.profile_end(ctx)
        kern = {k: prof[k][1] * 1e3 / reps for k in STEP_KERNELS if k in prof}
        out[verdict] = dict(five=t_five, step=t_step, stats=stats, kern=kern, n_pyr=res.n_pyramid, n_bow=res.n_bow, n_pairs=res.n_pairs)
        for db in dbs.values():
            db.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="150,500,2000")
    ap.add_argument("--stored", default="500,2000")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = ssvio_amd.Context(0)
    voc = make_vocabulary(k=10, L=4)
    V = svoc.Vocabulary.from_arrays(ctx, 10, 4, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    img = np.ascontiguousarray(make_stereo_pair(seed=0)[0])
    lines = ["# " + " ".join(["python", "tools/loop_keyframe_time.py"] + sys.argv[1:]),
             f"# commit: {a.commit or 'working tree'}; median (min) of {a.reps} runs after {a.warmup} warm-up runs, microseconds, one process; image {img.shape[1]}x{img.shape[0]}, {LEVELS} levels",
             "# five calls = describe_at + voc_transform + detect_loop + (match_features | kfdb_add); step = process_keyframe (+ add_pending when no loop)",
             "# kernels = HIP-event time of the step's launches per call, a run of their own; syncs / down = ssx_kfdb_debug_last_step",
             f"{'features':>8} {'stored':>6} {'verdict':>8} {'pyr kps':>7} {'words':>6} {'pairs':>6} {'five calls':>18} {'step':>18} {'five/step':>9} {'kernels':>8} {'syncs':>5} {'down B':>7}"]
    detail = []
    for nf in [int(s) for s in a.features.split(",")]:
        ex = orb.ORBextractor(ctx, nfeatures=nf)
        feats = np.ascontiguousarray(ex.Detect(img), dtype=KP_DTYPE)
        for ns in [int(s) for s in a.stored.split(",")]:
            r = case(ctx, V, ex, img, feats, ns, a.words, a.reps, a.warmup)
            for verdict, c in r.items():
                lines.append(f"{len(feats):>8} {ns:>6} {verdict:>8} {c['n_pyr']:>7} {c['n_bow']:>6} {c['n_pairs']:>6} {c['five'][0]:>9.1f} ({c['five'][1]:>6.1f}) "
                             f"{c['step'][0]:>9.1f} ({c['step'][1]:>6.1f}) {c['five'][0] / c['step'][0]:>8.2f}x {sum(c['kern'].values()):>8.1f} {c['stats']['syncs']:>5} "
                             f"{c['stats']['bytes_down']:>7}")
                print(lines[-1], flush=True)
                detail.append(f"# {len(feats):>5} features, {ns:>5} stored, {verdict:>7}: " + "  ".join(f"{k} {v:.1f}" for k, v in c["kern"].items()))
    text = "\n".join(lines + ["#", "# per-kernel HIP-event microseconds per step"] + detail) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    V.close()
    ctx.close()


if __name__ == "__main__":
    main()
