"""The keyframe step of loop closing for S streams: one ssx_kfdb_process_keyframe_batch call of S jobs against S calls of
ssx_kfdb_process_keyframe on S databases.

    python tools/loop_batch_time.py [--streams 1,8,32,64] [--features 200] [--stored 100] [--reps 30] [--warmup 5] [--runner 1] [--out FILE]

A KITTI-sized synthetic image (1241 x 376), --features features x 8 levels, a synthetic vocabulary of 10 000 words, databases of --stored
keyframes (the image's own keyframe under id 0, the others of about 1000 random words), asked once with the threshold of a revisit ("loop":
every job finds keyframe 0 and matches it) and once with a threshold no score reaches ("no loop").  Nothing is committed, so every
repetition sees the same databases.  The single calls run on one context and the batch call on another, each with its own copy of the
vocabulary and its own databases, so that neither re-plans the other's ORB workspace; both are called through ctypes with their arrays
prepared beforehand.  Host clock around calls that end in their synchronisation; per S the two alternate in the same process, --reps
repetitions after --warmup; median, quartiles and extremes in microseconds.

--runner 1: separately, ssx_run_kitti on the there-and-back drive of tools/loop_drive.py with loop closing on, --streams=32 unbatched against
--streams=32 --batched=1 --loop_batched=1: frames per second from the common start to the last stream's end."""
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ssvio_amd  # noqa: E402
from ssvio_amd import loop, orb, voc as svoc  # noqa: E402
from ssvio_amd._lib import KP_DTYPE, i32_p, u8_p  # noqa: E402
from tools.synth import make_stereo_pair, make_vocabulary  # noqa: E402

LEVELS = 8


def fill(ctx, n_stored, own, n_words, rng):
    db = loop.KeyframeDatabase(ctx, keyframes_hint=n_stored + 8)
    db.add(0, own["bow"], own["desc"], own["cls"])
    for i in range(1, n_stored):
        n = int(rng.integers(800, 1200))
        ids = np.sort(rng.choice(n_words, n, replace=False)).astype(np.int32)
        vals = rng.random(n) + 0.05
        db.add(i, (ids, vals / vals.sum()), own["desc"][:8], own["cls"][:8])
    return db


def spread(t):
    t = np.asarray(t) * 1e6
    return dict(med=float(np.median(t)), q1=float(np.percentile(t, 25)), q3=float(np.percentile(t, 75)), lo=float(t.min()), hi=float(t.max()))


def runner_frames_per_second(streams):
    from ssvio_amd import build
    from tools import loop_drive, synth
    exe = build.build_host()[1]
    out = {}
    with tempfile.TemporaryDirectory() as root:
        drive = loop_drive.make_loop_drive(root, n_leg=24, reach=7.0, right_factor=2.2, fx=450.0)
        voc = os.path.join(root, "voc.txt")
        synth.write_vocabulary_text(voc, synth.make_vocabulary(k=10, L=3))
        over = {"Loop.Closing.Open": 1, "Loop.Show.Closing.Result": 0, "Loop.Threshold.Heigher": 0.5, "Loop.Threshold.Lower": 0.02, "Pyramid.Level": 4,
                "Loop.Closig.Keyframe.Database.Min.Size": 3, "Loop.Min.Keyframe.Gap": 8, "DBOW2.VOC.Path": '"%s"' % voc}
        cfg = synth.write_settings(os.path.join(root, "cfg.yaml"), loop_drive.drive_settings(drive, over))
        for tag, extra in (("unbatched", ()), ("batched", ("--batched=1", "--loop_batched=1"))):
            r = subprocess.run([exe, "--config_yaml_path=" + cfg, "--kitti_dataset_path=" + drive["dir"], "--streams=%d" % streams, "--preload=1", *extra],
                               capture_output=True, text=True, timeout=400)
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            m = re.search(r"= ([0-9.]+) frames/s", r.stdout)
            loops = re.search(r"loop_calls (\d+) loop_jobs (\d+) loop_s ([0-9.]+)", r.stdout)
            out[tag] = (float(m.group(1)), loops.groups() if loops else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8,32,64")
    ap.add_argument("--features", type=int, default=200)
    ap.add_argument("--stored", type=int, default=100)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runner", type=int, default=1)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    Ss = [int(s) for s in a.streams.split(",")]
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
    n_in = len(pyr)
    res = loop.StepResult()
    o_pairs = np.zeros((n_in, 2), np.int32)
    lines = ["# " + " ".join(["python", "tools/loop_batch_time.py"] + sys.argv[1:]),
             f"# commit: {a.commit or 'working tree'}; image {img.shape[1]}x{img.shape[0]}, {len(feats)} features x {LEVELS} levels = {n_in} pyramid keypoints, "
             f"{len(own['cls'])} survive, {len(own['bow'][0])} words; databases of {a.stored} keyframes",
             f"# microseconds per S keyframe steps: median [quartiles] (min .. max) of {a.reps} repetitions after {a.warmup}, the two alternating in one process",
             "# single = S calls of ssx_kfdb_process_keyframe on S databases; batch = one ssx_kfdb_process_keyframe_batch of S jobs; launches / syncs: ssx_kfdb_debug_last_batch",
             f"{'S':>3} {'verdict':>8} {'single':>44} {'batch':>44} {'single/batch':>12} {'launches':>8} {'syncs':>5}"]
    fmt = lambda s: f"{s['med']:>9.1f} [{s['q1']:>8.1f} {s['q3']:>8.1f}] ({s['lo']:>8.1f} .. {s['hi']:>8.1f})"
    results = {}
    for verdict, threshold in (("no loop", 2.0), ("loop", 0.6)):
        for S in Ss:
            sd, bd = side["single"], side["batch"]
            prm = C.byref(sd["ex"].prm)

            def single():
                for db in sd["dbs"][:S]:
                    assert lib.ssx_kfdb_process_keyframe(db.handle, sd["V"].handle, 10 ** 6, img.ctypes.data_as(u8_p), img.strides[0], img.shape[0], img.shape[1], prm,
                                                         len(feats), feats.ctypes.data_as(C.c_void_p), LEVELS, 50, 20, threshold, n_in, o_pairs.ctypes.data_as(i32_p),
                                                         C.byref(res)) == 0
                    assert bool(res.found) == (verdict == "loop")

            jobs = [dict(db=db, kf_id=10 ** 6, image=img, features=feats, pairs_cap=n_in) for db in bd["dbs"][:S]]
            table, bres, status, keep, (rows, cols) = loop.step_job_table(jobs)

            def batch():
                assert lib.ssx_kfdb_process_keyframe_batch(bd["V"].handle, S, table, rows, cols, C.byref(bd["ex"].prm), LEVELS, 50, 20, threshold, 0) == 0
                assert all(bool(bres[j].found) == (verdict == "loop") and bres[j].n_pairs == res.n_pairs for j in range(S))

            ts, tb = [], []
            for rep in range(a.warmup + a.reps):
                t0 = time.perf_counter(); single(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
                if rep >= a.warmup:
                    ts.append(t1 - t0); tb.append(t2 - t1)
            st = loop.debug_last_batch(bd["ctx"])
            s, b = spread(ts), spread(tb)
            results[(verdict, S)] = (s, b)
            lines.append(f"{S:>3} {verdict:>8} {fmt(s)} {fmt(b)} {s['med'] / b['med']:>11.2f}x {st['launches']:>8} {st['syncs']:>5}")
            print(lines[-1], flush=True)
    lines.append("#")
    for verdict in ("no loop", "loop"):
        if (verdict, 32) in results:
            s, b = results[(verdict, 32)]
            lines.append(f"# condition 1, {verdict}: at S = 32 the batch call takes {b['med']:.1f} us against {s['med']:.1f} us of the 32 single calls: "
                         f"{'MET' if b['med'] < s['med'] else 'NOT MET'}")
        if (verdict, 1) in results:
            s, b = results[(verdict, 1)]
            tol = max(s["q3"] - s["q1"], b["q3"] - b["q1"])
            lines.append(f"# condition 2, {verdict}: at S = 1 the batch call takes {b['med']:.1f} us against {s['med']:.1f} us of the single call, the larger interquartile "
                         f"range is {tol:.1f} us: {'MET' if b['med'] <= s['med'] + tol else 'NOT MET'} (no slower beyond the measured spread)")
    if a.runner:
        r = runner_frames_per_second(32)
        lines += ["#", "# ssx_run_kitti, the there-and-back drive (47 stereo pairs of 320 x 200, a keyframe on every frame), loop closing inline, 32 streams, --preload=1:",
                  f"#   --streams=32                               {r['unbatched'][0]:>9.1f} frames/s",
                  f"#   --streams=32 --batched=1 --loop_batched=1  {r['batched'][0]:>9.1f} frames/s" +
                  (f"   (loop_calls {r['batched'][1][0]}, loop_jobs {r['batched'][1][1]}, {1e3 * float(r['batched'][1][2]):.1f} ms inside them)" if r["batched"][1] else "")]
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
